"""filter_throttle on the device (csrc/throttle.cpp through flbgpu_filter_throttle_create: the window on the host, the records found and
the first K of them copied on the device) against the recorded answers of the real plugin (tests/golden/throttle_ref_cases.json) and
against the CPU model (tests/throttle_model.py)."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import throttle_child as tch
import throttle_model as tm
from throttle_chunks import GROUP_START, T0, plain

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "throttle_ref_cases.json")))["cases"]


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case):
    steps = [(s[0], base64.b64decode(s[1]) if s[0] == "chunk" else s[1]) for s in case["steps"]]
    res, _ = tch.drive(g, "throttle", [tuple(p) for p in case["props"]], steps)
    assert res == [(s[2], base64.b64decode(s[3]) if s[3] is not None else None) for s in case["steps"] if s[0] == "chunk"]


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 300])
def test_first_k(g, k):
    """300 records (a group marker among them) against a window that has room for k: the first k go out; ticks between the calls"""
    n = 300
    rows = plain(n)
    data = b"".join(rows[:10]) + GROUP_START + b"".join(rows[10:])
    props = [("rate", str(max(k, 2))), ("window", "2")]                # room for 2 * rate records in the window
    room = 2 * max(k, 2)
    pre = room - k
    steps = [("tick", T0)] + ([("chunk", b"".join(plain(pre, 1000)))] if pre else []) + [("chunk", data), ("tick", T0 + 1), ("chunk", data), ("tick", T0 + 2), ("chunk", data)]
    res, (c, _) = tch.drive(g, "throttle", props, steps)
    ret, out = res[1 if pre else 0]
    assert (ret, out) == ((tm.MODIFIED, b"".join(rows[:k])) if k < n else (tm.NOTOUCH, None))
    assert c[0] == c[1] + c[2]

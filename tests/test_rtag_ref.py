"""The CPU model of filter_rewrite_tag (tests/rtag_model.py) against the answers of the real plugin that tools/gen_rtag_golden.py
recorded (tests/golden/rtag_ref_cases.json): cb_filter's return value, the output bytes and the list of (tag, bytes) the emitter was
handed, refusals included.  A case the real plugin did not start on must be refused by the model."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rtag_model as rm

CASES = json.load(open(os.path.join(HERE, "golden", "rtag_ref_cases.json")))["cases"]


def expected(case):
    """(ret, out, accepted emissions, refused emissions) as recorded"""
    em = [(base64.b64decode(t), base64.b64decode(b), r) for t, b, r in case["emitter"]]
    return (case["ret"], base64.b64decode(case["out"]) if case["out"] is not None else None,
            [(t, b) for t, b, r in em if not r], [(t, b) for t, b, r in em if r])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_real_plugin(case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused"):
        with pytest.raises(ValueError):
            rm.Model(props)
        return
    refused = []

    def refuse(i, tag, buf):
        if i in case["refuse"]:
            refused.append((tag, buf))
            return True
        return False
    m = rm.Model(props, base64.b64decode(case["tag"]), refuse)
    ret, out = m.filter(base64.b64decode(case["in"]))
    want = expected(case)
    assert (ret, out, m.emitted, refused) == want
    assert m.counters() == (len(want[2]), len(want[3]), 0, sum(len(t) for t, _ in want[2] + want[3]))


def test_the_recording_holds_what_the_pin_needs():
    by = {c["name"]: c for c in CASES}
    assert len(CASES) >= 100 and sum(1 for c in CASES if c.get("refused")) == 8
    # a group marker in front of a matched record travels with it (data + pre)
    c = by["call_group_marker_in_front_of_a_match"]
    ret, out, em, _ = expected(c)
    assert ret == 1 and len(em) == 2 and len(em[0][1]) > len(em[1][1])
    # emissions in front of undecodable bytes stand, the call answers NOTOUCH
    ret, out, em, _ = expected(by["call_trailing_garbage"])
    assert (ret, out) == (2, None) and len(em) == 2
    # everything emitted, nothing kept: MODIFIED with no bytes
    assert expected(by["call_all_matched_keep_false"])[:2] == (1, b"")
    # a refused emission keeps its record; with every emission refused the call is NOTOUCH
    ret, out, em, ref = expected(by["call_refused_in_the_middle"])
    assert ret == 1 and len(em) == 2 and len(ref) == 1 and ref[0][1] in out
    assert expected(by["call_all_refused"])[:3] == (2, None, [])
    # "%f" through the 32-byte buffer, a uint64 above 2^63-1, a duplicate key inside a map value, no region without groups
    assert expected(by["tpl_value_huge"])[2][0][0] == b"v.100000000000000005250476025520\x00.w"
    assert expected(by["tpl_value_big"])[2][0][0] == b"v.-1.w"
    assert expected(by["tpl_value_map"])[2][0][0].count(b'"k"') == 1
    assert expected(by["tpl_captures_no_groups"])[2][0][0] == b"|"
    assert len(expected(by["tpl_300_byte_tag"])[2][0][0]) == 300 and expected(by["tpl_empty_tag"])[2][0][0] == b""

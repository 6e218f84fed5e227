"""The call paths the lane-per-record filters share (csrc/filter_host.hpp): the counting pass, the pass again over the rows in front
of a record the decoder refuses, and the emit tail -- for modify, record_modifier, nest, type_converter, checklist, rewrite_tag,
expect and kubernetes alike (tests/filter_paths.py has their programs), each against its CPU model (tests/*_model.py): output bytes,
return value, flbgpu_filter_last_counts and the filter's own counters.  Every filter runs one configuration that changes every good record, on 130 records: two full waves and two records, so the
partial wave at the end is there.  After each case the same filter object takes the all-good chunk: a pass over the first `fb` rows
must leave nothing behind in the length column or the counter words."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
from filter_paths import BAD, FILTERS, good, make, same
import synth

pytestmark = pytest.mark.gpu
N = 130
GOOD = [good(i) for i in range(N)]
ALL = b"".join(GOOD)


def bad_at(p):
    return b"".join(GOOD[:p]) + BAD + b"".join(GOOD[p + 1:])


CASES = [("none", b""), ("one", GOOD[0]), ("all", ALL)] + [("bad%d" % p, bad_at(p)) for p in (0, 1, 63, 64, 65, 129)] + [
    ("garbage", ALL + good(N)[:4])]


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


@pytest.mark.parametrize("case", [c[0] for c in CASES])
@pytest.mark.parametrize("name", list(FILTERS))
def test_call_paths(g, name, case, tmp_path):
    f, m = make(g, name, tmp_path)
    try:
        same(name, f, m, dict(CASES)[case])
        # the same object again: every record is changed, whatever the call in front left behind
        ret, out = same(name, f, m, ALL)
        assert ret == g.MODIFIED and f.counts()[0] == N
        assert len(synth.unpack_all(out)) == (0 if name == "rewrite_tag" else N)
    finally:
        f.close()

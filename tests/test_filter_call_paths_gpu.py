"""The call paths the lane-per-record filters share (csrc/filter_host.hpp): the counting pass, the pass again over the rows in front
of a record the decoder refuses, and the emit tail -- for modify, record_modifier, nest, type_converter, checklist and rewrite_tag
alike, each against its CPU model (tests/*_model.py): output bytes, return value, flbgpu_filter_last_counts and the filter's own
counters.  Every filter runs one configuration that changes every good record, on 130 records: two full waves and two records, so the
partial wave at the end is there.  After each case the same filter object takes the all-good chunk: a pass over the first `fb` rows
must leave nothing behind in the length column or the counter words."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import checklist_model as cm
import modify_model as mm
import nest_model as nm
import recmod_model as rcm
import rtag_model as rm
import typeconv_model as tm
from checklist_chunks import third_list
from modify_chunks import rec
from nest_chunks import N1
from rtag_chunks import P1
from typeconv_chunks import P4
import synth

pytestmark = pytest.mark.gpu
N = 130
# modify: every record gets a key; record_modifier: every record loses one and gets one; nest: `host` moves under a new map;
# type_converter: `status` converts in every record; checklist: every `code` is on the list (exact mode); rewrite_tag: every `log`
# matches, and the rule does not keep the record
FILTERS = {
    "modify": ("FilterModify", mm.Model, [("Set", "k x")]),
    "record_modifier": ("FilterRecordModifier", rcm.Model, [("Record", "hostname h"), ("Remove_key", "agent")]),
    "nest": ("FilterNest", nm.Model, N1),
    "type_converter": ("FilterTypeConverter", tm.Model, P4),
    "checklist": ("FilterChecklist", cm.Model, [("lookup_key", "code"), ("record", "flag new"), ("record", "hit true")]),
    "rewrite_tag": ("FilterRewriteTag", rm.Model, P1),
}


def good(i):
    body = synth.KV([(b"log", b"an error in line %d" % i), (b"host", b"h%d" % (i % 9)), (b"agent", b"a" * (i % 23)), (b"status", b"%d" % (200 + i)),
                     (b"size", 1000 + i), (b"code", b"hit-%d" % (i % 7))])
    return rec(body, 1700000000 + i, i)


GOOD = [good(i) for i in range(N)]
ALL = b"".join(GOOD)
BAD = rec("not a map", 1, 0)


def bad_at(p):
    return b"".join(GOOD[:p]) + BAD + b"".join(GOOD[p + 1:])


CASES = [("none", b""), ("one", GOOD[0]), ("all", ALL)] + [("bad%d" % p, bad_at(p)) for p in (0, 1, 63, 64, 65, 129)] + [
    ("garbage", ALL + good(N)[:4])]


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def same(f, m, data):
    got, want = f.filter(data), m.filter(data)
    assert got == want, (got[0], want[0])
    assert f.counts() == m.counts()
    if hasattr(m, "counters"):
        assert f.counters() == m.counters()
    if hasattr(m, "emitted"):
        assert f.emitted() == m.emitted
    return got


@pytest.mark.parametrize("case", [c[0] for c in CASES])
@pytest.mark.parametrize("name", list(FILTERS))
def test_call_paths(g, name, case, tmp_path):
    cls, model, props = FILTERS[name]
    if name == "checklist":
        path = str(tmp_path / "list.txt")
        with open(path, "wb") as fh:
            fh.write(third_list(False))
        props = [("file", path)] + props
    f, m = getattr(g, cls)(props), model(props)
    try:
        same(f, m, dict(CASES)[case])
        # the same object again: every record is changed, whatever the call in front left behind
        ret, out = same(f, m, ALL)
        assert ret == g.MODIFIED and f.counts()[0] == N
        assert len(synth.unpack_all(out)) == (0 if name == "rewrite_tag" else N)
    finally:
        f.close()

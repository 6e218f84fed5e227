"""What tests/test_filter_call_paths_gpu.py and tests/lane_stride_child.py share: one configuration per lane-per-record filter that
changes every good record, the records, the undecodable record, and the comparison with the CPU models (tests/*_model.py)."""
import checklist_model as cm
import expect_model as em
import kube_model as km
import modify_model as mm
import nest_model as nm
import recmod_model as rcm
import rtag_model as rm
import typeconv_model as tm
from checklist_chunks import third_list
from kube_chunks import blob_of
from modify_chunks import rec
from nest_chunks import N1
from rtag_chunks import P1
from typeconv_chunks import P4
import synth

# modify: every record gets a key; record_modifier: every record loses one and gets one; nest: `host` moves under a new map;
# type_converter: `status` converts in every record; checklist: every `code` is on the list (exact mode); rewrite_tag: every `log`
# matches, and the rule does not keep the record; expect: a rule that fails nowhere under result_key, so every record is rebuilt;
# kubernetes: merge_log finds no JSON in `log`, every record is rebuilt with the pod's map behind it
FILTERS = {
    "modify": ("FilterModify", mm.Model, [("Set", "k x")]),
    "record_modifier": ("FilterRecordModifier", rcm.Model, [("Record", "hostname h"), ("Remove_key", "agent")]),
    "nest": ("FilterNest", nm.Model, N1),
    "type_converter": ("FilterTypeConverter", tm.Model, P4),
    "checklist": ("FilterChecklist", cm.Model, [("lookup_key", "code"), ("record", "flag new"), ("record", "hit true")]),
    "rewrite_tag": ("FilterRewriteTag", rm.Model, P1),
    "expect": ("FilterExpect", em.Model, [("key_exists", "$log"), ("action", "result_key"), ("result_key", "ok")]),
    "kubernetes": ("FilterKubernetes", km.Model, [("merge_log", "on")]),
}
MODIFIED, NOTOUCH = km.Model.MODIFIED, km.Model.NOTOUCH


def good(i):
    body = synth.KV([(b"log", b"an error in line %d" % i), (b"host", b"h%d" % (i % 9)), (b"agent", b"a" * (i % 23)), (b"status", b"%d" % (200 + i)),
                     (b"size", 1000 + i), (b"code", b"hit-%d" % (i % 7))])
    return rec(body, 1700000000 + i, i)


BAD = rec("not a map", 1, 0)


def make(g, name, tmp_path):
    """the filter `name` on the device and its model, set up alike"""
    cls, model, props = FILTERS[name]
    if name == "checklist":
        path = str(tmp_path / "list.txt")
        with open(path, "wb") as fh:
            fh.write(third_list(False))
        props = [("file", path)] + props
    f, m = getattr(g, cls)(props), model(props)
    if name == "kubernetes":
        pod = blob_of(37)
        f.set_meta(pod, None)
        m.set_meta(pod, None)
    return f, m


def holds_a_record(name, data):
    try:
        if name == "expect":
            mm.decode_event(data, 0)
        else:
            mm.unpack(data, 0)
        return True
    except mm.Bad:
        return False


def same(name, f, m, data):
    got, want = f.filter(data), m.filter(data)
    # a chunk that holds no whole record never reaches a filter of this library: the call answers NOTOUCH where the reference's
    # expect and kubernetes hand back an empty buffer (tests/test_expect_gpu.py and tests/test_kube_gpu.py say the same)
    if name in ("expect", "kubernetes") and want == (MODIFIED, b"") and not holds_a_record(name, data):
        want = (NOTOUCH, None)
    assert got == want, (got[0], want[0])
    assert f.counts() == m.counts()
    if hasattr(m, "counters"):
        assert f.counters() == m.counters()
    if hasattr(m, "emitted"):
        assert f.emitted() == m.emitted
    return got

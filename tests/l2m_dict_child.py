"""The dictionary cases of tests/test_l2m_edges_gpu.py that need FLBGPU_L2M_INIT_CAP / FLBGPU_L2M_INIT_ARENA (read once per process): one
process per setting, started by the test with the setting's environment.  Every scenario compares whole snapshots with
oracle_binding.L2M and prints "OK <setting>" at the end."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import flbamd_loader
import l2m_chunks as lc
import oracle_binding as ob
from synth import v2_record
from test_grep_pair_gpu import _upload

g = flbamd_loader.load()
g.init(0)
# a plain label name takes k_l2m_lane, a nested one k_l2m_extract: both insert through l2m_series_id_lv
SHAPES = [([("label_field", "k")], lambda k: v2_record(1, 0, {"k": k})), ([("add_label", "k $m['k']")], lambda k: v2_record(1, 0, {"m": {"k": k}}))]


def run(props, chunks):
    """-> (stats of the device filter); the snapshots of both sides are equal, label order included"""
    o, f = ob.L2M("counter", props), g.FilterLogToMetrics("counter", props)
    for c in chunks:
        if isinstance(c, lc.RowChunk):
            chunk, bufs, blob = _upload(g, c.rows)
            assert o.filter(c) == f.filter_dev(chunk)[0]
            g.lib().flbgpu_dev_free(bufs[0]); g.lib().flbgpu_dev_free(bufs[1])
        else:
            assert o.filter(c) == f.filter(c)[0]
    a, b = f.snapshot(), o.snapshot()[2]
    assert [(x["labels"], x["value"]) for x in a] == [(x["labels"], x["value"]) for x in b], (a[:20], b[:20])
    st = f.stats()
    f.close()
    return a, st


def cap16():
    """12 .. 17 keys into 16 slots, which hold 8 series: 8 keys fill the dictionary exactly (no growth), the 9th grows it; two of the
    first keys have the last slot as their home, so the probe sequence wraps at cap_mask"""
    assert os.environ["FLBGPU_L2M_INIT_CAP"] == "16"
    keys = lc.wrap_keys(16)
    assert [lc.home_slot(k, 16) for k in keys[:2]] == [15, 15]
    for props, rec in SHAPES:
        for nk in (2, 7, 8, 9, 12, 13, 14, 15, 16, 17):
            ks = keys[:nk]
            data = b"".join(rec(ks[(i * 5) % nk]) for i in range(3 * nk)) + b"".join(rec(k) for k in ks)
            a, st = run(props, [data, data])
            assert len(a) == nk, (nk, len(a))
            if nk <= 8:
                assert st["grows"] == 0 and st["slots"] == 16, (nk, st)            # max_series is reached exactly at 8
            else:
                assert st["grows"] >= 1 and st["slots"] >= 32, (nk, st)


def arena():
    """the arena holds exactly the padded keys of the first call (no growth), and is 8 bytes short of them (one growth)"""
    assert os.environ["FLBGPU_L2M_INIT_ARENA"] == "64"
    fit = [b"a" * 15, b"b" * 15, b"c" * 9, b"e" * 7, b"f"]                               # 16 + 16 + 16 + 8 + 8 = 64
    assert sum(lc.padded(k) for k in fit) == 64
    for props, rec in SHAPES:
        data = b"".join(rec(fit[(i * 3) % len(fit)]) for i in range(200))
        a, st = run(props, [data, data])
        assert len(a) == len(fit) and st["grows"] == 0, st
        more = fit + [b"g" * 3]
        assert sum(lc.padded(k) for k in more) == 64 + 8
        data = b"".join(rec(more[(i * 5) % len(more)]) for i in range(200))
        a, st = run(props, [data, data])
        assert len(a) == len(more) and st["grows"] == 1, st


def phantom(grow):
    """rows behind a row that does not decode may enter their key into the dictionary: the entry is hidden until a record really
    touches it, and then takes the place of its real first appearance (a, b, zz); with a small table the second call also grows the
    dictionary, so k_l2m_rehash re-enters the hidden entry with the others"""
    for props, rec in SHAPES:
        first = lc.row_chunk([rec("a")] * 100 + [lc.BAD] + [rec("zz")] * 5)
        second = b"".join([rec("b"), rec("zz")] + ([rec("g%d" % i) for i in range(12)] if grow else []))
        o, f = ob.L2M("counter", props), g.FilterLogToMetrics("counter", props)
        chunk, bufs, blob = _upload(g, first.rows)
        assert o.filter(first) == f.filter_dev(chunk)[0]
        g.lib().flbgpu_dev_free(bufs[0]); g.lib().flbgpu_dev_free(bufs[1])
        assert [(x["labels"], x["value"]) for x in f.snapshot()] == [((b"a",), 100.0)]       # hidden
        grows0 = f.stats()["grows"]
        assert o.filter(second) == f.filter(second)[0]
        a, b = f.snapshot(), o.snapshot()[2]
        assert [(x["labels"], x["value"]) for x in a] == [(x["labels"], x["value"]) for x in b]
        assert [x["labels"][0] for x in a[:3]] == [b"a", b"b", b"zz"] and [x["value"] for x in a[:3]] == [100.0, 1.0, 1.0]
        if grow:
            assert os.environ["FLBGPU_L2M_INIT_CAP"] == "16" and f.stats()["grows"] > grows0 and len(a) == 15, f.stats()
        f.close()


if __name__ == "__main__":
    what = sys.argv[1]
    {"cap16": cap16, "arena": arena, "phantom": lambda: phantom(False), "phantom_grow": lambda: phantom(True)}[what]()
    print("OK " + what)

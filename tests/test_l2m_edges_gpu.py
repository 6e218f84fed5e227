"""filter_log_to_metrics' extract, stale, aggregate and dictionary kernels (csrc/l2m_kernels.inc, csrc/l2m_dev.inc) on the named cases of
tests/l2m_chunks.py (tests/test_l2m_chunks.py proves on the CPU that each case sits on its edge and that the models are the oracle's).

Columns go through the test aids flbgpu_l2m_stale_dev / flbgpu_l2m_aggregate_dev and are compared with the plain models WORD FOR WORD,
every word of every row after every call of a chain, no tolerance; after a chain every row also goes through flbgpu_l2m_finalize_row
and is compared with the rounding model bit for bit.  The grid-stride cases are built from the device's CU count.

Records go through FilterLogToMetrics against oracle_binding.L2M with check() of tests/test_l2m_gpu.py; the filter's profile has to
name the kernel the case is for (a nested label name forces k_l2m_extract without host rules; a float label defers to k_l2m_generic).

The dictionary cases that need a small table or arena run in a child process per setting (tests/l2m_dict_child.py): the settings are
read once per process.  The cap-16 sweep keeps the wrap predicate -- restating l2m_mix and the FNV stream is a few lines
(l2m_chunks.key_hash): two of the first keys have slot 15 as their home, so one must wrap at cap_mask whatever the order."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import flbamd_loader
import l2m_chunks as lc
from synth import v2_record
from test_grep_pair_gpu import _upload
from test_l2m_gpu import check
from test_lane_edges_gpu import Profiled

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


@pytest.fixture(scope="module")
def cus(g):
    n = int(g.lib().flbgpu_device_cus())
    assert n > 0
    return n


@pytest.fixture(scope="module")
def agg(cus):
    return lc.agg_cases(cus)


def same_f64(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b) or (math.isnan(a) and math.isnan(b))


def first_diff(a, b):
    d = np.argwhere(a != b)
    return None if len(d) == 0 else (tuple(int(x) for x in d[0]), int(a[tuple(d[0])]), int(b[tuple(d[0])]), len(d))


def run_all(cases, one):
    """every case runs; the names of those that fail are what the assertion shows"""
    failed = []
    for c in cases:
        try:
            one(c)
        except AssertionError as e:
            failed.append((c.name, str(e)[:300]))
    assert not failed, "%d of %d cases failed: %s" % (len(failed), len(cases), failed[:12])


# ------------------------------------------------------------------------------------------ columns: the stale scan
def stale_one(g, c):
    sid, val = g.l2m_stale_dev(c.sid, c.val, c.first_bad)
    wsid, wval = lc.stale_model(c.sid, c.val, c.first_bad)
    assert np.array_equal(sid, wsid), ("sid", first_diff(sid, wsid))
    assert np.array_equal(val, wval), ("val", first_diff(val, wval))
    keep = c.sid < lc.STALE                                    # an assigning row is never rewritten
    assert np.array_equal(sid[keep], c.sid[keep]) and np.array_equal(val[keep], c.val[keep])


@pytest.mark.parametrize("part", ["small", "spine"])
def test_stale_columns(g, part):
    cs = [c.check() for c in lc.stale_cases() if (c.n > 100 * lc.L2M_ST_TILE) == (part == "spine")]
    assert len(cs) >= 6
    run_all(cs, lambda c: stale_one(g, c))


# ------------------------------------------------------------------------------------------ columns: the aggregation
def agg_one(g, c):
    m = lc.AggModel(c.mode, c.nseries, c.bounds)
    rows = np.zeros((c.nseries, lc.row_words(c.mode, len(c.bounds))), dtype=np.uint64)
    for k, (sid, val, fb, base) in enumerate(c.calls):
        rows = g.l2m_aggregate_dev(c.mode, sid, val, rows, first_bad=fb, idx_base=base, bounds=c.bounds)
        m.call(sid, val, fb, base)
        want = m.rows()
        assert np.array_equal(rows, want), ("call", k, first_diff(rows, want))
    finalize_all(g, c.mode, len(c.bounds), rows, m)


def finalize_all(g, mode, nb, rows, m):
    for s in range(min(len(rows), 2000)):
        d, f = g.finalize_row(mode, nb, rows[s]), m.final(s)
        if mode != lc.HISTOGRAM:
            assert same_f64(d["value"], f["value"]), (s, d, f)
        else:
            assert d["buckets"] == f["buckets"] and d["count"] == f["count"] and same_f64(d["sum"], f["sum"]), (s, d, f)


@pytest.mark.parametrize("mode", [lc.COUNTER, lc.GAUGE, lc.HISTOGRAM], ids=["counter", "gauge", "histogram"])
def test_aggregate_columns(g, agg, mode):
    cs = [c.check() for c in agg if c.mode == mode and "/chain/" not in c.name and "more_words" not in c.name]
    assert len(cs) >= 14
    run_all(cs, lambda c: agg_one(g, c))


def test_aggregate_chains_and_their_rounding(g, agg):
    cs = [c.check() for c in agg if "/chain/" in c.name]
    assert len(cs) >= 15
    run_all(cs, lambda c: agg_one(g, c))


def test_aggregate_more_words_than_combiner_slots(g, agg):
    cs = [c.check() for c in agg if "more_words" in c.name]
    assert len(cs) == 1
    run_all(cs, lambda c: agg_one(g, c))


def test_gauge_keeps_a_series_whose_last_index_lies_behind_the_call(g):
    c = lc.gauge_later_range_case().check()
    m = lc.AggModel(lc.GAUGE, 2)
    m.first[1], m.last[1], m.lastval[1] = 5, int(c.rows[1, lc.L2M_W_LASTIDX]), int(c.rows[1, lc.L2M_W_LASTVAL])
    assert np.array_equal(m.rows(), c.rows)
    rows = g.l2m_aggregate_dev(lc.GAUGE, c.sid, c.val, c.rows, idx_base=c.idx_base)
    m.call(c.sid, c.val, lc.NOBAD, c.idx_base)
    assert np.array_equal(rows, m.rows()), first_diff(rows, m.rows())
    assert lc.b2f(rows[1, lc.L2M_W_LASTVAL]) == 7.25 and lc.b2f(rows[0, lc.L2M_W_LASTVAL]) == 4.0


def test_gauge_last_writer_is_a_stale_row(g):
    """the stale scan's output into the aggregation: the row that wins the gauge took its value from another series' row"""
    B = lc.L2M_AGG_BLOCK
    sid = np.full(2 * B + 3, lc.NONE, dtype=np.uint32)
    val = (np.arange(len(sid), dtype=np.float64) + 0.5).view(np.uint64)
    sid[0], sid[1], sid[B - 1], sid[B], sid[2 * B + 2], sid[2 * B + 1] = 0, 1, 2, 0 | lc.STALE, 1 | lc.STALE, lc.DEFER
    s1, v1 = g.l2m_stale_dev(sid, val)
    w1, wv1 = lc.stale_model(sid, val)
    assert np.array_equal(s1, w1) and np.array_equal(v1, wv1)
    rows = g.l2m_aggregate_dev(lc.GAUGE, s1, v1, np.zeros((3, 4), dtype=np.uint64))
    m = lc.AggModel(lc.GAUGE, 3)
    m.call(w1, wv1)
    assert np.array_equal(rows, m.rows()), first_diff(rows, m.rows())
    assert [lc.b2f(x) for x in rows[:, lc.L2M_W_LASTVAL]] == [B - 1 + 0.5, B - 1 + 0.5, B - 1 + 0.5]


def test_aggregate_aid_refuses_an_id_beyond_the_rows(g):
    with pytest.raises(RuntimeError):
        g.l2m_aggregate_dev(lc.COUNTER, np.array([0, 2], dtype=np.uint32), None, np.zeros((2, 4), dtype=np.uint64))
    rows = g.l2m_aggregate_dev(lc.COUNTER, np.array([0, 2], dtype=np.uint32), None, np.zeros((2, 4), dtype=np.uint64), first_bad=1)
    assert rows[0, lc.L2M_W_COUNT] == 1 and not rows[1].any()


# ------------------------------------------------------------------------------------------ records
class Prof(Profiled):
    """Profiled, and a RowChunk goes in as a device chunk with its rows"""

    def FilterLogToMetrics(self, *a, **kw):
        f = Profiled.FilterLogToMetrics(self, *a, **kw)
        host, g = f.filter, self.g

        def filt(c):
            if not isinstance(c, lc.RowChunk):
                return host(c)
            chunk, bufs, blob = _upload(g, c.rows)
            try:
                return f.filter_dev(chunk)[0], b""
            finally:
                g.lib().flbgpu_dev_free(bufs[0]); g.lib().flbgpu_dev_free(bufs[1])
        f.filter = filt
        return f


def rcheck(g, mode, props, chunks, ran="k_l2m_extract", not_ran="k_l2m_lane"):
    pg = Prof(g)
    s, st = check(pg, mode, props, chunks, value_field=None if mode == "counter" else "v")
    assert len(pg.seen) == 1 and ran in pg.seen[0] and (not_ran is None or not_ran not in pg.seen[0]), pg.seen
    return s, st


@pytest.mark.parametrize("family", ["fit", "single", "chunk_end", "rows"])
def test_extract_staging(g, family):
    cs = {"fit": lc.extract_fit_cases, "single": lc.extract_single_cases, "chunk_end": lc.extract_end_cases, "rows": lc.extract_count_cases}[family]()
    assert len(cs) >= 7
    run_all([c.check() for c in cs], lambda c: rcheck(g, c.mode, c.props, [c.data]))
    if family == "single":
        # the small records on both sides of the records read in place are all counted
        c = [c for c in cs if c.name.endswith("lane_20_21")][0]
        s, _ = rcheck(g, "counter", c.props, [c.data])
        assert sum(x["value"] for x in s) == len(c.recs) and {x["labels"] for x in s} >= {(b"over20",), (b"over21",)}


def test_extract_second_trip(g, cus):
    c = lc.second_trip_rows(cus).check()
    s, _ = rcheck(g, "counter", c.props, [c.data])
    assert s[-1]["labels"] == (b"2nd",) and s[-1]["value"] == 65.0 and sum(x["value"] for x in s) == len(c.recs)


def test_extract_on_device_chunks(g, cus):
    cs = [c.check() for c in lc.extract_dev_cases(cus)]
    assert len(cs) == 6
    run_all(cs, lambda c: rcheck(g, c.mode, c.props, c.chunks))
    # the rows behind the one that does not decode never ran: their series does not exist, the call after them counts
    c = cs[-1]
    s, _ = rcheck(g, "counter", c.props, c.chunks)
    assert (b"never",) not in {x["labels"] for x in s} and {(b"g",), (b"h",)} <= {x["labels"] for x in s}
    assert sum(x["value"] for x in s) == 2 * cus * lc.L2M_BLOCK - 1 + 2


def test_generic_second_trip(g):
    c = lc.generic_case().check()
    s, st = rcheck(g, c.mode, c.props, [c.data], ran="k_l2m_generic", not_ran=None)
    assert st["deferred"] == len(c.recs)
    assert [(x["labels"], x["value"]) for x in s][-1] == ((b"2.500000",), 64.0) and sum(x["value"] for x in s) == len(c.recs)


@pytest.mark.parametrize("props,ran", [([("label_field", "k")], "k_l2m_lane"), ([("add_label", "k $m['k']")], "k_l2m_extract")], ids=["lane", "extract"])
def test_dictionary_one_wave_inserts_one_key(g, props, ran):
    """64 lanes of the first wave insert the same new key, the next 64 a key each"""
    rec = (lambda k: v2_record(1, 0, {"k": k})) if ran == "k_l2m_lane" else (lambda k: v2_record(1, 0, {"m": {"k": k}}))
    data = b"".join([rec("same")] * 64 + [rec("d%d" % i) for i in range(64)])
    s, _ = rcheck(g, "counter", props, [data, data], ran=ran, not_ran=None)
    assert len(s) == 65 and s[0]["value"] == 128.0 and all(x["value"] == 2.0 for x in s[1:])


@pytest.mark.parametrize("setting", ["cap16", "arena", "phantom", "phantom_grow"])
def test_dictionary_in_a_child_process(g, setting):
    env = dict(os.environ)
    env.update({"cap16": {"FLBGPU_L2M_INIT_CAP": "16"}, "arena": {"FLBGPU_L2M_INIT_ARENA": "64"}, "phantom": {},
                "phantom_grow": {"FLBGPU_L2M_INIT_CAP": "16"}}[setting])
    r = subprocess.run([sys.executable, os.path.join(HERE, "l2m_dict_child.py"), setting], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK " + setting in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]

"""The one-pass lane kernels (csrc/jlane_kernels.inc k_json_lane, glane_kernels.inc k_grep_lane, l2mlane_kernels.inc k_l2m_lane; lane_dev.inc,
lookback.inc) at their staging, walk and copy edges, bit-exact against the CPU references: jsonfuzz.oracle() row by row,
oracle_binding.Grep (return code, bytes, counts), oracle_binding.L2M through test_l2m_gpu.check().

Every row of these kernels has a second answer (k_json_rows / k_json_generic; decode_event / grep_decide / l2m_record), so bytes alone
prove nothing about the lane path: the JSON cases assert JsonPacker.tile_stats() against the `taken` flag each case carries (written by
hand in tests/lane_chunks.py), the grep and log_to_metrics cases assert the kernel's name in the filter's profile on chunks whose
records are of the shape the lean walk takes (tests/test_lane_chunks.py proves the shapes on the CPU).  The look-back's second window
(more than 256 units in front) is made reachable by the large chunks; whether a workgroup takes it depends on timing and is not asserted."""
import numpy as np
import pytest
import jsonfuzz as jf
import oracle_binding as ob
import flbamd_loader
import lane_chunks as lc
from synth import v2_record, Raw
from test_gpu_parity import first_diff, oracle_chain
from test_grep_pair_gpu import _upload, _download
from test_l2m_gpu import check

pytestmark = pytest.mark.gpu
CASES = lc.json_cases()


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


@pytest.fixture(autouse=True)
def _no_ahead_launch(monkeypatch):
    # (a small chunk is otherwise launched ahead of its sizes, which keeps the three-launch kernels: test_grep_pair_gpu.py)
    monkeypatch.setenv("FLBGPU_NO_SPEC", "1")


# ---------------------------------------------------------------------------------------------------------------- JSON
_WANT = {}
_ORACLE = []


def want(row):
    """the reference's answer for a row, kept by the row's bytes (the families repeat a few rows many times)"""
    w = _WANT.get(row)
    if w is None:
        if not _ORACLE:
            _ORACLE.append(jf.oracle())
        w = _ORACLE[0](row)
        one = w[0] == 0 and w[3] == 1 and w[2] == 1 and row[w[4]:].strip(b" \t\r\n") == b""
        w = _WANT[row] = (w, v2_record(lc.TS[0], lc.TS[1], Raw(w[1])) if one else b"")
    return w


def run_json(g, rows, events, what=""):
    p = g.JsonPacker()
    outs, rec, cons, rt, st = p.run_host(rows, events=events, ts=lc.TS)
    ts = p.tile_stats()
    p.close()
    for i, r in enumerate(rows):
        w, ev = want(r)
        if events:
            assert outs[i] == ev, (what, i, r[:100], outs[i][:60], ev[:60])
        elif w[0] != 0:
            assert st[i] == 1 and outs[i] == b"", (what, i, r[:100], st[i], outs[i][:40])
        else:
            assert st[i] == 0 and (0, outs[i], int(rt[i]), int(rec[i]), int(cons[i])) == w, (what, i, r[:100], outs[i][:60], w[1][:60], rt[i], rec[i], cons[i], w[2:])
    return ts


def json_both(g, rows, left, what=""):
    for events in (False, True):
        ts = run_json(g, rows, events, what)
        print(what, "events" if events else "msgpack", ts)
        assert ts["left_rows"] == left and ts["tile_rows"] == len(rows) - left, (what, events, left, ts)
        if left == 0:
            assert ts["launches"] == 1, (what, ts)


@pytest.mark.parametrize("family", sorted(CASES))
def test_json_case(g, family):
    """B: the in-place rewrite.  Each case row three times (first, middle, last of a tile) among a service's log lines; the rows the
    pass leaves are exactly the copies of a case whose `taken` is False -- a flag wrong in either direction fails"""
    for c in CASES[family]:
        rows, pos = lc.json_case_chunk(c)
        json_both(g, rows, 0 if c.taken else len(pos), "%s/%s (%s)" % (family, c.name, c.cond))


@pytest.mark.parametrize("align", [0, 5, 15])
def test_json_tile_fits_exactly(g, align):
    """A.1: 64 rows from a tile's first row whose combined length goes through the wave's 15 872 bytes a byte at a time"""
    sweep = lc.json_fit_sweep(align)
    lefts = []
    for T, rows, left in sweep:
        ts = run_json(g, rows, True, "total %d" % T)
        lefts.append(ts["left_rows"])
        assert run_json(g, rows, False, "total %d" % T)["left_rows"] == lefts[-1]
    print(lefts)
    assert lefts == sorted(lefts) and lefts[0] == 0 and lefts[-1] >= 1
    assert lefts == [left for _, _, left in sweep]                       # the tile that ends AT the capacity fits


@pytest.mark.parametrize("L", [16001, 40000])
def test_json_row_longer_than_a_wave(g, L):
    """A.2: the long row and every row behind it in its tile are left, the tiles around it are taken whole"""
    for where in (0, 31, 63):
        rows, left = lc.json_too_long(L, where)
        json_both(g, rows, left, "%d bytes at %d" % (L, where))


@pytest.mark.parametrize("L,n", [(400, 77), (400, 130), (3000, 9), (14000, 3), (14000, 2), (100, 2), (100, 3)])
def test_json_fewer_rows_to_a_tile(g, L, n):
    """A.3: R in the thirties, 4 and 1; a partial last tile; a last workgroup with a wave that has no tile; the smallest chunks the pass takes"""
    json_both(g, lc.json_uniform(L, n), 0, "%d rows of %d" % (n, L))


def test_json_alignment_and_the_end_of_the_data(g):
    """A.4: a tile's first row at every residue of a 16-byte address, the data's end at every residue (the partial-sixteen staging)"""
    for a in range(16):
        for e in range(16):
            rows, left = lc.json_align(a, e)
            json_both(g, rows, left, "align %d end %d" % (a, e))
    for e in range(16):
        for tail in ("no_newline", "open_string"):
            rows, left = lc.json_align(5, e, tail)
            json_both(g, rows, left, "end %d %s" % (e, tail))


def test_json_more_units_than_a_look_back_window(g):
    """A.6: 40 000 rows are 313 workgroups' units; the rows' places are the running sum of their lengths (run_host cuts the output there)"""
    rows = lc.json_big()
    left = sum(1 for r in rows if b"\\u" in r)
    json_both(g, rows, left, "40000 rows")


# ---------------------------------------------------------------------------------------------------------------- filter_grep
class Grep:
    """one filter_grep on the device and in the oracle, for many chunks"""

    def __init__(self, g, rules, op=None):
        self.g, self.rules, self.op = g, rules, op
        self.f, self.o = g.FilterGrep(rules, op), ob.Grep(rules, op)
        self.f.profile(True)

    def run(self, recs, lane=True, what=""):
        g = self.g
        chunk, bufs, blob = _upload(g, recs)
        try:
            ret, out = self.f.filter_dev(chunk)
            wret, wout = self.o.filter(blob)
            what = (what, self.rules[:3], self.op)
            assert ret == wret, (what, ret, wret, g.last_error())
            if lane:
                assert "k_grep_lane" in self.f.profile_read(), (what, self.f.profile_read())
            if ret != g.MODIFIED:
                return ret, None, None
            got, off = _download(g, out)
            assert got == wout, (what, first_diff(wout, got))
            assert self.f.counts() == (ob.count_records(blob), ob.count_records(wout)), what
            return ret, got, off
        finally:
            g.lib().flbgpu_dev_free(bufs[0]); g.lib().flbgpu_dev_free(bufs[1])

    def close(self):
        self.f.close()


def grep_once(g, recs, rules, op=None, lane=True, what=""):
    q = Grep(g, rules, op)
    try:
        return q.run(recs, lane, what)
    finally:
        q.close()


def all_fit(recs):
    return all(lc.fits(recs, lc.grep_geometry)[0])


def test_grep_tile_fits_exactly(g):
    """A.1: one record of a tile grows until the tile's last records miss the wave's LDS; they are decided and copied from the chunk"""
    q = Grep(g, *lc.A_RULES)
    for over, recs in lc.fit_sweep(lc.grep_geometry):
        assert q.run(recs, what="over %d" % over)[0] == g.MODIFIED
    q.close()


@pytest.mark.parametrize("L", [16001, 16015, 40000])
def test_grep_record_longer_than_a_wave(g, L):
    """A.2: the `!have` decision on the chunk itself and the 16-bytes-a-lane copy from the chunk with its byte tail"""
    q = Grep(g, *lc.A_RULES)
    for behind in (0, 1, 5, 60, 63):
        for keep in (True, False):
            recs, at = lc.too_long(L, behind, keep)
            ret, got, off = q.run(recs, what="%d bytes, %d behind, kept %s" % (L, behind, keep))
            assert ret == g.MODIFIED and int(off[at + 1] - off[at]) == (L if keep else 0)
    q.close()


@pytest.mark.parametrize("L,n", [(400, 187), (3000, 21), (14000, 5), (14000, 1), (120, 1), (120, 2)])
def test_grep_fewer_records_to_a_tile(g, L, n):
    q = Grep(g, *lc.A_RULES)
    q.run(lc.uniform(L, n), what="%d records of %d" % (n, L))
    q.run([lc.event(i, L, keep=False) for i in range(n)], what="%d dropped records of %d" % (n, L))
    q.close()


def test_grep_alignment_and_the_end_of_the_data(g):
    q = Grep(g, *lc.A_RULES)
    for a in range(16):
        for e in range(16):
            q.run(lc.aligned(a, e), what="align %d end %d" % (a, e))
    q.close()


@pytest.mark.parametrize("over_16k", [False, True])
def test_grep_chunk_that_asks_for_its_longest_tile(g, over_16k):
    """A.5: 66 000 records: lane_geometry launches k_tile_max; a run of 64 records four times as long sizes the waves' LDS"""
    recs = lc.tile_max_chunk(over_16k)
    assert grep_once(g, recs, *lc.A_RULES)[0] == g.MODIFIED


def test_grep_more_units_than_a_look_back_window(g):
    """A.6: 70 000 records are 274 units whose byte counts differ; the output offsets are the running sum of the kept lengths"""
    recs, flags = lc.run_pattern_chunk()
    ret, got, off = grep_once(g, recs, *lc.A_RULES)
    assert ret == g.MODIFIED
    keep_len = np.fromiter((len(r) if k else 0 for r, k in zip(recs, flags)), dtype=np.uint64, count=len(recs))
    want_off = np.zeros(len(recs) + 1, dtype=np.uint64)
    np.cumsum(keep_len, out=want_off[1:])
    assert (off == want_off).all(), int(np.argmax(off != want_off))


def _name_chunk(n):
    recs = [lc.rec(b, i) for i, (_, b, _) in enumerate(lc.name_records(n))]
    assert all_fit(recs)
    return recs


@pytest.mark.parametrize("n", lc.NAME_LENS)
def test_grep_names(g, n):
    """C.1: the walk's masked dword compare of a rule's name against the record's keys"""
    recs = _name_chunk(n)
    for kind in ("regex", "exclude"):
        ret, got, off = grep_once(g, recs, [(kind, lc.name(n).decode() + " ^hit$")], what="name of %d" % n)
        assert ret == g.MODIFIED
    # two records only, the name the very last key of the chunk: the dwords read for it run past the data
    grep_once(g, [lc.rec({b"other": b"hit"}), lc.rec({lc.name(n): b""})], [("exclude", lc.name(n).decode() + " ^$")], what="last key of the data, %d" % n)


def test_grep_eight_and_nine_names(g):
    lens = [1, 3, 4, 5, 7, 8, 9, 12, 16]
    recs = [r for n in lens for r in _name_chunk(n)]
    assert all_fit(recs)
    for k, lane in ((8, True), (9, False)):
        for kind in ("regex", "exclude"):
            rules = [(kind, lc.name(n).decode() + " ^hit$") for n in lens[:k]]
            grep_once(g, recs, rules, "OR", lane=lane, what="%d names" % k)
            grep_once(g, recs, rules, "AND", lane=lane, what="%d names" % k)


@pytest.mark.parametrize("pattern", lc.VALUE_PATTERNS)
def test_grep_values(g, pattern):
    """C.2: the automaton's 4-byte step on values of every length and encoding, the cells "match whatever follows" and "hand the value on"
    at every place of the step, values that are no strings"""
    recs = [lc.rec({b"log": v}, i) for i, (_, v, _) in enumerate(lc.value_records())]
    assert all_fit(recs)
    for kind in ("regex", "exclude"):
        grep_once(g, recs, [(kind, "log " + pattern)], what=pattern)
        # (six automata side by side: the same value under six rules, the asked pattern last)
        grep_once(g, recs, [(kind, "log ^never%d$" % i) for i in range(5)] + [(kind, "log " + pattern)], "OR", what=pattern)
    # the value as the last bytes of the data: what the 4-byte step reads behind it is the padding, not the next record's header
    q = Grep(g, [("regex", "log " + pattern)])
    for L in (0, 1, 2, 3, 5, 6, 7, 9):
        for last in (b"a" * L, b"a" * L + b"b", b"xx"[:L % 3] + b"Q"):
            q.run([lc.rec({b"log": b"aab"}), lc.rec({b"log": b"Q"}), lc.rec({b"log": last})], what=(pattern, last))
    q.close()


@pytest.mark.parametrize("rule", lc.SUBKEY_RULES)
def test_grep_sub_keys(g, rule):
    recs = [lc.rec(b, i) for i, (_, b, _) in enumerate(lc.subkey_records())]
    assert all_fit(recs)
    for kind in ("regex", "exclude"):
        grep_once(g, recs, [(kind, rule)], what=rule)
        grep_once(g, recs, [(kind, rule), (kind, "nothing x")], "OR", what=rule)


def _count_filters(n):
    out = [(lc.count_rules(n, kind), op) for kind in ("regex", "exclude") for op in (None, "AND", "OR")]
    mixed = [("regex" if i % 2 == 0 else "exclude", r) for i, (_, r) in enumerate(lc.count_rules(n, "regex"))]
    return out + [(mixed, None), ([("exclude" if k == "regex" else "regex", r) for k, r in mixed], None)]


@pytest.mark.parametrize("n", lc.RULE_COUNTS)
def test_grep_rule_counts(g, n):
    """C.3: the automata run six side by side and the verdict is a 64-bit mask"""
    recs = [lc.rec(b, i) for i, (_, b) in enumerate(lc.count_records(n))]
    assert all_fit(recs)
    for rules, op in _count_filters(n):
        grep_once(g, recs, rules, op, what="%d rules" % n)


def test_grep_record_shapes(g):
    """C.4: the shapes the lean walk declines are decided by decode_event / grep_decide in the same kernel"""
    shapes = lc.shape_records()
    recs = [lc.event(i) for i in range(192)]
    for k, (what, row, plain, notouch) in enumerate(s for s in shapes if not s[3]):
        recs[3 + 11 * k] = row
    recs[64] = recs[127] = recs[128] = b""                               # rows an earlier filter emptied, at a tile's first and last place
    assert all_fit(recs)
    q = Grep(g, *lc.A_RULES)
    assert q.run(recs, what="shapes")[0] == g.MODIFIED
    for what, row, plain, notouch in shapes:
        if notouch:
            bad = [lc.event(i) for i in range(130)]
            for at in (0, 63, 129):
                one = list(bad)
                one[at] = row
                assert q.run(one, what=what)[0] == g.NOTOUCH
    q.close()
    grep_once(g, [lc.event(i) for i in range(130)], [("regex", "msg ok$")], what="nothing dropped")     # NOTOUCH by the record counts


def test_grep_copy_out(g):
    """C.5: the byte path, one lane, the overlapping last 32-byte step and the second round of a record's eight lanes"""
    recs = lc.copy_chunk()
    ret, got, off = grep_once(g, recs, *lc.COPY_RULES, what="copy-out")
    assert ret == g.MODIFIED
    lens = [int(off[i + 1] - off[i]) for i in range(len(recs))]
    assert lens[:6] == [14, 0, 14, 31, 0, 31] and lens[64:128] == [0] * 64 and lens[128:192] == [0] * 63 + [65] and lens[192:206] == lc.REC_LENS


def run_pair(g, recs, r1, op1, r2, op2, what=""):
    chunk, bufs, blob = _upload(g, recs)
    f1, f2 = g.FilterGrep(r1, op1), g.FilterGrep(r2, op2)
    try:
        ch = g.FilterChain([f1, f2])
        f1.profile(True)
        ret, out = ch.filter_dev(chunk)
        assert "k_grep_lane(two instances)" in f1.profile_read(), (what, f1.profile_read())
        wret, wout = oracle_chain([ob.Grep(r1, op1), ob.Grep(r2, op2)], blob)
        assert ret == wret, (what, r1[:2], r2[:2])
        if ret == g.MODIFIED:
            got, _ = _download(g, out)
            assert got == wout, (what, r1[:2], r2[:2], first_diff(wout, got))
    finally:
        f1.close(); f2.close()
        g.lib().flbgpu_dev_free(bufs[0]); g.lib().flbgpu_dev_free(bufs[1])


def test_grep_pairs(g):
    """C.6: the families C.1 to C.3 through two instances that run as one pass, the names split between them"""
    for n in lc.NAME_LENS:
        recs = _name_chunk(n)
        run_pair(g, recs, [("regex", lc.name(n).decode() + " ^hit$")], None, [("exclude", "other ^x$")], None, "names %d" % n)
        run_pair(g, recs, [("exclude", "other ^x$")], None, [("exclude", lc.name(n).decode() + " ^hit$")], None, "names %d" % n)
    recs = [lc.rec({b"log": v, b"n": b"%d" % i}, i) for i, (_, v, plain) in enumerate(lc.value_records())]
    for pattern in lc.VALUE_PATTERNS:
        run_pair(g, recs, [("exclude", "n ^[0-9]*7$")], None, [("regex", "log " + pattern)], None, pattern)
        run_pair(g, recs, [("exclude", "log " + pattern)], None, [("regex", "n [0-5]$")], None, pattern)
    recs = [lc.rec(b, i) for i, (_, b, _) in enumerate(lc.subkey_records())]
    for rule in lc.SUBKEY_RULES:
        run_pair(g, recs, [("regex", "k .")], None, [("exclude", rule)], None, rule)
    for n in lc.RULE_COUNTS[1:]:
        recs = [lc.rec(b, i) for i, (_, b) in enumerate(lc.count_records(n))]
        rules = lc.count_rules(n, "regex")
        h = n // 2
        run_pair(g, recs, rules[:h], "OR", [("exclude", r) for _, r in rules[h:]], "AND", "%d rules" % n)
        run_pair(g, recs, [("exclude", r) for _, r in rules[:h]], "AND", rules[h:], "OR", "%d rules" % n)


# ---------------------------------------------------------------------------------------------------------------- log_to_metrics
class Profiled:
    """the package with log_to_metrics filters whose profile is on and is read when check() closes them"""

    def __init__(self, g):
        self.g, self.seen = g, []

    def __getattr__(self, k):
        return getattr(self.g, k)

    def FilterLogToMetrics(self, *a, **kw):
        f = self.g.FilterLogToMetrics(*a, **kw)
        f.profile(True)
        close = f.close

        def close_and_note():
            self.seen.append(f.profile_read())
            close()
        f.close = close_and_note
        return f


def l2m_check(g, mode, props, chunks, value_field="duration", lane=True):
    pg = Profiled(g)
    s, st = check(pg, mode, props, chunks, value_field=None if mode == "counter" else value_field)
    assert len(pg.seen) == 1 and (not lane or "k_l2m_lane" in pg.seen[0]), pg.seen
    return s, st


MODES = ["counter", "gauge", "histogram"]


@pytest.mark.parametrize("mode", MODES)
def test_l2m_staging(g, mode):
    """D / A.1 to A.4 for k_l2m_lane: the same staging code a third time, checked on whole snapshots"""
    l2m_check(g, mode, lc.L2M_LABELS, [b"".join(recs) for _, recs in lc.fit_sweep(lc.l2m_geometry)])
    for L in (16001, 40000):
        chunks = [b"".join(lc.too_long(L, behind, True)[0]) for behind in (0, 1, 5, 60, 63)]
        s, st = l2m_check(g, mode, lc.L2M_LABELS, chunks)
        longs = [x for x in s if x["labels"][0] == b"long"]               # the long records' label and value are observed
        assert len(longs) == 2 and (mode != "counter" or sum(x["value"] for x in longs) == 5.0) and (mode != "gauge" or longs[0]["value"] == 77.0)
    for L, n in ((400, 187), (3000, 21), (14000, 5), (14000, 1), (120, 1), (120, 2)):
        l2m_check(g, mode, lc.L2M_LABELS, [b"".join(lc.uniform(L, n))])
    l2m_check(g, mode, lc.L2M_LABELS, [b"".join(lc.aligned(a, e)) for a in range(16) for e in range(16)])


@pytest.mark.parametrize("mode", ["gauge", "histogram"])
def test_l2m_value_field(g, mode):
    s, st = l2m_check(g, mode, lc.L2M_LABELS, [b"".join(lc.l2m_value_chunk())])
    print(st)
    kinds = [k for _, _, k in lc.l2m_value_records()]
    assert st["deferred"] == 2 * kinds.count("deferred")                 # the 40-digit decimal went through k_l2m_generic
    assert {x["labels"][0] for x in s} == {w.encode() for w, _, k in lc.l2m_value_records() if k != "other"}


@pytest.mark.parametrize("mode", MODES)
def test_l2m_labels(g, mode):
    l2m_check(g, mode, lc.L2M_LABELS, [b"".join(lc.l2m_label_chunk())])


@pytest.mark.parametrize("n", lc.NAME_LENS)
def test_l2m_names(g, n):
    """C.1's names as a label key and as the value key"""
    k, vk, recs = lc.l2m_name_chunk(n)
    for mode in MODES:
        l2m_check(g, mode, [("label_field", k.decode()), ("label_field", "color")], [b"".join(recs)], value_field=vk.decode())

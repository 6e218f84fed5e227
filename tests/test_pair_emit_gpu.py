"""The fused [filter_parser, filter_grep] pair (csrc/fused_kernels.inc k_pg_decide / k_pg_emit, flbgpu.cpp run_pair_fused) on the named
chunks of tests/pair_chunks.py: the staging area of k_pg_emit at both its sizes and every alignment, one record around the staging
size, a whole group of 64 in one batch, the queue's wave and workgroup seams, 16-byte tail copies next to a neighbour's record, the
time text at the chunk's end, parsers of 1 .. 31 fields, values around the register window and around 0xFFFF bytes, and rules that
k_pg_decide walks from registers, from LDS tables and from global ones.  Every expected byte, return code, row offset and count is
the CPU oracle's (filter_parser then filter_grep); tests/test_pair_chunks.py asserts on the CPU that each chunk sits on its edge.
Each case runs through the host-level and the device-level call, launched ahead of its sizes and the usual way, and asserts from the
profile that the fused kernels it is meant for really ran."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import oracle_binding as ob
import pair_chunks as pc
import test_pair_chunks as tpc
from test_tile_gpu import MODES

pytestmark = pytest.mark.gpu
BUILD_ENVS = ("FLBGPU_EMIT_GENERAL", "FLBGPU_NO_DESC", "FLBGPU_DEFER_TIME", "FLBGPU_TILE_MODE", "FLBGPU_NO_TILE", "FLBGPU_FX", "FLBGPU_NO_FUSE")


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


@pytest.fixture(params=["ahead", "usual"], autouse=True)
def launch(request, monkeypatch):
    """a chunk of up to 8 MB is launched ahead of its sizes (flbgpu.cpp SpecCall); FLBGPU_NO_SPEC=1: sized first, the larger chunks' way.
    The library reads the variables at every call."""
    for k in BUILD_ENVS + ("FLBGPU_NO_SPEC",):
        monkeypatch.delenv(k, raising=False)
    if request.param == "usual":
        monkeypatch.setenv("FLBGPU_NO_SPEC", "1")
    return request.param


class Pair:
    """one parser, its filter_parser, a filter_grep and the chain over the two; made once per configuration and reused across a sweep"""

    def __init__(self, g, pargs, rules, op=None):
        self.g = g
        self.p = g.Parser(**pargs)
        self.fp, self.fg = g.FilterParser("log", [self.p]), g.FilterGrep(list(rules), op)
        self.ch = g.FilterChain([self.fp, self.fg])

    def close(self):
        self.fg.close(); self.fp.close(); self.p.close()


class Pairs(dict):
    def get(self, g, c):
        key = (tuple(sorted(c.pargs.items())), tuple(c.rules), c.op)
        if key not in self:
            self[key] = Pair(g, c.pargs, c.rules, c.op)
        return self[key]

    def close(self):
        for p in self.values():
            p.close()
        self.clear()


def want_stats(c, res):
    r1, o1, r2, o2, keep_len = res
    n, kept = len(c.recs), sum(1 for x in keep_len if x)
    return [dict(ret=ob.MODIFIED, in_records=n, out_records=n, out_bytes=len(o1)), dict(ret=ob.MODIFIED, in_records=n, out_records=kept, out_bytes=len(o2))]


def first_diff(a, b):
    n = min(len(a), len(b))
    i = next((k for k in range(n) if a[k] != b[k]), n)
    return "first difference at byte %d of %d / %d: %r / %r" % (i, len(a), len(b), a[max(i - 8, 0):i + 16], b[max(i - 8, 0):i + 16])


def _ok(g, ret, what):
    """a call that comes back without MODIFIED; a device fault ends the session (nothing more is started on a faulted device)"""
    err = g.last_error()
    if ret != g.MODIFIED and ("illegal memory access" in err or "hardware exception" in err or "unspecified launch failure" in err):
        pytest.exit("device fault in %r: %s" % (what, err), returncode=3)
    assert ret == g.MODIFIED, (what, ret, err)


def run_both(g, pair, c, res, kernels=("k_pg_emit",), absent=("k_parser_emit",), what=""):
    """the chunk through FilterChain.filter (host bytes) and FilterChain.filter_dev (an uploaded chunk): bytes, return code, counts and
    -- on the device-level call -- row offsets against the oracle; the named kernels in (and out of) the profile of each call
    (k_parser_emit is the unfused chain's writer: a call launched ahead of its sizes launches k_pg_emit before it knows that the chunk is
    not the pair's, so only its absence says that the fused kernels wrote the output)"""
    r1, o1, r2, o2, keep_len = res
    stats = want_stats(c, res)
    what = (c.name, what)
    # host level
    pair.fp.profile(True)
    ret, out = pair.ch.filter(c.blob + c.tail)
    prof = pair.fp.profile_read()
    _ok(g, ret, what)
    assert out == o2, (what, "host", first_diff(out, o2))
    assert pair.ch.last_stats() == stats, (what, "host", pair.ch.last_stats(), stats)
    assert all(k in prof for k in kernels) and not any(k in prof for k in absent), (what, "host", sorted(prof))
    # device level: the rows' offsets given, 16 spare bytes behind the chunk (and the undecodable tail, when there is one, in them or behind)
    L = g.lib()
    blob = c.blob
    off = np.zeros(len(c.recs) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(r) for r in c.recs), dtype=np.uint64, count=len(c.recs)), out=off[1:])
    d_data, d_off = L.flbgpu_dev_alloc(len(blob) + len(c.tail) + 16), L.flbgpu_dev_alloc(off.nbytes)
    assert d_data and d_off, g.last_error()
    try:
        L.flbgpu_memcpy_h2d(d_data, blob + c.tail, len(blob) + len(c.tail)); L.flbgpu_memcpy_h2d(d_off, off.ctypes.data, off.nbytes)
        pair.fp.profile(True)
        ret, o = pair.ch.filter_dev(g.DevChunk(d_data, d_off, len(c.recs), len(blob)))
        prof = pair.fp.profile_read()
        _ok(g, ret, what)
        assert int(o.bytes) == len(o2) and int(o.n) == len(c.recs), (what, "device", ret, int(o.bytes), len(o2), int(o.n), g.last_error())
        got = ctypes.create_string_buffer(len(o2))
        L.flbgpu_memcpy_d2h(got, o.data, len(o2))
        assert got.raw == o2, (what, "device", first_diff(got.raw, o2))
        goff = np.zeros(len(c.recs) + 1, dtype=np.uint64)
        L.flbgpu_memcpy_d2h(goff.ctypes.data, o.row_off, goff.nbytes)
        want_off = np.zeros(len(c.recs) + 1, dtype=np.uint64)
        np.cumsum(np.asarray(keep_len, dtype=np.uint64), out=want_off[1:])
        assert np.array_equal(goff, want_off), (what, "device row offsets", int(np.argmax(goff != want_off)))
        assert pair.ch.last_stats() == stats, (what, "device", pair.ch.last_stats(), stats)
        assert all(k in prof for k in kernels) and not any(k in prof for k in absent), (what, "device", sorted(prof))
    finally:
        L.flbgpu_dev_free(d_data); L.flbgpu_dev_free(d_off)


# ------------------------------------------------------------------------------------------ (a) the staging sweep
@pytest.mark.parametrize("build", ["plain", "general", "no descriptors"])
def test_staging_sweep(g, monkeypatch, build):
    """batches that end at STG - 1, at STG, and whose next record would end at STG + 1, starting at every alignment, for both staging
    sizes (the plain build's 8192, the general build's 9728 -- every chunk runs under every build: an edge of the one is an ordinary
    chunk to the other)"""
    if build == "general":
        monkeypatch.setenv("FLBGPU_EMIT_GENERAL", "1")
    if build == "no descriptors":
        monkeypatch.setenv("FLBGPU_NO_DESC", "1")                       # rec_load + spans_to_lds instead of the descriptor
    pairs = Pairs()
    for c, res in tpc._results("staging"):
        pair = pairs.get(g, c)
        # every kept record with an agent has its descriptor: the plain build writes them all (an empty agent is the generic kernel's row)
        run_both(g, pair, c, res, absent=("k_parser_emit", "k_pg_emit_general") if c.notes["first_agent"] else ("k_parser_emit",), what=build)
        assert pair.fp.paths()["plain_emit"] == (build == "plain"), (c.name, build, pair.fp.paths())
    pairs.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_staging_under_the_three_builds_of_pass_one(g, monkeypatch, mode):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    pick = {"reg": 3, "tile": 8, "phase": 13}[mode]                     # one alignment each
    cases = [(c, r) for c, r in tpc._results("staging") if c.notes["first_agent"] == pick]
    assert len(cases) == 6
    pairs = Pairs()                                                     # (the parser is made under the mode's variables)
    for c, res in cases:
        run_both(g, pairs.get(g, c), c, res, what=mode)
    pairs.close()


# ------------------------------------------------------------------------------------------ (b) one record around the staging size
@pytest.mark.parametrize("build", ["plain", "general"])
def test_one_record_around_the_staging_size(g, monkeypatch, build):
    """a kept record without a descriptor whose size is the staging size less the alignment, one byte less, one byte more (`direct`):
    the plain build hands it on to the general one; with fewer than 64 kept records it stays the chosen build"""
    if build == "general":
        monkeypatch.setenv("FLBGPU_EMIT_GENERAL", "1")
    pairs = Pairs()
    for c, res in tpc._results("one_big"):
        pair = pairs.get(g, c)
        run_both(g, pair, c, res, kernels=("k_pg_emit", "k_pg_emit_general") if build == "plain" else ("k_pg_emit",), what=build)
        assert pair.fp.paths()["plain_emit"] == (build == "plain") and not pair.fp.paths()["aside"]["plain_emit"], (c.name, pair.fp.paths())
    pairs.close()


# ------------------------------------------------------------------------------------------ (c) a full batch of 64
def test_full_batch_of_64(g):
    pairs = Pairs()
    for c, res in tpc._results("full_batch"):
        run_both(g, pairs.get(g, c), c, res)
    pairs.close()


# ------------------------------------------------------------------------------------------ (d) the queue's seams
def test_queue_seams(g, launch):
    pairs = Pairs()
    for c, res in tpc._results("queue"):
        run_both(g, pairs.get(g, c), c, res)
    # the named exception: one record, kept -- grep answers NOTOUCH, the pair hands the chunk to the unfused kernels; the parser's bytes leave
    c = pc.unfused_queue_chunk()
    r1, o1, r2, o2, keep_len = tpc.oracle_pair(c)
    pair = pairs.get(g, c)
    pair.fp.profile(True)
    ret, out = pair.ch.filter(c.blob)
    prof = pair.fp.profile_read()
    assert (ret, out) == (g.MODIFIED, o1) and "k_parser_emit" in prof and (launch == "ahead" or "k_pg_emit" not in prof), (ret, sorted(prof))
    st = pair.ch.last_stats()
    assert [(s["ret"], s["in_records"], s["out_records"], s["out_bytes"]) for s in st] == [(ob.MODIFIED, 1, 1, len(o1)), (ob.NOTOUCH, 1, 1, len(o1))], st
    pairs.close()


# ------------------------------------------------------------------------------------------ (e) last-field tails
@pytest.mark.parametrize("build", ["plain", "general", "no descriptors"])
def test_last_field_tails(g, monkeypatch, build):
    """an agent of 0 .. 48 bytes as the last field of the last record of a batch, of the last kept record and of the last record of the
    chunk, with and without bytes behind the chunk: the 16-byte tail copy must neither write into the neighbour's record nor depend on
    what follows the chunk"""
    if build == "general":
        monkeypatch.setenv("FLBGPU_EMIT_GENERAL", "1")
    if build == "no descriptors":
        monkeypatch.setenv("FLBGPU_NO_DESC", "1")
    pairs = Pairs()
    for c, res in tpc._results("tails"):
        run_both(g, pairs.get(g, c), c, res, what=build)
    pairs.close()


# ------------------------------------------------------------------------------------------ (f) the time text at the chunk's end
@pytest.mark.parametrize("defer", ["emit pass", "single pass"])
def test_time_text_at_the_chunks_end(g, monkeypatch, defer):
    """pge_time reads 32 bytes from the time text's start, or the 27 .. 31 the chunk still has"""
    if defer == "single pass":
        monkeypatch.setenv("FLBGPU_DEFER_TIME", "0")
    pairs = Pairs()
    for c, res in tpc._results("time_end"):
        if c.notes["odd"]:
            continue
        pair = pairs.get(g, c)
        run_both(g, pair, c, res, what=defer)
        assert pair.fp.paths()["emit_time"] == (defer == "emit pass"), (c.name, pair.fp.paths())
    pairs.close()
    reported = set()
    for c, res in tpc._results("time_end"):
        if not c.notes["odd"]:
            continue
        pair = Pair(g, c.pargs, c.rules, c.op)                          # a fresh filter: a reported text moves the lookup for the next calls
        run_both(g, pair, c, res, what=defer)
        if pair.fp.paths()["aside"]["emit_time"]:                       # reported by the emit pass (counts[13]), the call repeated
            reported.add("middle" if c.notes.get("middle") else c.notes["left"])
        pair.close()
    # the report-and-repeat route is taken in the middle of a chunk and for its last record, with fewer than 32 bytes left and with more
    # (not every last record's lookup is left to the emit pass: the single pass keeps the lookup of the rows its fix-up launch takes)
    assert reported >= ({"middle", 31, 33} if defer == "emit pass" else set()) and (defer == "emit pass" or not reported), reported


# ------------------------------------------------------------------------------------------ (g) field counts
def test_field_counts(g):
    pairs = Pairs()
    for c, res in tpc._results("fields"):
        if c.notes.get("unfused"):
            run_both(g, pairs.get(g, c), c, res, kernels=("k_parser_emit",), absent=())       # the NFA engine's parser: the unfused kernels
        else:
            run_both(g, pairs.get(g, c), c, res)
    pairs.close()


def test_a_parser_of_more_than_31_fields_is_refused(g):
    """the regex compiler takes 31 capture groups: a parser of 32 or 33 named groups is refused when it is made, with a message, so
    `nfields > 32` of pair_fusable is never met; 31 is the widest parser there is"""
    for nf in pc.REFUSED_FIELD_COUNTS:
        with pytest.raises(ValueError, match="more than 31 capture groups"):
            g.Parser(regex=pc.fields_regex(nf))
    g.Parser(regex=pc.fields_regex(31)).close()


# ------------------------------------------------------------------------------------------ (h) value lengths
def test_value_length_seams(g):
    (c1, r1), (c2, r2) = tpc._results("values")
    pairs = Pairs()
    # 268 .. 276 bytes: beyond 272 the single pass takes the value's rest from memory windows; the rows keep their descriptors
    run_both(g, pairs.get(g, c1), c1, r1, absent=("k_parser_emit", "k_pg_emit_general"))
    # 65534 .. 65536 bytes: u16 spans in LDS below 0xFFFF, the span columns from there on; every one of them `direct`
    run_both(g, pairs.get(g, c2), c2, r2, kernels=("k_pg_emit", "k_pg_emit_general"))
    pairs.close()


def test_value_length_seams_general_build(g, monkeypatch):
    monkeypatch.setenv("FLBGPU_EMIT_GENERAL", "1")
    pairs = Pairs()
    for c, res in tpc._results("values"):
        run_both(g, pairs.get(g, c), c, res, absent=("k_parser_emit", "k_pg_emit_general"))
    pairs.close()


# ------------------------------------------------------------------------------------------ (i) rules
def _table_bytes(g, rule):
    """bytes of a rule's match-only tables as upload_dfa lays them out (256 classes, 2 bytes per transition, 1 per state)"""
    L = g.lib()
    L.flbgpu_rx_compile.restype = ctypes.c_void_p
    L.flbgpu_rx_compile.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    L.flbgpu_rx_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    L.flbgpu_rx_free.argtypes = [ctypes.c_void_p]
    pat = rule.split(" ", 1)[1].encode()
    h = L.flbgpu_rx_compile(pat, len(pat), 0, 0, None, 0)
    assert h
    info = (ctypes.c_int * 12)()
    L.flbgpu_rx_info(h, info)
    L.flbgpu_rx_free(h)
    return 256 + 2 * info[0] * info[1] + info[1]


def test_rules_in_k_pg_decide(g):
    """`Z$` on a field of 0 .. 32 bytes (the register DFA up to 16 bytes, dfa_match beyond), last byte Z or not; the rows reach
    k_pg_decide through a rule on the kept time field or through a byte >= 0x80 in a field no rule tests; OR, AND and the legacy list"""
    sizes = [_table_bytes(g, v) for _, v in pc.BIG_TABLE_RULES]
    pad = lambda x: (x + 15) & ~15
    # the first rule's tables are staged, the second's no longer fit (walked in global memory), the third's fit behind the first's
    assert sizes[0] <= pc.RULE_LDS_ROOM < pad(sizes[0]) + sizes[1] and pad(sizes[0]) + sizes[2] <= pc.RULE_LDS_ROOM, sizes
    pairs = Pairs()
    for c, res in tpc._results("rules"):
        run_both(g, pairs.get(g, c), c, res, kernels=("k_pg_decide", "k_pg_emit"))
    pairs.close()

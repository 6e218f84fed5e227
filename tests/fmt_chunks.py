"""Named chunks for the msgpack -> JSON formatter (csrc/kernels_fmt.hip k_fmt_size / k_fmt_groups / k_fmt_emit, fmt_dev.inc, packfmt.cpp):
every chunk sits on one edge of the kernels -- the staging area of k_fmt_emit (exact fit, one byte over, the direct path, all 16
alignments, split batches, rows that print nothing, the flush's 16-byte seams, string tails at the chunk's end), the second trip of both
grid-stride loops, the 1024-row tiles of k_fmt_groups with its three carried values and the 1000-skipped-rows guard, the order in which
a bad row, a NULL row and the skip limit end the walk, and value sweeps (floats, dates, strings) at a row per value.

fmt_plan() restates the batch loop of k_fmt_emit in plain Python; FMT_STG and the tile size are read out of kernels_fmt.hip, so a change
there moves the chunks with it (or fails tests/test_fmt_chunks.py, which proves on the CPU, from the oracle alone, that each chunk is on
its edge).  expect() is the CPU oracle's answer for a chunk: text (or NULL), rows walked, row offsets, and whether the group pass runs."""
import os
import random
import re
import struct

import numpy as np

import oracle_binding as ob
from synth import mp, KV, Raw

HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = open(os.path.join(os.path.dirname(HERE), "fluent-bit_amd", "csrc", "kernels_fmt.hip")).read()
FMT_STG = int(re.search(r"constexpr int FMT_STG = (\d+)", _SRC).group(1))
TILE = int(re.search(r"__launch_bounds__\((\d+)\)\s+k_fmt_groups", _SRC).group(1))
T = TILE
SKIP_LIMIT = 1000                      # the decoder's recursion guard (src/flb_log_event_decoder.c:27)

JSON, STREAM, LINES = 1, 2, 3
N, OPEN, CLOSE, SKIP, BAD = 0, 1, 2, 3, 4      # row kinds: printing, group opener, group closer, negative time, refused by the decoder


def CFG(fmt=LINES, df=2, dk=b"date", esc=1, nan=0):
    return dict(json_format=fmt, date_format=df, date_key=dk, escape_unicode=esc, nan_to_null=nan)


def oracle(data, cfg, fmt=None):
    return ob.msgpack_to_json_format(data, cfg["json_format"] if fmt is None else fmt, cfg["date_format"], cfg["date_key"],
                                     cfg["escape_unicode"], cfg["nan_to_null"])


def fmt_plan(row_lens, fmt_stg):
    """the batch loop of k_fmt_emit: for each wave of 64 rows the batches (lo, m, align, direct); a direct row has m = 0"""
    n = len(row_lens)
    off = [0] * (n + 1)
    for i, x in enumerate(row_lens):
        off[i + 1] = off[i] + int(x)
    waves = []
    for base in range(0, n, 64):
        cnt = min(64, n - base)
        lo, batches = 0, []
        while lo < cnt:
            batch_base = off[base + lo]
            align = batch_base & 15
            m = 0
            while lo + m < cnt and off[base + lo + m + 1] - batch_base + align <= fmt_stg:
                m += 1
            if m == 0:
                batches.append((lo, 0, align, True))
                lo += 1
            else:
                batches.append((lo, m, align, False))
                lo += m
        waves.append(batches)
    return waves


# ------------------------------------------------------------------------------------------ rows
def ev(sec, nsec, body, meta=b"\x80"):
    return b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + meta + body


def opener(attrs=None, meta=b"\x80"):
    return ev(0xffffffff, 0, mp(KV([(b"resource", b"r1")])) if attrs is None else attrs, meta)


CLOSER = ev(0xfffffffe, 0, b"\x80")
NEG = b"\x92\x92\xcb" + struct.pack(">d", -5.0) + b"\x80" + mp(KV([(b"x", 1)]))
BADROW = b"\xc1"
SEC = 1700000000


def row(i, extra=b""):
    return ev(SEC + i, 5, mp(KV([(b"i", i), (b"s", extra)])) if extra else mp(KV([(b"i", i)])))


class Chunk:
    """recs: the rows (bytes each) or None for a chunk kept as blob + rlen; kinds: one of N / OPEN / CLOSE / SKIP / BAD per row"""

    def __init__(self, name, cfg, recs=None, kinds=None, blob=None, rlen=None, notes=None):
        self.name, self.cfg, self.notes = name, cfg, notes or {}
        if recs is not None:
            blob = b"".join(recs)
            rlen = np.fromiter((len(r) for r in recs), dtype=np.uint64, count=len(recs))
        self.recs, self.blob, self.rlen = recs, blob, rlen
        self.n = len(rlen)
        self.kinds = np.zeros(self.n, dtype=np.uint8) if kinds is None else np.asarray(kinds, dtype=np.uint8)
        assert len(self.kinds) == self.n and int(rlen.sum()) == len(blob)
        self._exp = None

    def in_off(self):
        off = np.zeros(self.n + 1, dtype=np.uint64)
        np.cumsum(self.rlen, out=off[1:])
        return off

    def walk_end(self):
        """rows the decoder walks: up to the first row it refuses, or the row that directly follows 1000 skipped ones"""
        nz = np.flatnonzero(self.kinds)
        if len(nz) == 0:
            return self.n
        run = 0
        for r in range(int(nz[0]), self.n):
            k = self.kinds[r]
            if k == BAD or run >= SKIP_LIMIT:
                return r
            run = run + 1 if k in (OPEN, CLOSE, SKIP) else 0
        return self.n

    def groups(self, indexed=False):
        """packfmt.cpp runs k_fmt_groups (and k_fmt_size again) for a chunk that holds a marker or 1000 skipped rows, counted over all the
        rows it is given; indexed: the rows were found by the record indexer, which stops at the first byte that is no msgpack object"""
        k = self.kinds
        bad = np.flatnonzero(k == BAD)
        if indexed and len(bad):
            k = k[:int(bad[0])]
        return bool(((k == OPEN) | (k == CLOSE)).any() or int(((k == OPEN) | (k == CLOSE) | (k == SKIP)).sum()) >= SKIP_LIMIT)

    def expect(self):
        """dict(out = the oracle's text or None, n = rows walked, lens = text bytes per row, row_off, groups)"""
        if self._exp is not None:
            return self._exp
        cfg = self.cfg
        out = oracle(self.blob, cfg)
        e = dict(out=out, groups=self.groups(), groups_indexed=self.groups(True), n=None, lens=None, row_off=None)
        if out is not None:
            lines = out if cfg["json_format"] == LINES else oracle(self.blob, cfg, LINES)
            n = self.walk_end()
            lens = np.zeros(n, dtype=np.uint64)
            if lines:
                nl = np.flatnonzero(np.frombuffer(lines, dtype=np.uint8) == 10)
                ll = np.diff(np.concatenate(([-1], nl))).astype(np.uint64)
                prints = np.flatnonzero(self.kinds[:n] == N)
                assert len(prints) == len(ll), (self.name, "the oracle prints %d rows, the builder expects %d" % (len(ll), len(prints)))
                lens[prints] = ll - (1 if cfg["json_format"] == STREAM else 0)
            else:
                assert not (self.kinds[:n] == N).any(), self.name
            off = np.zeros(n + 1, dtype=np.uint64)
            np.cumsum(lens, out=off[1:])
            assert int(off[-1]) + (cfg["json_format"] == JSON) == len(out) or (cfg["json_format"] == JSON and out == b"[]"), self.name
            e.update(n=n, lens=lens, row_off=off)
        self._exp = e
        return e


_base = {}


def frame(cfg):
    return 0 if cfg["json_format"] == STREAM else 1


def sized_row(L, cfg, sec=SEC, ch=b"a"):
    """a row whose text (frame included) is exactly L bytes in cfg's format: {"date":..,"s":"aaa.."}"""
    key = (cfg["date_format"], cfg["date_key"], sec)
    if key not in _base:
        _base[key] = len(oracle(ev(sec, 5, mp(KV([(b"s", b"")]))), cfg, LINES)) - 1
    k = L - frame(cfg) - _base[key]
    assert k >= 0, (L, _base[key])
    return ev(sec, 5, mp(KV([(b"s", ch * k)])))


ALL_FMT = (LINES, JSON, STREAM)


# ------------------------------------------------------------------------------------------ (a) staging and batches
def stg_edge(fmt):
    """for every align 0..15 and d in -1, 0, +1 a row of L + align = FMT_STG + d first in its batch, behind a small pad row"""
    cfg = CFG(fmt)
    recs, cur, want = [], 0, []
    for align in range(16):
        for d in (-1, 0, 1):
            pad = 40 + (align - cur - 40) % 16
            recs.append(sized_row(pad, cfg))
            cur += pad
            L = FMT_STG + d - align
            recs.append(sized_row(L, cfg))
            want.append((len(recs) - 1, align, d))
            cur += L
    return Chunk("stg_edge/%d" % fmt, cfg, recs, notes=dict(big=want))


ESC_PIECE = b'a"b\\c\nd\te\x01f\x7fg/h\r\x08\x0c plain text in between '
ILL_PIECE = (b"ok \xc3\xa9 \xe2\x82\xac \xf0\x9f\x98\x80 \x80 \xbf \xc0\x80 \xc3 x \xe2\x82 y \xe2\x28\xa1 \xed\xa0\x80 \xe0\x9f\xbf \xf0\x8f\xbf\xbf "
             b"\xf4\x90\x80\x80 \xf5\x80\x80\x80 \xf8\x88\x80\x80\x80 \xfe \xff \xf0\x9f\x98 z \xef\xbf\xbd \xee\x83\x8e sixteen clean bytes.. ")
DIRECT_LANES = (0, 1, 31, 62, 63)


def _tail_row(t, i):
    """an oversized row whose last string ends t bytes before the end of its line: `"` + closers + `}` + newline (t = 3 .. 8), or
    `","z":<digits>}` + newline (t = 9 .. 17)"""
    s = b"a" * (FMT_STG + 100 + t)
    if t <= 8:
        v = s
        for _ in range(t - 3):
            v = [v]
        return ev(SEC + i, 5, mp(KV([(b"s", v)])))
    return ev(SEC + i, 5, mp(KV([(b"s", s), (b"z", 10 ** (t - 9))])))


def direct_rows(fmt, esc):
    """rows over FMT_STG at lanes 0, 1, 31, 62, 63 of a wave: escapes, ill-formed UTF-8, a duplicate key, ext + bin + floats, and last
    strings that end 3 .. 17 bytes before the end of the row's line (0 .. 2 do not exist: `"}` and the newline follow a string)"""
    cfg = CFG(fmt, esc=esc)
    k = FMT_STG // len(ESC_PIECE) + 2
    big = [ev(SEC, 5, mp(KV([(b"e", ESC_PIECE * k), (b"last", b"x" * 7)]))),
           ev(SEC + 1, 5, mp(KV([(b"u", ILL_PIECE * (FMT_STG // len(ILL_PIECE) + 2) + b"\xe2\x82")]))),
           ev(SEC + 2, 5, mp(KV([(b"k", b"dropped" * 50), (b"other", 1), (b"k", b"kept " * (FMT_STG // 5 + 9)), (b"n", KV([(b"q", 1), (b"q", 2)]))]))),
           ev(SEC + 3, 5, mp(KV([(b"x", Raw(b"\xc7\x05\x07\x00\x7f\x80\xff\x41")), (b"b", Raw(b"\xc5" + struct.pack(">H", FMT_STG + 3) + ILL_PIECE[:64] * (FMT_STG // 64) + b"end")),
                                  (b"f", [0.1, 1e22, 2.5, -0.0, float("nan"), 5e-324, Raw(b"\xca" + struct.pack(">f", 0.1))])]))),
           _tail_row(3, 4)]
    tails = [_tail_row(t, 10 + t) for t in range(4, 18)] + [ev(SEC + 30, 5, mp(KV([(b"e", ESC_PIECE * k + b'"')])))]
    recs = [row(i) for i in range(64)]
    lanes = []
    for w, group in enumerate([big, tails[0:5], tails[5:10], tails[10:15]]):
        wave = [row(1000 * w + i, b"ordinary " * (i % 5)) for i in range(64)]
        for lane, r in zip(DIRECT_LANES, group):
            wave[lane] = r
            lanes.append(len(recs) + lane)
        recs += wave
    recs += [row(i) for i in range(10)]
    return Chunk("direct_rows/%d/%d" % (fmt, esc), cfg, recs, notes=dict(direct=lanes))


def batch_split(fmt):
    cfg = CFG(fmt)
    q = FMT_STG // 64
    assert q * 64 == FMT_STG and FMT_STG % 16 == 0
    last_short = [sized_row(q, cfg)] * 63 + [sized_row(q - 1, cfg)]
    return [Chunk("batch_split/split/%d" % fmt, cfg, [sized_row(400 + (i % 3), cfg) for i in range(64)] + [row(1)]),
            Chunk("batch_split/full/%d" % fmt, cfg, [sized_row(q, cfg)] * 64 + [row(1)]),
            Chunk("batch_split/over/%d" % fmt, cfg, [sized_row(q, cfg)] * 63 + [sized_row(q + 1, cfg)] + [row(1)]),
            Chunk("batch_split/align/%d" % fmt, cfg, last_short + last_short + [row(1)])]


def zero_rows(fmt, marker):
    """rows that print nothing at a batch's first lane, at its last lane, as a whole wave, and 70 of them in front of the first printing
    row (which still gets the `[` of format json)"""
    cfg = CFG(fmt)
    z = CLOSER if marker else NEG
    zk = CLOSE if marker else SKIP
    recs, kinds = [z] * 70, [zk] * 70                               # wave 0 prints nothing; rows 64 .. 69 lead wave 1
    recs += [sized_row(400, cfg)] * 58; kinds += [N] * 58           # wave 1 ends here
    wave = [sized_row(400, cfg)] * 64                               # wave 2: zero rows at lane 0, in front of the row that no longer fits, at lane 63
    wk = [N] * 64
    fit = (FMT_STG - 15) // 400                                     # lanes 1 .. fit fit behind the zero row at lane 0, at any alignment
    for lane in (0, fit + 1, fit + 2, 63):
        wave[lane] = z; wk[lane] = zk
    recs += wave; kinds += wk
    recs += [z] * 64 + [row(7)]; kinds += [zk] * 64 + [N]           # wave 3: a batch whose total is 0, in mid-chunk
    return Chunk("zero_rows/%d/%d" % (fmt, marker), cfg, recs, kinds)


TAIL_N = (1, 63, 64, 65, 255, 256, 257)


def tail_waves(fmt):
    cfg = CFG(fmt)
    return [Chunk("tail_waves/%d/%d" % (n, fmt), cfg, [row(i, b"t" * (i * 7 % 23)) for i in range(n)]) for n in TAIL_N]


def flush_seams(fmt):
    """4 chunks of 5 x 64 rows of 2 .. 40 bytes (no date key; `{}` rows among them): the 16 seams between their waves fall on the 16
    byte alignments, so one wave's single-byte tail and the next one's single-byte head share a 16-byte piece"""
    cfg = CFG(fmt, dk=None)
    r = random.Random(160)
    f = frame(cfg)

    def small(L):                                                   # text of L bytes, frame included
        L -= f
        if L == 2: return ev(SEC, 5, b"\x80")
        if L == 6: return ev(SEC, 5, mp(KV([(b"", 1)])))
        if L == 7: return ev(SEC, 5, mp(KV([(b"", 10)])))
        assert L >= 8
        return ev(SEC, 5, mp(KV([(b"k", b"a" * (L - 8))])))
    sizes = [2 + f, 6 + f, 7 + f] + list(range(8 + f, 41))
    out = []
    for c in range(4):
        recs, cur = [], 0
        for w in range(5):
            for i in range(63):
                L = 2 + f if i % 9 == 0 else r.choice(sizes)
                recs.append(small(L)); cur += L
            L = 12 + f + ((4 * c + w + 1) % 16 - cur - 12 - f) % 16        # the wave ends at alignment 4c + w + 1 (mod 16)
            recs.append(small(L)); cur += L
        out.append(Chunk("flush_seams/%d/%d" % (c, fmt), cfg, recs))
    return out


def str_tails(fmt, esc):
    """the last value of a row a clean string of 1 .. 33 bytes: 33 rows in mid-chunk, then one as the very last bytes of the chunk"""
    cfg = CFG(fmt, esc=esc)
    mid = [ev(SEC + k, 5, mp(KV([(b"s", b"b" * k)]))) for k in range(1, 34)]
    return [Chunk("str_tails/%d/%d/%d" % (k, fmt, esc), cfg, mid + [ev(SEC, 5, mp(KV([(b"s", b"c" * k)])))]) for k in range(1, 34)]


# ------------------------------------------------------------------------------------------ (b) the grid
SLOW_EVERY = 4099


def tiny_rows(n):
    """n rows of 21 bytes ({"k": uint32}); every 4099th is longer and holds a duplicate key (its slow bit is set)"""
    a = np.zeros((n, 21), dtype=np.uint8)
    a[:, :4] = (0x92, 0x92, 0xd7, 0x00)
    i = np.arange(n, dtype=np.uint64)
    sec = (SEC + i).astype(">u4")
    a[:, 4:8] = sec.view(np.uint8).reshape(n, 4)
    a[:, 11] = 5
    a[:, 12:16] = (0x80, 0x81, 0xa1, ord("k"))
    a[:, 16] = 0xce
    a[:, 17:21] = i.astype(">u4").view(np.uint8).reshape(n, 4)
    rlen = np.full(n, 21, dtype=np.uint64)
    parts = []
    for j in range(0, n, SLOW_EVERY):
        s = ev(SEC + j, 5, mp(KV([(b"k", b"dropped"), (b"row", j), (b"k", b"the later one stays %d" % j)])))
        rlen[j] = len(s)
        parts.append(s)
        parts.append(a[j + 1:j + SLOW_EVERY].tobytes())
    return b"".join(parts), rlen


def emit_second_trip(cus):
    n = cus * 8 * 256 + 64 * 3 + 5
    blob, rlen = tiny_rows(n)
    return Chunk("emit_second_trip/%d" % cus, CFG(LINES), blob=blob, rlen=rlen)


def size_second_trip(cus):
    n = cus * 32 * 256 + 64 + 3
    blob, rlen = tiny_rows(n)
    return Chunk("size_second_trip/%d" % cus, CFG(LINES), blob=blob, rlen=rlen)


# ------------------------------------------------------------------------------------------ (c) groups and the skip guard
GROUP_FMT = (LINES, JSON)


def _body(i):
    if i % 11 == 3:
        return mp(KV([(b"i", i), (b"d", b"first"), (b"d", b"second")]))
    return mp(KV([(b"i", i)]))


def _meta(i):
    return mp(KV([(b"m", i)])) if i % 7 == 2 else b"\x80"


def group_edges(fmt):
    """openers at rows 0, T-1, T and 2T-1, closers at T-1 and T, a group over three tiles, an opener straight behind an opener, a closer
    without an opener, an opener with an empty body map; governed rows with metadata of their own and with duplicate keys"""
    cfg = CFG(fmt)
    out = []
    marks = {0: opener(mp(KV([(b"g", 0)]))), T - 1: CLOSER, T: opener(mp(KV([(b"g", b"T")])), mp(KV([(b"om", 1)]))),
             2 * T - 1: opener(mp(KV([(b"g", b"2T-1"), (b"deep", [1, KV([(b"a", b"b")])])])))}
    n = 4 * T + 5
    recs = [marks.get(i) or ev(SEC + i, 5, _body(i), _meta(i)) for i in range(n)]
    kinds = [N] * n
    for i, m in marks.items():
        kinds[i] = CLOSE if m is CLOSER else OPEN
    out.append(Chunk("group_edges/a/%d" % fmt, cfg, recs, kinds, notes=dict(openers=[0, T, 2 * T - 1], closers=[T - 1], governed=[1, T + 1, 2 * T, 3 * T, 4 * T + 4], free=[])))
    marks = {5: CLOSER, T - 1: opener(mp(KV([(b"g", b"T-1")]))), T: CLOSER, T + 10: opener(mp(KV([(b"g", b"early")]))),
             T + 11: opener(mp(KV([(b"g", b"late")]))), 2 * T - 1: opener(b"\x80")}
    n = 2 * T + 40
    recs = [marks.get(i) or ev(SEC + i, 5, _body(i), _meta(i)) for i in range(n)]
    kinds = [N] * n
    for i, m in marks.items():
        kinds[i] = CLOSE if m is CLOSER else OPEN
    out.append(Chunk("group_edges/b/%d" % fmt, cfg, recs, kinds,
                     notes=dict(openers=[T - 1, T + 10, T + 11, 2 * T - 1], closers=[5, T], governed=[T + 12, 2 * T - 2], free=[6, T + 1, 2 * T, 2 * T + 39])))
    # a refused row inside a group
    recs = [row(0), opener(), row(1), row(2), BADROW, row(3)]
    out.append(Chunk("group_edges/bad/%d" % fmt, cfg, recs, [N, OPEN, N, N, BAD, N], notes=dict(openers=[1], closers=[], governed=[2, 3], free=[0])))
    return out


def _run(kind, k):
    if kind == "markers":
        return [CLOSER] * k, [CLOSE] * k
    if kind == "negative":
        return [NEG] * k, [SKIP] * k
    recs = [CLOSER if i % 3 == 0 else NEG for i in range(k)]
    return recs, [CLOSE if i % 3 == 0 else SKIP for i in range(k)]


def _seq(parts):
    """parts: ints (that many printing rows) and (kind, k) runs"""
    recs, kinds, runs = [], [], []
    for p in parts:
        if isinstance(p, int):
            recs += [row(len(recs) + i) for i in range(p)]; kinds += [N] * p
        else:
            a, b = _run(*p)
            runs.append((len(recs), len(recs) + len(a) - 1))
            recs += a; kinds += b
    return recs, kinds, runs


def skip_runs(fmt):
    cfg = CFG(fmt)
    out = []

    def add(name, parts, limit):
        recs, kinds, runs = _seq(parts)
        out.append(Chunk("skip_runs/%s/%d" % (name, fmt), cfg, recs, kinds, notes=dict(runs=runs, limit=limit)))
    for kind in ("markers", "negative", "mixed"):
        for k in (SKIP_LIMIT - 1, SKIP_LIMIT):
            for last in (T - 2, T - 1, T):                          # tile 0 into tile 1 where last = T
                add("%s-%d-%d" % (kind, k, last), [last - k + 1, (kind, k), 3], k >= SKIP_LIMIT)
    add("whole-tile", [T - 24, ("mixed", T + 76), 3], True)
    # 999 skipped, one printing row, 999 skipped: the printing row in the tile before / in the same tile as the row behind the second run
    add("999-1-999-carry", [20, ("negative", 999), 1, ("mixed", 999), 4], False)            # printing rows at 1019 (tile 0) and 2019 (tile 1)
    add("999-1-999-first-lane", [2 * T - 1999, ("markers", 999), 1, ("negative", 999), 4], False)    # ... at 2T-1000 (tile 1) and 2T (first of tile 2)
    add("999-total", [10, ("negative", 500), 1, ("negative", 499), 5], False)               # 999 skipped rows, no marker: no group pass
    add("1000-total", [10, ("negative", 500), 1, ("negative", 500), 5], False)              # 1000, never 1000 in a row: the group pass, no limit
    return out


def _nested(depth):
    v = 1
    for _ in range(depth):
        v = [v]
    return v


def null_rows(fmt, depth=None):
    """the rows on which the reference returns NULL: the temporary map passes 32 open containers, the input does not"""
    if fmt == JSON:
        return [ev(SEC, 5, mp(KV([(b"k", 1)])), mp(KV([(b"m", _nested(29 if depth is None else depth))])))], [N]
    return [opener(mp(KV([(b"a", _nested(30 if depth is None else depth))]))), row(1)], [OPEN, N]


def walk_order(fmt):
    """B = a row the decoder refuses, N = a row on which the reference returns NULL, L = a row behind 1000 skipped rows, in every order, 70
    printing rows in front of each (so each sits in a wave of its own)"""
    cfg = CFG(fmt)
    out = []
    items = {"B": lambda: ([BADROW], [BAD]), "N": lambda: null_rows(fmt), "L": lambda: _run("negative", SKIP_LIMIT),
             "l": lambda: _run("negative", SKIP_LIMIT - 1)}
    for order in ("BNL", "BLN", "NBL", "NLB", "LBN", "LNB", "lNB", "lBN"):
        recs, kinds = [], []
        for x in order:
            recs += [row(len(recs) + i) for i in range(70)]; kinds += [N] * 70
            a, b = items[x]()
            recs += a; kinds += b
        recs += [row(i) for i in range(10)]; kinds += [N] * 10
        out.append(Chunk("walk_order/%s/%d" % (order, fmt), cfg, recs, kinds, notes=dict(order=order)))
    # skipped rows directly in front of the NULL row: 1000 hide it.  In format json the NULL row is one row and 999 do not hide it; in
    # format lines the opener in front of it is a skipped row itself: 999 still hide it, 998 do not
    for k in (SKIP_LIMIT, SKIP_LIMIT - 1, SKIP_LIMIT - 2):
        recs, kinds = [row(i) for i in range(70)], [N] * 70
        for a, b in (_run("negative", k), null_rows(fmt)):
            recs += a; kinds += b
        recs += [row(i) for i in range(10)]; kinds += [N] * 10
        out.append(Chunk("walk_order/hide-%d/%d" % (k, fmt), cfg, recs, kinds, notes=dict(hide=k)))
    return out


# ------------------------------------------------------------------------------------------ (d) values
def float_list():
    """doubles: odd m * 2^-k (17 significant digits exactly, ending in 5, where m * 2^-k has 17 - k digits in front of the point: the
    ties of %.16g), 10^(+-k) with its neighbours, random bit patterns, subnormals, whole numbers"""
    r = random.Random(1616)
    vals = []
    for k in range(1, 24):                                          # exact ties: the digits of m / 2^k are those of m * 5^k, 17 of them
        lo, hi = -(-10 ** 16 // 5 ** k), min(10 ** 17 // 5 ** k + 1, 2 ** 53)
        for _ in range(8 if lo < hi else 0):
            m = r.randrange(lo, hi) | 1
            vals.append(m / 2.0 ** k)
            vals.append(-(m / 2.0 ** k))
    for k in range(1, 60):
        for _ in range(200):
            m = r.getrandbits(r.randrange(2, 54)) | 1
            vals.append(m / 2.0 ** k)
    for k in range(0, 308):
        for s in ("1e%d" % k, "1e-%d" % k):
            b = struct.unpack(">Q", struct.pack(">d", float(s)))[0]
            vals += [struct.unpack(">d", struct.pack(">Q", b + d))[0] for d in (-2, -1, 0, 1, 2)]
    vals += [struct.unpack(">d", struct.pack(">Q", r.getrandbits(64)))[0] for _ in range(30000)]
    vals += [struct.unpack(">d", struct.pack(">Q", r.getrandbits(52) | (r.getrandbits(1) << 63)))[0] for _ in range(2000)]
    for _ in range(1500):                                           # whole numbers: "%.1f" below 2^63 and at -2^63, "%.16g" from 2^63 on
        m, e = r.getrandbits(r.randrange(1, 54)), r.randrange(0, 12)
        vals.append(float(m * 2 ** e) * r.choice((1, -1)))
    vals += [0.0, -0.0, 2.0 ** 63, -(2.0 ** 63), 2.0 ** 63 - 1024, 2.0 ** 64, float("inf"), float("-inf"), float("nan"), -float("nan"), 5e-324, 1.7976931348623157e308]
    return vals


def py_float_rule(x, nan_to_null):
    """msgpack2json's float rule (src/flb_pack.c:1020-1034) said with Python's correctly rounded formatting"""
    if x != x:
        return "null" if nan_to_null else ("-nan" if struct.pack(">d", x)[0] & 0x80 else "nan")
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    if (abs(x) < 2.0 ** 63 or x == -(2.0 ** 63)) and x == int(x):
        return "%.1f" % x
    return "%.16g" % x


def floats(width, nan):
    vals = float_list()
    if width == 64:
        recs = [ev(SEC, 5, b"\x81\xa1f\xcb" + struct.pack(">d", v)) for v in vals]
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            f32 = np.asarray(vals, dtype=np.float64).astype(np.float32)
        recs = [ev(SEC, 5, b"\x81\xa1f\xca" + struct.pack(">I", int(b))) for b in f32.view(np.uint32)]
        vals = [float(v) for v in f32]
    return Chunk("floats/%d/%d" % (width, nan), CFG(LINES, dk=None, nan=nan), recs, notes=dict(vals=vals))


def dates(df):
    r = random.Random(20000101)
    ts = [(r.randrange(0, 2 ** 32 - 2), r.randrange(0, 10 ** 9)) for _ in range(65536)]
    day = 86400
    special = [951782400, 951782400 + day - 1, 951782400 + day, 1078012800, 1078099199, 4107542400 - day, 4107542400, 68169600, 946684799, 946684800,
               2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3, 0, 1, day - 1, day]
    ts += [(s, ns) for s in special for ns in (0, 1, 999, 1000, 999999, 1000000, 499999999, 999999999)]
    recs = [ev(s, ns, b"\x80") for s, ns in ts]
    recs += [mp([t, {}]) for t in (0, 1, SEC, 2 ** 32, 253402300799, 253402300800, 2 ** 40, 2 ** 40 - 1, 2 ** 33 + 5)]
    recs += [mp([t, {}]) for t in (0.0, 1.25, 1700000000.5, 1700000000.123456789, 4294967296.75, 0.999999999, 951782400.000001)]
    return Chunk("dates/%d" % df, CFG(LINES, df=df), recs)


def _srow(s):
    return ev(SEC, 5, b"\x81\xa1s" + mp(s))


def strings(which, esc):
    cfg = CFG(LINES, dk=None, esc=esc)
    if which == "pairs":                                            # all 65 536 two-byte strings
        n = 65536
        a = np.zeros((n, 19), dtype=np.uint8)
        a[:, :17] = np.frombuffer(ev(SEC, 5, b"\x81\xa1s\xa2"), dtype=np.uint8)
        i = np.arange(n)
        a[:, 17] = i >> 8; a[:, 18] = i & 255
        return Chunk("strings/pairs/%d" % esc, cfg, blob=a.tobytes(), rlen=np.full(n, 19, dtype=np.uint64))
    if which == "seam":                                             # every byte behind a clean run of 0 .. 16 (the 16-byte block seam of j_str)
        return Chunk("strings/seam/%d" % esc, cfg, [_srow(b"a" * k + bytes([b])) for k in range(17) for b in range(256)])
    r = random.Random(3434)
    lead = [(0xc2, 0xdf), (0xe0, 0xe0), (0xe1, 0xec), (0xed, 0xed), (0xee, 0xef), (0xf0, 0xf0), (0xf1, 0xf3), (0xf4, 0xf4), (0xf5, 0xf7), (0xf8, 0xff),
            (0xc0, 0xc1), (0x80, 0xbf), (0x20, 0x7e)]
    cont = [(0x80, 0x8f), (0x90, 0x9f), (0xa0, 0xbf), (0x20, 0x7e), (0xc2, 0xf4), (0x00, 0x1f)]
    recs = []
    for _ in range(20000):
        s = bytes([r.randint(*r.choice(lead))] + [r.randint(*r.choice(cont[:3] if r.random() < 0.7 else cont)) for _ in range(r.choice((2, 3)))])
        recs.append(_srow(b"a" * r.choice((0, 0, 5, 13, 14, 15)) + s))
    return Chunk("strings/sampled/%d" % esc, cfg, recs)


def plain_chunk(fmt, n=300):
    """no markers, nothing skipped"""
    return Chunk("plain/%d" % fmt, CFG(fmt), [row(i, b"p" * (i % 50)) for i in range(n)])

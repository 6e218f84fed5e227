"""The named chunks of tests/fmt_chunks.py sit on the edges they are named for: asserted here on the CPU, from the oracle's output alone
(row lengths are the oracle's lines, zero at the rows the builder knows to print nothing), with fmt_plan -- the batch loop of k_fmt_emit
restated in Python -- for the staging edges.  tests/test_fmt_edges_gpu.py runs the same chunks on the device.

No chunk may be skipped or shrunk by a condition at run time: a chunk that cannot be built fails the test."""
import decimal
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fmt_chunks as fc
from fmt_chunks import FMT_STG, T, JSON, LINES, N, ALL_FMT, GROUP_FMT

BUILD = {
    "stg_edge": lambda: [fc.stg_edge(f) for f in ALL_FMT],
    "direct_rows": lambda: [fc.direct_rows(f, e) for f in ALL_FMT for e in (1, 0)],
    "batch_split": lambda: [c for f in ALL_FMT for c in fc.batch_split(f)],
    "zero_rows": lambda: [fc.zero_rows(f, m) for f in ALL_FMT for m in (0, 1)],
    "tail_waves": lambda: [c for f in ALL_FMT for c in fc.tail_waves(f)],
    "flush_seams": lambda: [c for f in ALL_FMT for c in fc.flush_seams(f)],
    "str_tails": lambda: [c for f in ALL_FMT for e in (1, 0) for c in fc.str_tails(f, e)],
    "group_edges": lambda: [c for f in GROUP_FMT for c in fc.group_edges(f)],
    "skip_runs": lambda: [c for f in GROUP_FMT for c in fc.skip_runs(f)],
    "walk_order": lambda: [c for f in GROUP_FMT for c in fc.walk_order(f)],
    "floats": lambda: [fc.floats(w, nan) for w in (64, 32) for nan in (0, 1)],
    "dates": lambda: [fc.dates(df) for df in range(5)],
    "strings": lambda: [fc.strings(w, e) for w in ("pairs", "seam", "sampled") for e in (1, 0)],
    "plain": lambda: [fc.plain_chunk(f) for f in ALL_FMT],
}
_cache = {}


def chunks(name):
    """the chunks of one family, built once and shared (with their oracle answers) by every test that needs them"""
    if name not in _cache:
        _cache[name] = BUILD[name]()
    return _cache[name]


def plan(c):
    return fc.fmt_plan(c.expect()["lens"], FMT_STG)


def text(c, r):
    e = c.expect()
    return e["out"][int(e["row_off"][r]):int(e["row_off"][r + 1])]


def test_constants_are_read_from_the_kernel_source():
    assert FMT_STG % 16 == 0 and FMT_STG >= 1024 and T % 64 == 0 and T >= 64


def test_fmt_plan_on_a_hand_made_wave():
    assert fc.fmt_plan([10, 6, 100, 0, 120, 1], 112) == [[(0, 2, 0, False), (2, 2, 0, False), (4, 0, 4, True), (5, 1, 12, False)]]
    assert fc.fmt_plan([1] * 65, 64) == [[(0, 64, 0, False)], [(0, 1, 0, False)]]


# ------------------------------------------------------------------------------------------ (a)
def test_stg_edge():
    for c in chunks("stg_edge"):
        p, lens, seen = plan(c), c.expect()["lens"], set()
        for r, align, d in c.notes["big"]:
            b = [x for x in p[r // 64] if x[0] == r % 64]
            assert len(b) == 1, (c.name, r)                         # first in its batch
            assert b[0][2] == align and int(lens[r]) + align == FMT_STG + d and b[0][3] == (d > 0), (c.name, r, b, int(lens[r]))
            seen.add((align, d))
        assert seen == {(a, d) for a in range(16) for d in (-1, 0, 1)}


def test_direct_rows():
    for c in chunks("direct_rows"):
        direct = [w * 64 + b[0] for w, wave in enumerate(plan(c)) for b in wave if b[3]]
        assert direct == c.notes["direct"] and {r % 64 for r in direct} == set(fc.DIRECT_LANES), (c.name, direct)
        assert len({r // 64 for r in direct}) == 4 and all(int(c.expect()["lens"][r]) > FMT_STG for r in direct)
        if c.cfg["json_format"] == LINES:
            tails = set()
            for r in direct:
                t = text(c, r)
                tails.add(len(t) - 1 - t.rindex(b"a"))
            assert tails >= set(range(3, 18)), (c.name, sorted(tails))
        dup = text(c, direct[2])
        assert b"dropped" not in dup and b'"q":1' not in dup and b"kept" in dup


def test_batch_split():
    for f in ALL_FMT:
        split, full, over, align = [c for c in chunks("batch_split") if c.cfg["json_format"] == f]
        p = plan(split)
        assert len(p[0]) >= 2 and not any(b[3] for b in p[0])
        assert plan(full)[0] == [(0, 64, 0, False)] and int(full.expect()["row_off"][64]) == FMT_STG
        po = plan(over)[0]
        assert po == [(0, 63, 0, False), (63, 1, po[1][2], False)] and int(over.expect()["row_off"][64]) == FMT_STG + 1
        pa = plan(align)
        assert pa[0] == [(0, 64, 0, False)] and int(align.expect()["row_off"][64]) == FMT_STG - 1
        assert pa[1][0][2] == 15 and len(pa[1]) == 2 and not pa[1][1][3], pa[1]


def test_zero_rows():
    for c in chunks("zero_rows"):
        e = c.expect()
        lens, first, last_mid, last_63, empty = e["lens"], False, False, False, False
        for w, wave in enumerate(plan(c)):
            for lo, m, align, direct in wave:
                assert not direct
                tot = int(lens[w * 64 + lo:w * 64 + lo + m].sum())
                first |= tot > 0 and lens[w * 64 + lo] == 0
                last_mid |= tot > 0 and lens[w * 64 + lo + m - 1] == 0 and lo + m < 64     # in front of the row that no longer fits
                last_63 |= tot > 0 and lens[w * 64 + lo + m - 1] == 0 and lo + m == 64
                empty |= tot == 0 and m == 64
        assert first and last_mid and last_63 and empty, (c.name, first, last_mid, last_63, empty)
        assert int(np.flatnonzero(lens)[0]) >= 64
        if c.cfg["json_format"] == JSON:
            assert e["out"].startswith(b'[{"date"') and e["out"].endswith(b"}]")


def test_tail_waves():
    for f in ALL_FMT:
        assert tuple(c.expect()["n"] for c in chunks("tail_waves") if c.cfg["json_format"] == f) == fc.TAIL_N == (1, 63, 64, 65, 255, 256, 257)


def test_flush_seams():
    for f in ALL_FMT:
        starts, ends, empties = set(), set(), 0
        for c in [c for c in chunks("flush_seams") if c.cfg["json_format"] == f]:
            lens, fr = c.expect()["lens"], fc.frame(c.cfg)
            assert c.n == 5 * 64 and int(lens.min()) == 2 + fr and int(lens.max()) <= 40 + fr
            empties += int((lens == 2 + fr).sum())
            for w, wave in enumerate(plan(c)):
                assert len(wave) == 1 and wave[0][:2] == (0, 64)
                starts.add(wave[0][2])
                ends.add((wave[0][2] + int(lens[w * 64:w * 64 + 64].sum())) & 15)
        assert starts == ends == set(range(16)) and empties >= 16, (f, sorted(starts), sorted(ends))


def test_str_tails():
    cs = chunks("str_tails")
    assert len(cs) == 3 * 2 * 33
    for c in cs:
        k = int(c.name.split("/")[1])
        assert c.blob.endswith(bytes([0xa0 | k]) + b"c" * k if k < 32 else b"\xd9" + bytes([k]) + b"c" * k) and c.expect()["n"] == 34
        assert b'"' + b"c" * k + b'"}' in text(c, 33)


# ------------------------------------------------------------------------------------------ (b)
def test_grid_chunks():
    c = fc.emit_second_trip(256)
    e = c.expect()
    assert c.n == e["n"] == 524485 and c.n > 256 * 8 * 256 + 64 * 3
    slow = np.arange(0, c.n, fc.SLOW_EVERY)
    assert (c.rlen[slow] > 21).all() and int((c.rlen == 21).sum()) == c.n - len(slow)
    assert int(e["lens"][slow].min()) > int(np.delete(e["lens"], slow).max()) and b"dropped" not in e["out"][:200] and b"the later one stays 0" in e["out"][:200]
    # the same builder at one compute unit (the size pass's cap is 32 blocks there); 256 units give 2 097 219 rows
    c = fc.size_second_trip(1)
    assert c.n == c.expect()["n"] == 32 * 256 + 64 + 3 and 256 * 32 * 256 + 64 + 3 == 2097219


# ------------------------------------------------------------------------------------------ (c)
def test_group_edges():
    for f in GROUP_FMT:
        cs = [c for c in chunks("group_edges") if c.cfg["json_format"] == f]
        openers, closers = set(), set()
        for c in cs:
            e = c.expect()
            assert e["groups"]
            for r in c.notes["openers"]:
                assert c.recs[r][4:8] == b"\xff\xff\xff\xff" and e["lens"][r] == 0
            for r in c.notes["closers"]:
                assert c.recs[r][4:8] == b"\xff\xff\xff\xfe" and e["lens"][r] == 0
            for r in c.notes["governed"]:
                assert b'"group_attributes":{' in text(c, r), (c.name, r)
            for r in c.notes["free"]:
                assert b"group_attributes" not in text(c, r), (c.name, r)
            openers |= set(c.notes["openers"]); closers |= set(c.notes["closers"])
        assert openers >= {0, T - 1, T, 2 * T - 1} and closers >= {T - 1, T}
        a, b, bad = cs
        assert b'"g":"2T-1"' in text(a, 2 * T) and b'"g":"2T-1"' in text(a, 4 * T + 4)        # one group over three tiles
        assert b'"g":"late"' in text(b, T + 12) and b"early" not in b.expect()["out"]            # the later opener governs
        r = next(i for i in range(2, T - 1) if i % 7 == 2)
        assert b'"group_attributes":{"g":0},"log_metadata":{"m":%d}' % r in text(a, r)
        r = next(i for i in range(2 * T, 2 * T + 40) if i % 7 == 2)                            # behind the opener with an empty body map
        assert b'"__internal__":{"group_attributes":{},"log_metadata":{"m":%d}}' % r in text(b, r) and b"__internal__" not in text(b, 2 * T)
        r = next(i for i in range(2, T - 1) if i % 11 == 3)
        assert b"first" not in text(a, r) and b"second" in text(a, r) and b"group_attributes" in text(a, r)
        assert bad.expect()["n"] == 4 and bad.expect()["out"].count(b"group_attributes") == 2


def test_skip_runs():
    for c in chunks("skip_runs"):
        e, name = c.expect(), c.name.split("/")[1]
        runs, limit = c.notes["runs"], c.notes["limit"]
        assert e["n"] == (runs[0][0] + fc.SKIP_LIMIT if limit else c.n), (c.name, e["n"])
        parts = name.split("-")
        if parts[0] in ("markers", "negative", "mixed"):
            k, last = int(parts[1]), int(parts[2])
            assert runs == [(last - k + 1, last)] and last in (T - 2, T - 1, T) and k in (999, 1000) and limit == (k == 1000)
            assert e["groups"] == (parts[0] != "negative" or k == 1000)
            kinds = set(c.kinds[runs[0][0]:last + 1].tolist())
            assert kinds == {"markers": {fc.CLOSE}, "negative": {fc.SKIP}, "mixed": {fc.CLOSE, fc.SKIP}}[parts[0]]
    by = {c.name.split("/")[1]: c for c in chunks("skip_runs") if c.cfg["json_format"] == LINES}
    assert by["whole-tile"].notes["runs"][0][0] < T and by["whole-tile"].notes["runs"][0][1] >= 2 * T
    c = by["999-1-999-carry"]
    assert c.notes["runs"] == [(20, 1018), (1020, 2018)] and 1019 < T <= 2019 and c.expect()["n"] == c.n
    c = by["999-1-999-first-lane"]
    assert c.notes["runs"] == [(2 * T - 1999, 2 * T - 1001), (2 * T - 999, 2 * T - 1)] and c.kinds[2 * T] == N and c.kinds[2 * T - 1000] == N
    assert T <= 2 * T - 1000 and c.expect()["n"] == c.n
    assert not by["999-total"].expect()["groups"] and by["1000-total"].expect()["groups"] and by["1000-total"].expect()["n"] == by["1000-total"].n


def _lines(recs, fmt):
    out = fc.oracle(b"".join(recs), fc.CFG(fmt), LINES if fmt == LINES else JSON)
    if out is None:
        return None
    return out.count(b"\n") if fmt == LINES else out.count(b'{"date"')


def test_walk_order():
    p = fc.row(1)
    for f in GROUP_FMT:
        null, _ = fc.null_rows(f)
        # each row has its effect behind one printing row
        assert _lines([p, fc.BADROW, p], f) == 1
        assert _lines([p] + null + [p], f) is None
        assert _lines([p] + fc.null_rows(f, 29 if f == LINES else 28)[0] + [p], f) == 3                  # one level less: prints
        assert _lines([p] + fc.null_rows(f, 31 if f == LINES else 30)[0] + [p], f) == 1                  # one level more: a decoder error
        assert _lines([p] + [fc.NEG] * 1000 + [p, p], f) == 1 and _lines([p] + [fc.NEG] * 999 + [p, p], f) == 3
        want = dict(BNL=70, BLN=70, NBL=None, NLB=None, LBN=70, LNB=70, lNB=None, lBN=140)
        for c in [c for c in chunks("walk_order") if c.cfg["json_format"] == f]:
            e = c.expect()
            if "order" in c.notes:
                w = want[c.notes["order"]]
            else:
                hidden = c.notes["hide"] >= (1000 if f == JSON else 999)
                w = 70 if hidden else None
            if w is None:
                assert e["out"] is None, c.name
            else:
                assert e["out"] is not None and int((e["lens"] > 0).sum()) == w, (c.name, w)


# ------------------------------------------------------------------------------------------ (d)
def test_floats_against_the_python_rule():
    ties = shapes = None
    for c in chunks("floats"):
        out = c.expect()["out"]
        got = out.split(b"\n")[:-1]
        vals, nan = c.notes["vals"], c.cfg["nan_to_null"]
        assert len(got) == len(vals) > 46000
        want = [fc.py_float_rule(v, nan) for v in vals]
        for g, w, v in zip(got, want, vals):
            assert g == b'{"f":%s}' % w.encode(), (c.name, v.hex(), g, w)
        if c.name == "floats/64/0":
            ties = 0
            for v in vals:
                if v == v and abs(v) != float("inf") and v != 0:
                    d = decimal.Decimal(v).as_tuple().digits
                    while d and d[-1] == 0:
                        d = d[:-1]
                    ties += len(d) == 17 and d[-1] == 5
            # the three print shapes: "%.1f" of a whole number, "%.16g" in fixed and in exponent notation
            finite = [(v, w) for v, w in zip(vals, want) if v == v and abs(v) != float("inf")]
            whole = sum(1 for v, w in finite if v == int(v) and w == "%.1f" % v)
            expo = sum(1 for v, w in finite if "e" in w)
            shapes = [whole, len(finite) - whole - expo, expo]
    assert ties >= 20 and min(shapes) >= 1000, (ties, shapes)


def test_dates_and_strings_print_every_row():
    for c in chunks("dates") + chunks("strings"):
        assert c.expect()["n"] == c.n >= 4352 and int((c.expect()["lens"] > 0).sum()) == c.n
    assert [c.n for c in chunks("strings")] == [65536, 65536, 4352, 4352, 20000, 20000]

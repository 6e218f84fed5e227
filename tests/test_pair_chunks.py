"""The named chunks of tests/pair_chunks.py on the CPU oracle alone (filter_parser then filter_grep, the way flb_filter_do runs them):
every chunk keeps some of its records and drops some -- otherwise the fused pair hands it to the unfused kernels and the device test
would test nothing -- and the batching model of k_pg_emit, fed the ORACLE's record sizes, shows the edge the chunk is named for.  A
named edge that no chunk covers is a failure.  The device side: tests/test_pair_emit_gpu.py."""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_binding as ob
import pair_chunks as pc


def _skip(b, p):
    """the position behind the msgpack object at p"""
    t = b[p]
    if t < 0x80 or t >= 0xe0 or t in (0xc0, 0xc2, 0xc3):
        return p + 1
    if t < 0x90:
        n, p = 2 * (t & 15), p + 1
    elif t < 0xa0:
        n, p = t & 15, p + 1
    elif t < 0xc0:
        return p + 1 + (t & 31)
    elif t in (0xd9, 0xc4):
        return p + 2 + b[p + 1]
    elif t in (0xda, 0xc5):
        return p + 3 + int.from_bytes(b[p + 1:p + 3], "big")
    elif t in (0xdb, 0xc6):
        return p + 5 + int.from_bytes(b[p + 1:p + 5], "big")
    elif t in (0xcc, 0xd0):
        return p + 2
    elif t in (0xcd, 0xd1):
        return p + 3
    elif t in (0xce, 0xd2, 0xca):
        return p + 5
    elif t in (0xcf, 0xd3, 0xcb):
        return p + 9
    elif 0xd4 <= t <= 0xd8:
        return p + 2 + (1 << (t - 0xd4))
    elif t == 0xdc:
        n, p = int.from_bytes(b[p + 1:p + 3], "big"), p + 3
    elif t == 0xde:
        n, p = 2 * int.from_bytes(b[p + 1:p + 3], "big"), p + 3
    else:
        raise ValueError("msgpack type %#x" % t)
    for _ in range(n):
        p = _skip(b, p)
    return p


def split_records(b):
    out, p = [], 0
    while p < len(b):
        q = _skip(b, p)
        out.append(b[p:q])
        p = q
    return out


@functools.lru_cache(maxsize=None)
def _filters(pargs, rules, op):
    return ob.FilterParser("log", [ob.Parser(**dict(pargs))]), ob.Grep(list(rules), op)


def oracle_pair(c):
    """-> (ret of filter_parser, its output, ret of filter_grep, its output, keep_len per input row): the oracle's two filters one
    after the other; keep_len[r] = bytes of the record row r leaves in the pair's output (0: dropped).  Every input row gives one
    record behind filter_parser and filter_grep copies records as they are, so its output is matched against the parsed records."""
    fp, fg = _filters(tuple(sorted(c.pargs.items())), tuple(c.rules), c.op)
    blob = c.blob + c.tail
    r1, o1 = fp.filter(blob)
    assert r1 == ob.MODIFIED, c
    r2, o2 = fg.filter(o1)
    parsed = split_records(o1)
    assert len(parsed) == len(c.recs), (c, len(parsed))
    keep_len, kept, k = [0] * len(parsed), split_records(o2) if r2 == ob.MODIFIED else parsed, 0
    for r, rec in enumerate(parsed):
        if k < len(kept) and kept[k] == rec:
            keep_len[r] = len(rec)
            k += 1
    assert k == len(kept), c
    return r1, o1, r2, o2, keep_len


@functools.lru_cache(maxsize=None)
def _results(name):
    return [(c, oracle_pair(c)) for c in pc.group(name)]


def test_every_chunk_keeps_some_and_drops_some():
    """0 < kept < parsed, nothing unparsed that was meant to parse, no group-marker time: what run_pair_fused needs to stay fused"""
    for g in pc.GROUPS:
        for c, (r1, o1, r2, o2, keep_len) in _results(g):
            kept = sum(1 for x in keep_len if x)
            assert r2 == ob.MODIFIED and 0 < kept < len(keep_len), (g, c, kept)
            assert all(rec[4:8] not in (b"\xff\xff\xff\xff", b"\xff\xff\xff\xfe") for rec in split_records(o2)), (g, c)
    c = pc.unfused_queue_chunk()
    r1, o1, r2, o2, keep_len = oracle_pair(c)
    assert (r1, r2) == (ob.MODIFIED, ob.NOTOUCH) and keep_len == [len(o1)]


def test_layout_sizes_are_the_oracles():
    """parsed_size / apache_size, which lay the chunks out, against the oracle's record sizes, across the str-header steps"""
    for n in (0, 1, 31, 32, 33, 198, 255, 256, 9000, 65535 - pc.LINE_BASE, 65536 - pc.LINE_BASE):
        c = pc.Chunk("x", [pc.record(pc.apache_line(agent=b"a" * n)), pc.record(pc.apache_line(code=200))], pc.P_APACHE)
        assert oracle_pair(c)[4] == [pc.apache_size(n), 0], n
    assert [pc.agent_for_size(pc.apache_size(n)) for n in (1, 31, 32, 255, 256, 9400)] == [1, 31, 32, 255, 256, 9400]
    assert pc.agent_for_size(pc.apache_size(31) + 1) is None and pc.agent_for_size(pc.apache_size(255) + 1) is None


def _edges(results, stg):
    b = [x for c, res in results for x in pc.batches(res[4], stg)]
    return ({x.align for x in b if not x.direct and x.end == stg}, {x.align for x in b if not x.direct and x.end == stg - 1},
            {x.align for x in b if not x.direct and x.next_end == stg + 1})


def test_staging_sweep_reaches_every_alignment_at_both_sizes():
    every = set(range(16))
    for stg in (pc.PGE_STG_PLAIN, pc.PGE_STG_GENERAL):
        res = [(c, r) for c, r in _results("staging") if c.notes["stg"] == stg]
        exact, below, over = _edges(res, stg)
        assert exact == every, ("a batch ends at STG", stg, sorted(every - exact))
        assert below == every, ("a batch ends at STG - 1", stg, sorted(every - below))
        assert over == every, ("the next record would end at STG + 1", stg, sorted(every - over))
        for c, r in res:
            # each chunk sits on ITS edge, in the first batch of the second group; every kept value fits the register window
            b = [x for x in pc.batches(r[4], stg) if x.group == 1][0]
            d = c.notes["delta"]
            assert (b.end == stg + d if d <= 0 else b.next_end == stg + 1) and b.lo == 0, (c, b)
            assert all(pc.value_len(rec) <= pc.REG_WINDOW for rec in c.recs), c
        # the 16-byte flush has a ragged head AND a ragged tail, next to another batch's bytes on both sides
        assert any(x.align and x.end & 15 and x.rows[0] > 0 and x.rows[-1] + 2 < len(r[4]) for c, r in res for x in pc.batches(r[4], stg)), stg


def test_one_record_around_the_staging_size():
    for stg in (pc.PGE_STG_PLAIN, pc.PGE_STG_GENERAL):
        seen = set()
        for c, r in _results("one_big"):
            if c.notes.get("stg") != stg:
                continue
            b = pc.batches(r[4], stg)
            big = [x for x in b if 1 in x.rows][0]
            a, d = c.notes["align"], c.notes["delta"]
            assert big.rows == [1] and big.align == a and big.end == stg + d and big.direct == (d > 0), (c, big)
            assert pc.value_len(c.recs[1]) > pc.REG_WINDOW and sum(1 for x in r[4] if x) < 64          # no descriptor; the plain build stays chosen
            seen.add((a, d))
        assert seen == {(a, d) for a in range(16) for d in (-1, 0, 1)}, stg
    c, r = _results("one_big")[-1]
    for stg in (pc.PGE_STG_PLAIN, pc.PGE_STG_GENERAL):
        b = pc.batches(r[4], stg)
        assert [x.direct for x in b] == [False, True, False] and [len(x.rows) for x in b] == [5, 1, 5] and len({x.group for x in b}) == 1, (c, b)


def test_full_batch_of_64():
    for c, r in _results("full_batch"):
        for stg in (pc.PGE_STG_PLAIN, pc.PGE_STG_GENERAL):
            b = pc.batches(r[4], stg)
            assert len(b[0].rows) == 64 and not b[0].direct and b[0].next_end is None, (c, b)
            assert [len(x.rows) for x in b] == {64: [64], 65: [64, 1], 128: [64, 64]}[c.notes["kept"]], (c, b)
        assert max(r[4]) < 128, c


def test_queue_patterns_reach_the_seams():
    counts, kept_rows, ns, last_only, last_kept = set(), set(), set(), False, False
    follows = set()
    for c, r in _results("queue"):
        keep_len = r[4]
        assert [i for i, x in enumerate(keep_len) if x] == c.notes["kept"], c
        w = pc.wave_kept(keep_len)
        counts.update(w)
        follows.update(zip(w, w[1:]))
        kept_rows.update(c.notes["kept"])
        ns.add(len(keep_len))
        last_kept |= bool(keep_len[-1])
        last_only |= c.notes["kept"] == [len(keep_len) - 1]
    assert {0, 1, 63, 64, 65, 512} <= counts, sorted(counts)
    assert set(pc.SEAM_ROWS) <= kept_rows
    assert ns | {1} == set(pc.QUEUE_N) and {511, 513, 2049} <= ns
    assert last_kept and last_only
    assert (512, 0) in follows and (0, 512) in follows            # a full window in front of an empty one, and the mirror image
    # rows 2047 / 2048: the last row of a workgroup's rows and the first of the next one's
    assert pc.PGE_WORKGROUP_ROWS - 1 in pc.SEAM_ROWS and pc.PGE_WORKGROUP_ROWS in pc.SEAM_ROWS


def test_tails_sit_where_they_are_named():
    seen = set()
    for c, r in _results("tails"):
        keep_len, ll = r[4], c.notes["agent"]
        want = pc.apache_size(ll)
        b = pc.batches(keep_len, pc.PGE_STG_PLAIN)
        assert keep_len[63] == want and b[0].rows[-1] == 63 and keep_len[64] == pc.apache_size(21), c       # last of its batch, the neighbour behind it
        last_kept = max(i for i, x in enumerate(keep_len) if x)
        assert keep_len[last_kept] == want, c
        seen.add((ll, last_kept == len(keep_len) - 1, bool(c.tail)))
        assert all(pc.value_len(rec) <= pc.REG_WINDOW for rec in c.recs)
    assert seen == {(ll, e, t) for ll in pc.TAIL_LENGTHS for e in (True, False) for t in (True, False)}
    assert {ll % 16 for ll in pc.TAIL_LENGTHS} >= {0, 1, 15} and 0 in pc.TAIL_LENGTHS


def test_time_text_at_the_chunks_end():
    lefts = set()
    for c, r in _results("time_end"):
        if c.notes.get("middle"):
            assert r[4][3] and b"Foo" in c.recs[3]
            continue
        keep_len = r[4]
        assert keep_len[-1] and not c.tail, c                     # the last record is kept: `left` is what the notes say
        blob = c.blob
        at = blob.rindex(b"[") + 1
        assert len(blob) - at == c.notes["left"], c
        lefts.add((c.notes["left"], c.notes["odd"]))
    assert {x for x, odd in lefts if not odd} == {27, 28, 31, 32, 33, 48} == {x for x, odd in lefts if odd}


def test_field_counts_and_metadata():
    nfs = set()
    for c, r in _results("fields"):
        if "nf" in c.notes:
            nfs.add(c.notes["nf"])
            kept = [x for x in r[4] if x]
            assert len(c.recs) == 200 and len(kept) == 67, c
            # (body map at byte 13) the header's width follows the PARSER's field count -- 0x8n below 16 named groups, de 00 nn from 16 on,
            # whatever is left after the empty fields are skipped; some kept record has every field, some have empty ones skipped
            entries = {rec[15] if rec[13] == 0xde else rec[13] & 15 for rec in split_records(r[3])}
            assert max(entries) == c.notes["nf"] and (c.notes["nf"] < 3 or min(entries) < c.notes["nf"]), (c, entries)
            assert all((rec[13] == 0xde) == (c.notes["nf"] >= 16) for rec in split_records(r[3])), c
        else:
            assert any(r[4][i] for i in c.notes["meta_rows"]) and not all(r[4][i] for i in c.notes["meta_rows"]), c
            assert any(rec[12:16] == b"\x81\xa1k\xa1" for rec in split_records(r[3])), c
    assert nfs == set(pc.FIELD_COUNTS) and {15, 16} <= nfs and max(nfs) == 31


def test_value_length_seams():
    (c1, r1), (c2, r2) = _results("values")
    assert [pc.value_len(rec) for rec, x in zip(c1.recs, r1[4]) if x] == list(range(268, 277)) and pc.REG_WINDOW == 272
    kept = [i for i, x in enumerate(r2[4]) if x]
    big = [i for i in kept if r2[4][i] > 60000]
    assert [pc.value_len(c2.recs[i]) for i in big] == [65534, 65535, 65536]
    assert all(0 < r2[4][i - 1] < 200 and 0 < r2[4][i + 1] < 200 for i in big), "each between two ordinary kept records"


def test_rule_chunks_depend_on_the_last_byte():
    for c, r in _results("rules"):
        keep_len = r[4]
        if c.notes.get("big_tables"):
            agents = [rec[rec.rindex(b'" "') + 3:-1] for rec in c.recs]
            assert {len(a) for a in agents} >= {12, 16, 17, 33}
            # the rule walked in global memory decides: some records pass the two staged rules and fail on the last byte alone
            by_stem = {}
            for a, x in zip(agents, keep_len):
                by_stem.setdefault(a[:-1], []).append((a[-1:], bool(x)))
            assert any(sorted(v) == [(b"Y", False), (b"Z", True)] for v in by_stem.values()), c
            assert any(sorted(v) == [(b"Y", False), (b"Z", False)] for v in by_stem.values()), c
            continue
        got = {}
        for rec, x in zip(c.recs, keep_len):
            agent = rec[rec.rindex(b'" "') + 3:-1]
            got[(len(agent), agent[-1:])] = bool(x)
        assert got == {(ll, last if ll else b""): (last == b"Z" and ll > 0) for ll in pc.RULE_FIELD_LENGTHS for last in (b"Z", b"Y")}, (c, got)

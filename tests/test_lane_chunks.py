"""The builders of tests/lane_chunks.py reach what they claim -- computed from the bytes they emit, with the CPU references, no GPU.
(tests/test_lane_edges_gpu.py runs the same chunks through k_json_lane, k_grep_lane and k_l2m_lane.)"""
import struct
import pytest
import jsonfuzz as jf
import oracle_binding as ob
import lane_chunks as lc
from synth import unpack_all


@pytest.fixture(scope="module")
def cases():
    return lc.json_cases()


@pytest.fixture(scope="module")
def oj():
    o, memo = jf.oracle(), {}

    def f(row):
        if row not in memo:
            memo[row] = o(row)
        return memo[row]
    return f


def one_object(oj, row):
    w = oj(row)
    return w[0] == 0 and w[3] == 1 and w[2] == 1 and row[w[4]:].strip(b" \t\r\n") == b""


# ---------------------------------------------------------------------------------------------------------------- JSON
def test_json_cases_have_an_answer_and_a_reason(cases, oj):
    seen = set()
    names = set()
    for fam, cs in cases.items():
        for c in cs:
            assert (fam, c.name) not in names, (fam, c.name)
            names.add((fam, c.name))
            w = oj(c.row)
            assert w[0] != 0 or (w[4] <= len(c.row) and (len(w[1]) <= len(c.row) or c.cond == "primitive_longer")), (fam, c.name)
            blank = c.row.strip(b" \t\r\n") == b""
            if c.taken:
                # what the pass takes is blank or exactly one object -- and then the reference writes it no longer than the text
                assert c.cond is None and (blank or one_object(oj, c.row)), (fam, c.name)
            else:
                assert c.cond in lc.CONDS and c.cond != "fit", (fam, c.name)
                seen.add(c.cond)
                # "one_object" is the only reason that is about the row's grammar: the others are valid single objects
                assert (c.cond == "one_object") == (not one_object(oj, c.row)) or c.cond in ("escape", "control"), (fam, c.name, c.cond)
    assert seen == set(lc.CONDS) - {"fit"}, set(lc.CONDS) - seen


def test_json_reasons_show_in_the_bytes(cases):
    for fam, cs in cases.items():
        for c in cs:
            if c.cond == "escape":
                assert b"\\u" in c.row or b"\\x" in c.row
            if c.cond == "control":
                assert any(b < 0x20 for b in c.row.rstrip(b"\r\n"))
            if c.cond == "depth":
                assert max(sum(1 if ch in b"{[" else -1 for ch in c.row[:i] if ch in b"{[]}") for i in range(len(c.row))) == 9
            if c.cond == "exact_decimal":
                assert lc.HARD_DECIMAL in c.row and len(lc.HARD_DECIMAL.replace(b".", b"")) == 40
            if c.cond == "string_moves_up":
                key = c.row.split(b'"')[1]
                assert (len(key) > 31 and c.row.startswith(b'{"')) or (len(key) > 255 and c.row.startswith(b'{ "'))
    depth_ok = [c for c in cases["nesting"] if c.taken]
    assert len(depth_ok) == 6                          # seven and eight open containers, three ways each


def test_json_string_and_number_families_cover_the_listed_edges(cases, oj):
    assert [len(unpack_all(oj(c.row)[1])[0][1][0][1]) for c in cases["string_values"][::2]] == lc.STR_LENS
    assert [len(unpack_all(oj(c.row)[1])[0][1][1][0]) for c in cases["string_keys"]] == lc.STR_LENS
    assert [unpack_all(oj(c.row)[1])[0][1][0][1] for c in cases["numbers_alone"][:len(lc.INTS)]] == [v if abs(v) < 2 ** 64 and v >= -2 ** 63 else float(v) for v in lc.INTS]
    # every msgpack integer width, both signs
    heads = {oj(c.row)[1][3] for c in cases["numbers_alone"][:len(lc.INTS)]}
    assert {0xcc, 0xcd, 0xce, 0xcf, 0xd0, 0xd1, 0xd2, 0xd3, 0xcb, 0x00, 0x7f, 0xff, 0xe0} <= heads
    # the escape runs change the header's size: raw 33 / 34 -> 31 / 32, raw 257 / 258 -> 255 / 256
    got = {c.name: oj(c.row)[1][3:6] for c in cases["escapes"] if c.name.startswith("run")}
    assert got["run33to31"][0] == 0xbf and got["run34to32"][:2] == b"\xd9\x20" and got["run257to255"][:2] == b"\xd9\xff" and got["run258to256"] == b"\xda\x01\x00"
    q = {c.name: c.row for c in cases["escapes"]}
    assert q["quote_16th"][6 + 15:6 + 16] == b'"' and q["quote_16th"][6 + 14:6 + 15] == b"\\" and q["quote_17th"][6 + 16:6 + 17] == b'"'
    for c in cases["utf8"]:
        o = int(c.name.split("@")[1])
        assert c.row[6 + o] >= 0x80 and c.row[6 + o - 1] < 0x80 and (o // 4 != (o + int(c.name[5]) - 1) // 4)      # straddles a 4-byte step
    assert any(int(c.name.split("@")[1]) // 16 != (int(c.name.split("@")[1]) + int(c.name[5]) - 1) // 16 for c in cases["utf8"])
    for n in (16, 17, 40):
        for c in cases["containers"]:
            if c.name.startswith(("root_obj%d" % n, "obj%d" % n)):
                assert b"\xde\x00" + bytes([n]) in oj(c.row)[1], c.name
            if c.name.startswith("arr%d_" % n):
                assert b"\xdc\x00" + bytes([n]) in oj(c.row)[1], c.name


def test_json_copy_out_rows_have_the_listed_lengths(cases, oj):
    assert [len(oj(c.row)[1]) for c in cases["copy_out"]] == lc.COPY_LENS
    assert len(set(struct.pack(">II", *lc.TS))) == 8


def test_json_case_chunks_put_the_row_where_they_say(cases):
    for fam, cs in cases.items():
        for c in cs:
            rows, pos = lc.json_case_chunk(c)
            have, R, cap = lc.fits(rows, lc.json_geometry)
            assert all(have), (fam, c.name)                            # no row of a case chunk is left for its length
            assert [p % R for p in pos[:3]] == [0, R // 2, R - 1] and len({p // R for p in pos}) == len(pos), (fam, c.name, R)
            assert all(rows[p] is c.row for p in pos) and sum(r is c.row for r in rows) == len(pos)
            if c.at_end:
                assert rows[-1] is c.row and not c.row.endswith(b"\n")


@pytest.mark.parametrize("align", [0, 5, 15])
def test_json_fit_sweep(oj, align):
    sweep = lc.json_fit_sweep(align)
    totals = [t for t, _, _ in sweep]
    assert min(totals) < lc.TEXT < max(totals) and totals == list(range(totals[0], totals[0] + 81))
    lefts = []
    for T, rows, left in sweep:
        have, R, cap = lc.fits(rows, lc.json_geometry)
        assert R == 64 and len(rows) == 576 and sum(len(r) for r in rows[64:128]) == T
        assert have.count(False) == left and (left == 0 or have.index(False) == 127)
        lefts.append(left)
        assert all(one_object(oj, r) for r in rows[120:130])
    assert lefts == sorted(lefts) and lefts[0] == 0 and lefts[-1] == 1
    # the boundary itself: a tile that ends exactly at the capacity fits, one byte more does not
    ends = {T + align: left for T, _, left in sweep}
    assert ends[lc.TEXT] == 0 and ends[lc.TEXT + 1] == 1
    assert sum(len(r) for r in sweep[0][1][:64]) % 16 == align


def test_json_staging_families(oj):
    for L in (16001, 40000):
        for where in (0, 31, 63):
            rows, left = lc.json_too_long(L, where)
            have, R, cap = lc.fits(rows, lc.json_geometry)
            assert R == 64 and len(rows[128 + where]) == L > lc.TEXT
            assert [i for i, h in enumerate(have) if not h] == list(range(128 + where, 192)) and left == 64 - where
    for L, n, R_want in ((400, 77, 36), (400, 130, 36), (3000, 9, 4), (14000, 3, 1), (14000, 2, 1), (100, 2, 64), (100, 3, 64)):
        have, R, cap = lc.fits(lc.json_uniform(L, n), lc.json_geometry)
        assert R == R_want and all(have)
    assert (77 + 35) // 36 % 2 == 1 and 77 % 36 and (9 + 3) // 4 % 2 == 1 and 9 % 4      # a partial last tile, a last workgroup with a wave to spare
    starts, ends = set(), set()
    for a in range(16):
        for e in range(16):
            rows, left = lc.json_align(a, e)
            have, R, cap = lc.fits(rows, lc.json_geometry)
            assert R == 64 and all(have) and len(rows) == 130
            starts.add(sum(len(r) for r in rows[:64]) % 16)
            ends.add(sum(len(r) for r in rows) % 16)
    assert starts == ends == set(range(16))
    rows, left = lc.json_align(3, 4, "open_string")
    assert left == 1 and not one_object(oj, rows[-1]) and rows[-1].count(b'"') % 2 == 1
    rows, left = lc.json_align(3, 4, "no_newline")
    assert left == 0 and one_object(oj, rows[-1]) and not rows[-1].endswith(b"\n")
    big = lc.json_big()
    R, _ = lc.json_geometry(sum(len(r) for r in big), len(big))
    assert len(set(big)) == 42 and (len(big) + R - 1) // R > 2 * 256                    # more workgroups (two tiles each) than one look-back window


# ---------------------------------------------------------------------------------------------------------------- log events
def test_events_are_plain_and_sized():
    for size in list(range(100, 140)) + [400, 3000, 14000, 16001, 16015, 40000]:
        for keep in (True, False):
            r = lc.event(size, size, keep=keep)
            assert len(r) == size and lc.plain_event(r)
            got = ob.Grep(*lc.A_RULES).filter(r)
            assert (got[0] == ob.NOTOUCH) == keep
    assert 16001 % 16 == 1 and 16015 % 16 == 15 and 40000 % 16 == 0


@pytest.mark.parametrize("which", ["grep", "l2m"])
def test_record_staging_families(which):
    geometry = lc.grep_geometry if which == "grep" else lc.l2m_geometry
    sweep = lc.fit_sweep(geometry)
    overs = [o for o, _ in sweep]
    assert len(sweep) == 16 and overs == sorted(overs) and overs[0] < -400 and 0 in overs and 1 in overs and overs[-1] >= 300
    for over, recs in sweep:
        have, R, cap = lc.fits(recs, geometry)
        assert R == 64 and len(recs) == 320 and all(lc.plain_event(r) for r in recs)
        tile = sum(len(r) for r in recs[64:128])
        assert tile - cap == over
        miss = [i for i, h in enumerate(have) if not h]
        assert (miss == []) == (over <= 0) and all(64 <= i < 128 for i in miss) and (not miss or miss[-1] == 127)
    for L in (16001, 16015, 40000):
        for behind in (0, 1, 5, 60, 63):
            recs, at = lc.too_long(L, behind, True)
            have, R, cap = lc.fits(recs, geometry)
            assert R == 64 and len(recs[at]) == L and at % 64 == 63 - behind
            assert [i for i, h in enumerate(have) if not h] == list(range(at, 192))
            kept = ob.Grep(*lc.A_RULES).filter(b"".join(recs[at:192]))
            assert kept[0] == ob.NOTOUCH                                 # the long record and what stands behind it are all kept
            assert ob.Grep(*lc.A_RULES).filter(lc.too_long(L, behind, False)[0][at])[1] == b""
    for L, n, R_want in ((400, 187, 36), (3000, 21, 4), (14000, 5, 1), (14000, 1, 1), (120, 1, 64), (120, 2, 64)):
        have, R, cap = lc.fits(lc.uniform(L, n), geometry)
        assert R == R_want and all(have)
        assert n < 5 or (((n + R - 1) // R) % 4 != 0 and (n % R != 0 or R == 1))
    starts, ends = set(), set()
    for a in range(16):
        for e in range(16):
            recs = lc.aligned(a, e)
            have, R, cap = lc.fits(recs, geometry)
            assert R == 64 and all(have)
            starts.add(sum(len(r) for r in recs[:64]) % 16)
            ends.add(sum(len(r) for r in recs) % 16)
    assert starts == ends == set(range(16))


def test_large_grep_chunks():
    for over in (False, True):
        recs = lc.tile_max_chunk(over)
        assert len(recs) >= 65536 and len(set(recs)) <= 13
        lens = [len(r) for r in recs]
        s = lens.index(384)
        assert s % 64 not in (0, 1) and lens[s:s + 63] == [384] * 63 and lens[s - 1] == 96 and (lens[s + 63] > 16384) == over
    recs, flags = lc.run_pattern_chunk()
    assert len(recs) == 70000 and (len(recs) + 255) // 256 > 256 and len(set(recs)) == 5
    o = ob.Grep(*lc.A_RULES)
    assert all((o.filter(r)[0] == ob.NOTOUCH) == k for r, k in {(r, k) for r, k in zip(recs, flags)})
    runs = [i for i in range(1, len(flags)) if flags[i] != flags[i - 1]]
    assert len({b - a for a, b in zip(runs, runs[1:])}) >= 10
    unit_bytes = {sum(len(r) for r, k in zip(recs[u:u + 256], flags[u:u + 256]) if k) for u in range(0, 70000, 256)}
    assert len(unit_bytes) > 100                                         # the look-back's words differ


# ---------------------------------------------------------------------------------------------------------------- grep families
def _decide(rules, op, row):
    r, out = ob.Grep(rules, op).filter(row)
    return r == ob.NOTOUCH or out != b""


def test_name_records():
    for n in lc.NAME_LENS:
        k = lc.name(n)
        recs = lc.name_records(n)
        keys = {}
        for what, body, plain in recs:
            r = lc.rec(body)
            assert lc.plain_event(r) == plain, (n, what)
            keys[what] = [kv[0] for kv in unpack_all(r)[0][1][1]]
            kept = _decide([("regex", k.decode() + " ^hit$")], None, r)
            assert kept == (what in ("exact", "forty", "twice_hit_last", "final_key", "str8_name", "str16_name")), (n, what)
        assert keys["exact"] == [k] and len(keys["shorter"][0]) == n - 1 and len(keys["longer"][0]) == n + 1
        assert keys["last_byte"][0][:-1] == k[:-1] and keys["last_byte"][0] != k and len(keys["forty"][0]) == 40
        if n >= 9:
            b9 = keys["byte9"][0]
            assert b9[:8] == k[:8] and b9[8] != k[8] and b9[9:] == k[9:] and len(b9) == n
        # the name is the body's last key: the dwords the walk reads for it run to the record's end or past it
        r = lc.rec(dict(recs)["final_key_empty_value"] if False else [b for w, b, _ in recs if w == "final_key_empty_value"][0])
        assert r.endswith(k + b"\xa0")


def test_value_records():
    vals = lc.value_records()
    for what, v, plain in vals:
        r = lc.rec({b"log": v})
        assert lc.plain_event(r) == plain, what
        for pat in lc.VALUE_PATTERNS:
            _decide([("regex", "log " + pat)], None, r)                  # a definite answer, no exception
    enc = {what: lc.rec({b"log": v})[13 + 1 + 4:][:1] for what, v, _ in vals}
    assert enc["a*5"] == b"\xa5" and enc["a*5 as str8"] == b"\xd9" and enc["a*5 as str16"] == b"\xda" and enc["a*32"] == b"\xd9" and enc["a*256"] == b"\xda"
    for what, v, _ in vals:
        if what.startswith("Q ends at"):
            assert v.index(b"Q") + 1 == int(what.split()[3].rstrip(","))
        if what.startswith("é at"):
            assert lc.nonascii_offset(v) == int(what.split()[2].rstrip(","))
    assert {lc.nonascii_offset(v) % 4 for w, v, _ in vals if w.startswith("é at")} == {0, 1, 2, 3}
    assert {(v.index(b"Q")) % 4 for w, v, _ in vals if w.startswith("Q ends")} == {0, 1, 2, 3}
    for what, body, plain in lc.subkey_records():
        r = lc.rec(body)
        assert lc.plain_event(r) == plain, what
        for rule in lc.SUBKEY_RULES:
            _decide([("regex", rule)], None, r)
    hits = [w for w, b, _ in lc.subkey_records() if _decide([("regex", lc.SUBKEY_RULES[0])], None, lc.rec(b))]
    assert hits == ["fixmap parents", "map16 parent", "map16 inner", "child twice, hit last", "parent twice", "long child key", "parent is a string"]


def test_rule_count_records():
    for n in lc.RULE_COUNTS:
        rules = lc.count_rules(n, "regex")
        assert len(rules) == n and len({r.split()[0] for _, r in rules}) == min(n, 8)
        recs = dict(lc.count_records(n))
        for what, body in recs.items():
            assert lc.plain_event(lc.rec(body)), (n, what)
        single = lambda i, what: _decide([rules[i]], None, lc.rec(recs[what]))
        assert [single(i, "only the last") for i in range(n)] == [i == n - 1 for i in range(n)]
        assert [single(i, "all but the last") for i in range(n)] == [i != n - 1 or n == 1 and False for i in range(n)]
        assert all(single(i, "all") for i in range(n)) and not any(single(i, "none") for i in range(n))


def test_shape_and_copy_records():
    for what, row, plain, notouch in lc.shape_records():
        assert lc.plain_event(row) == plain, what
        r, out = ob.Grep(*lc.A_RULES).filter(lc.event(0, keep=False) + row)
        assert (r == ob.NOTOUCH) == notouch, what
    for s in lc.REC_LENS:
        r = lc.copy_record(s, True)
        assert len(r) == s and lc.plain_event(r) and _decide(*lc.COPY_RULES, r)
    assert not _decide(*lc.COPY_RULES, lc.copy_record(40, False))
    recs = lc.copy_chunk()
    have, R, cap = lc.fits(recs, lc.grep_geometry)
    assert R == 64 and all(have) and len(recs) == 256
    keep = [_decide(*lc.COPY_RULES, r) for r in recs]
    assert not any(keep[64:128]) and keep[128:192] == [False] * 63 + [True]
    assert keep[:6] == [True, False, True, True, False, True] and all(keep[192:206]) and not any(keep[206:])


def test_l2m_records():
    for what, v, kind in lc.l2m_value_records():
        assert kind in ("value", "stale", "deferred", "other")
    recs = lc.l2m_value_chunk()
    o = ob.L2M("gauge", lc.L2M_LABELS, value_field="duration")
    assert o.filter(b"".join(recs)) == ob.NOTOUCH
    series = {s["labels"][0] for s in o.snapshot()[2]}
    # the variants log_to_metrics has no number for make no series
    assert series == {w.encode() for w, v, kind in lc.l2m_value_records() if kind != "other"}
    assert all(lc.plain_event(r) for r in recs) and all(lc.plain_event(r) for r in lc.l2m_label_chunk())
    for n in lc.NAME_LENS:
        k, vk, recs = lc.l2m_name_chunk(n)
        assert len(k) == len(vk) == n and k != vk and k[1:] == vk[1:] and all(lc.plain_event(r) for r in recs)
        o = ob.L2M("gauge", [("label_field", k.decode()), ("label_field", "color")], value_field=vk.decode())
        assert o.filter(b"".join(recs)) == ob.NOTOUCH and len(o.snapshot()[2]) >= 4

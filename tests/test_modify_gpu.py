"""filter_modify on the device (csrc/modify_kernels.inc through flbgpu_filter_modify_create) against the CPU model
(tests/modify_model.py) and against the recorded answers of the real plugin (tests/golden/modify_ref_cases.json): output bytes,
return value, record counts and the overread counter"""
import base64
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import modify_chunks as mc
import modify_model as mm
import oracle_binding as ob
import synth

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "modify_runtime_cases.json")))["cases"]
REF_CASES = json.load(open(os.path.join(HERE, "golden", "modify_ref_cases.json")))["cases"]
APACHE2 = (r'^(?<host>[^ ]*) [^ ]* (?<user>[^ ]*) \[(?<time>[^\]]*)\] "(?<method>\S+)(?: +(?<path>[^ ]*) +\S*)?" '
           r'(?<code>[^ ]*) (?<size>[^ ]*)(?: "(?<referer>[^\"]*)" "(?<agent>.*)")?$')
TIME_FMT = "%d/%b/%Y:%H:%M:%S %z"
M1 = [("Condition", "Key_exists agent"), ("Rename", "host client"), ("Add", "cluster eu-1"), ("Remove", "user"),
      ("Copy", "code status"), ("Remove_wildcard", "ref")]
M2 = [("Condition", r"Key_value_matches code ^5\d\d$")] + M1[1:]


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def same(g, props, data):
    try:
        m = mm.Model(props)
    except ValueError:
        with pytest.raises(ValueError):
            g.FilterModify(props)
        return None
    f = g.FilterModify(props)
    got = f.filter(data)
    want = m.filter(data)
    assert got == want, (props, got[0], want[0])
    assert f.counts() == m.counts()
    assert f.overread() == m.stats.get("overread", 0)
    f.close()
    return got


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_runtime_cases(g, case):
    if case.get("refused"):
        with pytest.raises(ValueError):
            g.FilterModify([tuple(p) for p in case["props"]])
        return
    data = b"".join(synth.mp([[synth.ext_ts(0, 0), {}], json.loads(p)[1]]) for p in case["inputs"])
    same(g, [tuple(p) for p in case["props"]], data)


@pytest.mark.parametrize("case", REF_CASES, ids=[c["name"] for c in REF_CASES])
def test_fixture_cases(g, case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused"):
        with pytest.raises(ValueError):
            g.FilterModify(props)
        return
    data = base64.b64decode(case["in"])
    ret, out = same(g, props, data)
    # the real plugin's bytes directly, behind the reference processor's pass over a unit's buffer: the filter's output, or -- where
    # it answered NOTOUCH -- its input
    assert mm.processor_output(out if ret == g.MODIFIED else data) == base64.b64decode(case["out"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 1025])
def test_wave_edges(g, n):
    data = mc.wave_rows(n)
    for props in (mc.W_COND, mc.W_PLAIN):
        m = mm.Model(props)
        m.filter(data)
        assert same(g, props, data)[0] == g.MODIFIED
        # rows 0, 3, .. are rebuilt; 1, 4, .. have no "go" (the condition is false / Remove finds nothing, the other rules apply);
        # 2, 5, .. carry a time the encoder refuses
        rebuilt = sum(1 for i in range(n) if i % 3 == 0) if props is mc.W_COND else sum(1 for i in range(n) if i % 3 != 2)
        assert m.stats.get("rebuilt", 0) == rebuilt and m.counts() == (n, n)


# programs with g rules that can add an entry (Add, Set, Copy, Hard_copy): a body of 32 - g entries fills the last LDS slot.  In the
# first of each group every such rule applies (final lists of 31, 32 and 33 entries); in the others some do not (Add of a present
# key, Copy of an absent source) and the room is asked for all the same.  Move_to_start and Hard_copy shift entries across the list.
LIST_PROGRAMS = [
    (1, [("Add", "new1 v"), ("Move_to_start", "e1")]),
    (1, [("Hard_copy", "src new4"), ("Move_to_start", "e1")]),
    (1, [("Add", "src v"), ("Move_to_start", "e1"), ("Remove", "e4")]),
    (1, [("Copy", "absent new3"), ("Move_to_end", "s")]),
    (4, [("Add", "new1 v"), ("Set", "new2 v"), ("Copy", "src new3"), ("Hard_copy", "src new4"), ("Move_to_start", "e1")]),
    (4, [("Add", "src v"), ("Copy", "absent new3"), ("Hard_copy", "src e2"), ("Set", "e0 v"), ("Move_to_start", "e1")]),
    (4, [("Hard_copy", "e5 e0"), ("Move_to_end", "s"), ("Add", "n v"), ("Set", "src w"), ("Copy", "e3 e3b")]),
]


@pytest.mark.parametrize("grow,props", LIST_PROGRAMS, ids=["%d-%d" % (p[0], i) for i, p in enumerate(LIST_PROGRAMS)])
def test_lds_list_boundary(g, grow, props):
    assert sum(1 for name, _ in props if name in ("Add", "Set", "Copy", "Hard_copy")) == grow
    lim = 32 - grow
    data = mc.list_rows(130, [lim - 1, lim, lim + 1])
    assert same(g, props, data)[0] == g.MODIFIED
    if props is LIST_PROGRAMS[0][1] or props is LIST_PROGRAMS[4][1]:
        out = synth.unpack_all(same(g, props, data)[1])
        assert sorted({len(body[1]) for _, body in out if len(body[1]) > 4}) == [31, 32, 33]


@pytest.mark.parametrize("n", [1024, 1025])
def test_arena_exact_fit_and_regrow(g, n):
    # rows of 64 entries and a program that adds none: a row asks the arena for exactly its 64 entries.  1024 rows ask for the 65 536
    # entries a filter starts with and fit; 1025 rows make the arena grow
    props = [("Move_to_end", "k1"), ("Rename", "k7 seven"), ("Remove_regex", "^k5")]
    data = mc.rows_of_64(n)
    want = mm.Model(props).filter(data)
    assert want[0] == g.MODIFIED
    f = g.FilterModify(props)
    for _ in range(2):                                 # the second call sees the arena as the first one left it (trimmed if grown)
        assert f.filter(data) == want
        assert f.counts() == (n, n) and f.overread() == 0
    # growth and a decoder error in one call: NOTOUCH, and the counts are those of the rows in front of the error
    assert f.filter(mc.rows_of_64(1100, bad_at=700)) == (g.NOTOUCH, None)
    assert f.counts() == (700, 700)
    assert f.filter(data) == want
    f.close()


OVER = synth.mp([[synth.ext_ts(1, 2), {}], synth.KV([(b"x", b"y"), (b"ab", 1)])])          # "ab\x01z" runs past this record's end
GOOD = synth.mp([[synth.ext_ts(1, 3), {}], synth.KV([(b"abc", 1), (b"ab\x01zz", 2), (b"k", b"v")])])


@pytest.mark.parametrize("at", [0, 1, 63, 64, 65, 199])
def test_decoder_error_positions(g, at):
    props = [("Remove_wildcard", "ab\x01z"), ("Set", "k x")]
    bad = synth.mp([[synth.ext_ts(1, 0), {}], "not a map"])
    rows = [GOOD] * 200
    rows[at] = bad
    before, behind = (at - 1 if at else None), (at + 1 if at < 199 else None)
    for i in (before, behind):
        if i is not None:
            rows[i] = OVER
    data = b"".join(rows)
    f = g.FilterModify(props)
    assert f.filter(data) == (g.NOTOUCH, None)         # although every record in front of the error was rebuilt
    assert f.counts() == (at, at)
    assert f.overread() == (1 if before is not None else 0)
    f.close()
    assert same(g, props, data) == (g.NOTOUCH, None)
    # without the bad row the same rows are MODIFIED and both overreads count
    rows[at] = GOOD
    assert same(g, props, b"".join(rows))[0] == g.MODIFIED


def test_cut_last_record(g):
    case = [c for c in REF_CASES if c["name"] == "garbage_cut_record"][0]
    data = base64.b64decode(case["in"])
    got = same(g, [tuple(p) for p in case["props"]], data)
    # the golden holds the one whole record as it came in, although the rule applies to it: the plugin answered NOTOUCH
    assert got == (g.NOTOUCH, None) and base64.b64decode(case["out"]) == mm.processor_output(data) != b""
    # 70 whole records and one cut inside a payload: NOTOUCH; cut behind the payload's header, msgpack-c has consumed all it was
    # given, the decoder's offset stands at the end and the call is MODIFIED (the golden's garbage_cut_behind_header)
    whole, last = b"".join([GOOD] * 70), synth.mp([[synth.ext_ts(1, 4), {}], {"k": "long value"}])
    f = g.FilterModify([("Set", "k x")])
    assert f.filter(whole + last[:-4]) == (g.NOTOUCH, None) and f.counts() == (70, 70)
    f.close()
    assert same(g, [("Set", "k x")], whole + last[:-4]) == (g.NOTOUCH, None)
    assert same(g, [("Set", "k x")], whole + last[:-10])[0] == g.MODIFIED


@pytest.mark.parametrize("seed", mc.FUZZ_SEEDS)
def test_fuzz(g, seed):
    # (tests/test_modify_ref.py holds the generator to its floors on the model: rows rebuilt and raw, every rule, every condition)
    r = random.Random(seed)
    for _ in range(40):
        props = mc.rnd_program(r)
        f, m = g.FilterModify(props), mm.Model(props)
        for _ in range(3):
            data = b"".join(mc.rnd_record(r) for _ in range(r.randrange(1, 61)))
            got, want = f.filter(data), m.filter(data)
            assert got == want, (props, got[0], want[0])
            assert f.counts() == m.counts()
        assert f.overread() == m.stats.get("overread", 0) == 0
        f.close()


def test_rows_an_earlier_filter_dropped(g):
    n = 200
    drop = {0, 63, 64, n - 1}
    blob = b"".join(synth.mp([[synth.ext_ts(1700000000 + i, i), {}], synth.KV([(b"lvl", b"drop" if i in drop else b"keep"), (b"n%d" % (i % 5), i),
                                                                               (b"k", b"v")])]) for i in range(n))
    grep = [("exclude", "lvl ^drop$")]
    props = [("Condition", "Key_exists n1"), ("Set", "k x"), ("Move_to_start", "n"), ("Copy", "lvl level")]
    fg, fm = g.FilterGrep(grep), g.FilterModify(props)
    w1 = ob.Grep(grep).filter(blob)[1]
    assert len(synth.unpack_all(w1)) == n - 4
    chain = g.FilterChain([fg, fm])
    r, out = chain.filter(blob)
    m = mm.Model(props)
    assert (r, out) == m.filter(w1) and r == g.MODIFIED
    st = chain.last_stats()[1]
    assert (st["in_records"], st["out_records"]) == m.counts() == (n - 4, n - 4)
    assert fm.overread() == 0
    fm.close()


def test_prefix_quirk(g):
    # key "re" followed by the positive fixint 0x66 ('f'): "ref" matches through the value byte, before and after a re-pack
    rec = synth.mp([[synth.ext_ts(1, 2), {}], synth.KV([(b"re", 0x66), (b"x", b"y")])])
    assert same(g, [("Remove_wildcard", "ref")], rec)[0] == g.MODIFIED
    assert same(g, [("Set", "q w"), ("Remove_wildcard", "ref")], rec)[0] == g.MODIFIED
    assert same(g, [("Set", "q w"), ("Move_to_end", "ref")], rec)[0] == g.MODIFIED
    # a compare that runs past the record: no match, and the record is counted
    tail = synth.mp([[synth.ext_ts(1, 2), {}], synth.KV([(b"x", b"y"), (b"ab", 1)])])
    f = g.FilterModify([("Remove_wildcard", "ab\x01z")])
    assert f.filter(tail * 3) == (g.NOTOUCH, None)
    assert f.overread() == 3
    f.close()
    assert same(g, [("Remove_wildcard", "ab\x01z")], tail)[0] == g.NOTOUCH


def test_call_level(g):
    rec = [synth.mp([[synth.ext_ts(1, i), {}], {"k": "v%d" % i, "n": i}]) for i in range(10)]
    # nothing modified: NOTOUCH
    assert same(g, [("Remove", "absent")], b"".join(rec))[0] == g.NOTOUCH
    assert same(g, [("Condition", "Key_exists absent"), ("Set", "k x")], b"".join(rec))[0] == g.NOTOUCH
    # a malformed record in the middle: NOTOUCH although records were modified
    bad = synth.mp([[synth.ext_ts(1, 0), {}], "not a map"])
    assert same(g, [("Set", "k x")], b"".join(rec[:5]) + bad + b"".join(rec[5:]))[0] == g.NOTOUCH
    # a raw device chunk (no offsets): the records are found on the device
    data = b"".join(rec)
    L = g.lib()
    d = L.flbgpu_dev_alloc(len(data) + 16)
    L.flbgpu_memcpy_h2d(d, data, len(data))
    f = g.FilterModify([("Set", "k x"), ("Move_to_end", "k")])
    ret, out = f.filter_dev(g.DevChunk(d, None, 0, len(data)))
    want = mm.Model([("Set", "k x"), ("Move_to_end", "k")]).filter(data)
    import ctypes
    buf = ctypes.create_string_buffer(out.bytes)
    L.flbgpu_memcpy_d2h(buf, out.data, out.bytes)
    assert (ret, buf.raw) == want
    assert f.counts() == (10, 10)
    f.close()
    L.flbgpu_dev_free(d)


def test_large_rows_and_wide_maps(g):
    r = random.Random(7)
    recs = []
    for i in range(40):
        n = r.choice([5, 31, 33, 300, 700])
        body = synth.KV([(b"k%d" % (j % 97), b"v" * r.randrange(3)) for j in range(n)] + [(b"log", b"L" * r.choice([10, 5000, 70000]))])
        recs.append(synth.mp([[synth.ext_ts(3, i), {}], body]))
    data = b"".join(recs)
    for props in ([("Set", "k1 x"), ("Copy", "log log2"), ("Remove_wildcard", "k2")],
                  [("Move_to_start", "k5"), ("Hard_rename", "k3 k4"), ("Add", "new 1")],
                  [("Condition", "Matching_keys_have_matching_values ^k v*"), ("Remove_regex", "^k[0-9]$")]):
        assert same(g, props, data)[0] == g.MODIFIED


def test_arena_grows_past_its_first_size(g):
    # 3 000 records of 60 keys: 180 000 entries in the HBM arena, more than the 65 536 a filter starts with -- the size pass runs
    # again on a grown arena, and the grown arena is handed back at the end of the call
    recs = [synth.mp([[synth.ext_ts(4, i), {}], {("k%d" % j): j for j in range(60)}]) for i in range(3000)]
    props = [("Move_to_end", "k1"), ("Copy", "k7 seven"), ("Remove_regex", "^k5")]
    data = b"".join(recs)
    assert same(g, props, data)[0] == g.MODIFIED
    assert same(g, props, data)[0] == g.MODIFIED


def test_chain_parser_grep_modify(g):
    data, off, ep = synth.apache_records(3000)
    blob = bytes(data)
    p = g.Parser(APACHE2, time_fmt=TIME_FMT, time_key="time")
    fp, fg = g.FilterParser("log", [p]), g.FilterGrep([("regex", r"code ^[25]\d\d$")])
    fm = g.FilterModify(M1)
    r, out = g.FilterChain([fp, fg, fm]).filter(blob)
    po = ob.Parser(APACHE2, time_fmt=TIME_FMT, time_key="time")
    _, w1 = ob.FilterParser("log", [po]).filter(blob)
    _, w2 = ob.Grep([("regex", r"code ^[25]\d\d$")]).filter(w1)
    assert (r, out) == mm.Model(M1).filter(w2)
    r2, out2 = fm.filter(w2)
    assert (r2, out2) == (r, out)


def test_ten_million_records(g):
    r = random.Random(3)
    block = b"".join(synth.mp([[synth.ext_ts(1700000000 + i, i), {}],
                               {"host": "h%d" % i, "user": "-", "code": r.choice(["200", "404", "500", "503"]), "agent": "a"}])
                     for i in range(100))
    for props in (M1, M2):
        want = mm.Model(props).filter(block)
        f = g.FilterModify(props)
        ret, out = f.filter(block * 100000)
        assert ret == want[0] == g.MODIFIED
        assert out == want[1] * 100000
        assert f.counts() == (10000000, 10000000)
        f.close()

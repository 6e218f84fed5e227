"""filter_modify on the device (csrc/modify_kernels.inc through flbgpu_filter_modify_create) against the CPU model
(tests/modify_model.py): output bytes, return value and record counts"""
import json
import os
import random
import struct
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import modify_model as mm
import oracle_binding as ob
import synth

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "modify_runtime_cases.json")))["cases"]
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


KEYS = [b"a", b"ab", b"abc", b"abcd", b"k", b"k1", b"k2", b"log", b"re", b"ref", b"referer", b"x", b"", b"true", b"A3"]


def rnd_val(r, depth=0):
    c = r.randrange(12 if depth < 2 else 9)
    if c == 0:
        return r.choice([b"", b"sample", b"abc", b"500", b"200", b"true", "café".encode(), b"x" * r.randrange(40)])
    if c == 1:
        return synth.Raw(b"\xc4" + bytes([3]) + b"abc")
    if c == 2:
        return r.choice([0, 1, 127, 128, 255, 256, 65535, 65536, 2 ** 32, 2 ** 63])
    if c == 3:
        return r.choice([-1, -32, -33, -128, -129, -32768, -32769, -2 ** 31, -2 ** 31 - 1])
    if c == 4:
        return synth.Raw(b"\xd0\x05")                 # a non-negative value in the signed family
    if c == 5:
        return synth.Raw(b"\xca" + struct.pack(">f", 1.5))
    if c == 6:
        return r.random() * 1000
    if c == 7:
        return r.choice([True, False])
    if c == 8:
        return None
    if c == 9:
        return [rnd_val(r, depth + 1) for _ in range(r.randrange(4))]
    if c == 10:
        return {r.choice(KEYS): rnd_val(r, depth + 1) for _ in range(r.randrange(4))}
    return synth.KV([(r.choice(KEYS), rnd_val(r, depth + 1)) for _ in range(r.randrange(4))])


def rnd_record(r):
    body = synth.KV([(r.choice(KEYS) if r.random() < 0.9 else r.choice([True, 7]), rnd_val(r)) for _ in range(r.randrange(8))])
    kind = r.randrange(8)
    if kind == 0:
        return synth.mp([r.randrange(2 ** 33), body])                          # legacy, integer time
    if kind == 1:
        return synth.mp([1700000000.25, body])                                 # legacy, float time
    if kind == 2:
        return synth.mp([[synth.ext_ts(5, 6), {"m": 1, "z": [1, 2]}], body])    # metadata
    if kind == 3 and r.random() < 0.3:
        return synth.mp([[synth.Raw(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), {}], {}])   # group marker
    return synth.mp([[synth.ext_ts(r.randrange(2 ** 32), r.randrange(10 ** 9)), {}], body])


def rnd_word(r):
    return r.choice([k.decode() or "''" for k in KEYS] + ["^a", "b$", "^k[0-9]$", "/^A/i", "x|y"])


def rnd_program(r):
    props = []
    for _ in range(r.randrange(5)):
        t = r.choice(mm.CONDS)
        if mm.a_rx(mm.CONDS.index(t)):
            props.append(("Condition", "%s %s %s" % (t, r.choice(["^a", "^k", "^re", "true", "."]), r.choice(["^s", "0", "t", "."]))))
        else:
            props.append(("Condition", "%s %s %s" % (t, r.choice(["a", "$a", "k1", "$a['k'][0]", "$a['ab']", "$TAG", "log"]),
                                                    r.choice(["sample", "^s", "abc", "''"]))))
    for _ in range(r.randrange(1, 17)):
        name = r.choice(list(mm.RULES1) + list(mm.RULES2))
        if name in mm.RULES1:
            w = rnd_word(r) if name == "remove_regex" else r.choice([k.decode() for k in KEYS if k] + ["r", "refe", "abx"])
            props.append((name, w))
        else:
            a, b = r.choice([k.decode() for k in KEYS if k]), r.choice([k.decode() for k in KEYS if k])
            if name == "hard_copy" and a == b:
                b = b + "_2"
            props.append((name, "%s %s" % (a, b)))
    r.shuffle(props)
    return props


def test_fuzz(g):
    r = random.Random(1234)
    modified = 0
    for it in range(150):
        props = rnd_program(r)
        data = b"".join(rnd_record(r) for _ in range(r.randrange(1, 60)))
        got = same(g, props, data)
        modified += got is not None and got[0] == g.MODIFIED
    assert modified > 30


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

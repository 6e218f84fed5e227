"""filter_record_modifier on the device (csrc/recmod_kernels.inc through flbgpu_filter_record_modifier_create) against the CPU model
(tests/recmod_model.py) and against the recorded answers of the real plugin (tests/golden/recmod_ref_cases.json): output bytes,
return value and record counts"""
import base64
import ctypes
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
import recmod_model as rm
import synth

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "recmod_ref_cases.json")))["cases"]
APACHE2 = (r'^(?<host>[^ ]*) [^ ]* (?<user>[^ ]*) \[(?<time>[^\]]*)\] "(?<method>\S+)(?: +(?<path>[^ ]*) +\S*)?" '
           r'(?<code>[^ ]*) (?<size>[^ ]*)(?: "(?<referer>[^\"]*)" "(?<agent>.*)")?$')
TIME_FMT = "%d/%b/%Y:%H:%M:%S %z"
R1 = [("Record", "hostname h"), ("Remove_key", "agent")]
R2 = [("Allowlist_key", "host"), ("Allowlist_key", "code"), ("Allowlist_key", "size")]


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def same(g, f, m, data):
    got = f.filter(data)
    want = m.filter(data)
    assert got == want, (got[0], want[0])
    assert f.counts() == m.counts()
    return got


def same_props(g, props, data):
    f = g.FilterRecordModifier(props)
    try:
        return same(g, f, rm.Model(props), data)
    finally:
        f.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused") or case.get("refused_here"):
        with pytest.raises(ValueError):
            g.FilterRecordModifier(props)
        return
    data = base64.b64decode(case["in"])
    got = same_props(g, props, data)
    # the real plugin's bytes directly
    assert got == (case["ret"], base64.b64decode(case["out"]) if case["out"] is not None else None)


def mixed_records(n):
    """every third record holds `agent` and loses it, the others go through the walk and keep all they have"""
    return b"".join(synth.mp([[synth.ext_ts(1700000000 + i, i), {}],
                              synth.KV([(b"host", b"h%d" % (i % 9))] + ([(b"agent", b"a" * (i % 23))] if i % 3 == 0 else []) + [(b"size", 1000 + i)])])
                    for i in range(n))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_block_edges(g, n):
    data = mixed_records(n)
    assert data.count(b"\xa5agent") == (n + 2) // 3
    for props in (R1, [("Remove_key", "agent")]):
        ret, out = same_props(g, props, data)
        assert ret == g.MODIFIED and len(synth.unpack_all(out)) == n
        assert out.count(b"\xa5agent") == 0 and out.count(b"\xa8hostname") == (n if props is R1 else 0)


KEYS = [b"a", b"A", b"ab", b"AB", b"aB", b"abc", b"ABCD", b"abcde", b"host", b"Host", b"HOSTNAME", b"k", b"k1", b"K2", b"log", b"",
        b"x" * 9, b"X" * 9, b"x" * 40, "é".encode(), "É".encode(), b"a\0b", b"ab\0"]
TABLE = ["a", "A", "ab", "Ab*", "abc", "abcd*", "host", "HOST*", "k*", "K1", "log", "*", "x" * 9, "X" * 8 + "*", "x" * 40, "é", "É*",
         "zz", "nothing*", "abcdefgh", "ABCDEFGH*"]


def random_hdr(b, *forms):
    h, n = forms[len(b) % len(forms)]
    return h + len(b).to_bytes(n, "big") + b


def rnd_key(r):
    c = r.random()
    k = r.choice(KEYS)
    if c < 0.55:
        return k
    if c < 0.7:
        return synth.Raw(random_hdr(k, (b"\xd9", 1), (b"\xda", 2), (b"\xdb", 4)))        # a STR key in a wider header
    if c < 0.85:
        return synth.Raw(random_hdr(k, (b"\xc4", 1), (b"\xc5", 2), (b"\xc6", 4)))        # a BIN key
    if c < 0.93:
        return r.choice([0, 7, 300, -1, 2 ** 40, True, None, 1.5])
    return r.choice([[1, b"a"], {b"a": 1}, synth.Raw(b"\xdc\x00\x01\xa1a")])             # a nested key


def rnd_val(r, depth=0):
    c = r.randrange(13 if depth < 2 else 10)
    if c == 0:
        return r.choice([b"", b"sample", b"abc", "café".encode(), b"x" * r.randrange(70), b"y" * 300])
    if c == 1:
        return synth.Raw(b"\xc4\x03abc")
    if c == 2:
        return r.choice([0, 1, 127, 128, 255, 256, 65535, 65536, 2 ** 32, 2 ** 63])
    if c == 3:
        return r.choice([-1, -32, -33, -128, -129, -32768, -32769, -2 ** 31, -2 ** 31 - 1])
    if c == 4:
        return synth.Raw(r.choice([b"\xd0\x05", b"\xd1\x01\x00", b"\xd2\x00\x01\x00\x00", b"\xd3" + bytes(7) + b"\x09", b"\xcd\x00\x07",
                                   b"\xce\x00\x00\x01\x00", b"\xcf" + bytes(7) + b"\x01", b"\xd1\xff\xff", b"\xd3" + b"\xff" * 8]))
    if c == 5:
        return synth.Raw(b"\xca" + struct.pack(">f", 1.5))
    if c == 6:
        return r.random() * 1000
    if c == 7:
        return r.choice([True, False, None])
    if c == 8:
        return synth.Raw(r.choice([b"\xda\x00\x03abc", b"\xdb\x00\x00\x00\x01z", b"\xc5\x00\x02hi", b"\xc7\x03\x05abc", b"\xd5\x01ab",
                                   b"\xc8\x00\x04\x02abcd", b"\xc9\x00\x00\x00\x02\x07ab"]))
    if c == 9:
        return synth.Raw(r.choice([b"\xdc\x00\x02\x01\x02", b"\xdd\x00\x00\x00\x01\xa1q", b"\xde\x00\x01\xa1q\x01", b"\xdf\x00\x00\x00\x00"]))
    if c == 10:
        return [rnd_val(r, depth + 1) for _ in range(r.randrange(4))]
    if c == 11:
        return {r.choice(KEYS): rnd_val(r, depth + 1) for _ in range(r.randrange(4))}
    return synth.KV([(rnd_key(r), rnd_val(r, depth + 1)) for _ in range(r.randrange(4))])


def rnd_body(r):
    items = [(rnd_key(r), rnd_val(r)) for _ in range(r.choice([0, 1, 2, 3, 5, 8, 15, 16, 17, 40]))]
    b = synth.mp(synth.KV(items))
    if r.random() < 0.2 and len(items) < 16:
        b = b"\xde" + struct.pack(">H", len(items)) + b[1:]                              # map16 where a fixmap would do
    elif r.random() < 0.1:
        b = b"\xdf" + struct.pack(">I", len(items)) + (b[1:] if len(items) < 16 else b[3:])
    return synth.Raw(b)


def rnd_record(r):
    body = rnd_body(r)
    kind = r.randrange(10)
    if kind == 0:
        return synth.mp([r.choice([0, 5, 1700000000, 2 ** 32 - 1, 2 ** 32, 2 ** 40]), body])      # legacy, integer time
    if kind == 1:
        return synth.mp([1700000000.25, body])                                                  # legacy, float time
    if kind == 2:
        return synth.mp([[synth.ext_ts(5, 6), synth.KV([(b"m", 1), (b"z", [1, synth.Raw(b"\xd0\x05")])])], body])
    if kind == 3:
        return synth.mp([[synth.ext_ts(5, 6), synth.Raw(b"\xde\x00\x01\xd9\x01m\xcd\x00\x01")], body])
    if kind == 4 and r.random() < 0.3:
        return synth.mp([[synth.Raw(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), {}], {}])      # group marker
    if kind == 5 and r.random() < 0.3:
        return synth.mp([synth.Raw(b"\xd7\x00" + struct.pack(">II", 9, 10)), body])              # legacy, EventTime
    return synth.mp([[synth.ext_ts(r.randrange(2 ** 32 - 2), r.randrange(10 ** 9)), {}], body])


def rnd_program(r):
    props = []
    c = r.random()
    if c < 0.45:
        props += [("Remove_key", x) for x in r.sample(TABLE, r.randrange(1, 7))]
    elif c < 0.9:
        props += [(r.choice(["Allowlist_key", "Whitelist_key"]), x) for x in r.sample(TABLE, r.randrange(1, 7))]
    for _ in range(r.choice([0, 0, 1, 2, 5])):
        props.append(("Record", r.choice(["h v", "hostname node-1", 'k "v w"', "a b c", "long " + "v" * 300, '"" e', "x" * 40 + " y"])))
    r.shuffle(props)
    return props


def rnd_chunk(r):
    recs = [rnd_record(r) for _ in range(r.randrange(1, 40))]
    c = r.random()
    if c < 0.08:                                     # a decoder error inside the chunk
        bad = r.choice([synth.mp([[synth.ext_ts(1), {}], "text"]), synth.mp([[synth.ext_ts(1, 10 ** 9), {}], {}]), synth.mp(5),
                        synth.mp([[synth.ext_ts(1), [1]], {}]), synth.mp(["time", {}]), synth.mp([1, {}, 3])])
        recs.insert(r.randrange(len(recs) + 1), bad)
    data = b"".join(recs)
    if 0.08 <= c < 0.14:                             # garbage / a cut record behind the rows
        data += r.choice([b"\xc1", b"\xc1\x00\x01", recs[0][:-1], b"\x92\x92\xd7", b"\xda\x00"])
    return data


def test_fuzz(g):
    r = random.Random(20261)
    chunks = modified = notouch = 0
    for _ in range(110):
        props = rnd_program(r)
        f, m = g.FilterRecordModifier(props), rm.Model(props)
        for _ in range(20):
            got = same(g, f, m, rnd_chunk(r))
            chunks += 1
            modified += got[0] == g.MODIFIED
            notouch += got[0] == g.NOTOUCH
        f.close()
    assert chunks >= 2000 and modified > 500 and notouch > 20


def wide_body(n, pad=b""):
    items = b"".join(synth.mp(b"k%d" % j) + synth.mp(b"v%d" % (j % 7) + pad) for j in range(n))
    return synth.Raw((b"\xde" + struct.pack(">H", n) if n < 65536 else b"\xdf" + struct.pack(">I", n)) + items)


def test_wide_maps(g):
    recs = [synth.mp([[synth.ext_ts(3, i), {}], wide_body(n)]) for i, n in enumerate([70, 300, 5, 65535, 64, 65, 300])]
    data = b"".join(recs)
    for props in ([("Remove_key", "k1*"), ("Record", "a b")], [("Allowlist_key", "k2*"), ("Allowlist_key", "K69")], [("Remove_key", "K299")]):
        assert same_props(g, props, data)[0] == g.MODIFIED
    assert same_props(g, [("Allowlist_key", "nothing")], data) == (g.NOTOUCH, None)
    # 70 000 entries: the reference gives up on the whole call with -1 -- unless a decoder error ends the loop in front of the record
    big = synth.mp([[synth.ext_ts(4, 0), {}], wide_body(70000)])
    for props in ([("Remove_key", "k1*")], [("Record", "a b")]):
        assert same_props(g, props, recs[0] + big + recs[1]) == (-1, None)
        assert same_props(g, props, big) == (-1, None)
        got = same_props(g, props, recs[0] + synth.mp(5) + big)
        assert got[0] == g.MODIFIED


def test_three_megabyte_record(g):
    big = b"L" * (3 << 20)
    recs = [synth.mp([[synth.ext_ts(1, 1), {}], synth.KV([(b"a", 1), (b"log", big), (b"z", b"tail")])]),
            synth.mp([[synth.ext_ts(1, 2), {}], synth.KV([(b"log", synth.Raw(b"\xc6" + struct.pack(">I", len(big)) + big)), (b"a", 2)])]),
            synth.mp([[synth.ext_ts(1, 3), {}], synth.KV([(b"a", 3)])])]
    data = b"".join(recs)
    assert same_props(g, [("Remove_key", "a")], data)[0] == g.MODIFIED
    assert same_props(g, [("Remove_key", "LOG"), ("Record", "k v")], data)[0] == g.MODIFIED
    assert same_props(g, [("Allowlist_key", "lo*")], data)[0] == g.MODIFIED


def test_call_level(g):
    rec = [synth.mp([[synth.ext_ts(1, i), {}], {"k": "v%d" % i, "n": i}]) for i in range(10)]
    data = b"".join(rec)
    # nothing listed occurs, no Record: NOTOUCH
    assert same_props(g, [("Remove_key", "absent")], data) == (g.NOTOUCH, None)
    assert same_props(g, [], data) == (g.NOTOUCH, None)
    # every record loses every key: nothing in the encoder, NOTOUCH
    assert same_props(g, [("Remove_key", "*")], data) == (g.NOTOUCH, None)
    # a decoder error in the middle: MODIFIED with the records in front of it
    bad = synth.mp([[synth.ext_ts(1, 0), {}], "not a map"])
    got = same_props(g, [("Remove_key", "n")], b"".join(rec[:5]) + bad + b"".join(rec[5:]))
    assert got[0] == g.MODIFIED and len(synth.unpack_all(got[1])) == 5
    assert same_props(g, [("Remove_key", "n")], bad + data) == (g.NOTOUCH, None)


def test_raw_device_chunk_and_host_buffer(g):
    rec = [synth.mp([[synth.ext_ts(1, i), {}], {"k": "v%d" % i, "Agent": "x", "n": i}]) for i in range(1000)]
    data = b"".join(rec)
    want = rm.Model(R1).filter(data)
    assert want[0] == g.MODIFIED
    L = g.lib()
    d = L.flbgpu_dev_alloc(len(data) + 16)
    L.flbgpu_memcpy_h2d(d, data, len(data))
    f = g.FilterRecordModifier(R1)
    ret, out = f.filter_dev(g.DevChunk(d, None, 0, len(data)))          # no offsets: the records are found on the device
    buf = ctypes.create_string_buffer(out.bytes)
    L.flbgpu_memcpy_d2h(buf, out.data, out.bytes)
    assert (ret, buf.raw) == want
    assert f.counts() == (1000, 1000)
    assert f.filter(data) == want                                        # flbgpu_filter_run on the host buffer
    assert f.counts() == (1000, 1000)
    f.close()
    L.flbgpu_dev_free(d)


def test_chains(g):
    data, off, ep = synth.apache_records(3000)
    blob = bytes(data)
    p = g.Parser(APACHE2, time_fmt=TIME_FMT, time_key="time")
    fp, fg = g.FilterParser("log", [p]), g.FilterGrep([("regex", r"code ^[25]\d\d$")])
    po = ob.Parser(APACHE2, time_fmt=TIME_FMT, time_key="time")
    _, w1 = ob.FilterParser("log", [po]).filter(blob)
    _, w2 = ob.Grep([("regex", r"code ^[25]\d\d$")]).filter(w1)
    for props in (R1, R2):
        fr = g.FilterRecordModifier(props)
        chain = g.FilterChain([fp, fg, fr])
        r, out = chain.filter(blob)
        m = rm.Model(props)
        assert (r, out) == m.filter(w2)
        st = chain.last_stats()[2]
        assert (st["in_records"], st["out_records"]) == m.counts()
        assert fr.filter(w2) == (r, out)
        fr.close()
    # modify -> record_modifier
    M = [("Remove", "agent"), ("Add", "hostname h"), ("Rename", "host Client")]
    RM = [("Remove_key", "client"), ("Record", "cluster eu-1")]
    fm, fr = g.FilterModify(M), g.FilterRecordModifier(RM)
    r, out = g.FilterChain([fm, fr]).filter(w2)
    _, x1 = mm.Model(M).filter(w2)
    assert (r, out) == rm.Model(RM).filter(x1)


def test_ten_million_records(g):
    r = random.Random(3)
    block = b"".join(synth.mp([[synth.ext_ts(1700000000 + i, i), {}],
                               {"host": "h%d" % i, "user": "-", "code": r.choice(["200", "404", "500", "503"]), "size": "%d" % (i * 37),
                                "agent": "a" * (i % 5)}])
                     for i in range(100))
    for props in (R1, R2):
        want = rm.Model(props).filter(block)
        f = g.FilterRecordModifier(props)
        ret, out = f.filter(block * 100000)
        assert ret == want[0] == g.MODIFIED
        assert f.counts() == (10000000, 10000000)
        assert len(out) == len(want[1]) * 100000
        # a seeded sample of blocks, then everything
        for b in random.Random(11).sample(range(100000), 50):
            assert out[b * len(want[1]):(b + 1) * len(want[1])] == want[1]
        assert out == want[1] * 100000
        f.close()

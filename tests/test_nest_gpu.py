"""filter_nest on the device (csrc/nest_kernels.inc through flbgpu_filter_nest_create) against the CPU model (tests/nest_model.py) and
against the recorded answers of the real plugin (tests/golden/nest_ref_cases.json): output bytes, return value, record counts and the
filter's own counters"""
import base64
import ctypes
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import nest_model as nm
from nest_chunks import L1, N1, mixed_records, rec, rnd_program, rnd_record, wide_body
import oracle_binding as ob
import synth

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "nest_ref_cases.json")))["cases"]


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
    assert f.counters() == m.counters()
    return got


def same_props(g, props, data):
    f, m = g.FilterNest(props), nm.Model(props)
    try:
        return same(g, f, m, data), m
    finally:
        f.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused"):
        with pytest.raises(ValueError):
            g.FilterNest(props)
        return
    data = base64.b64decode(case["in"])
    (ret, out), m = same_props(g, props, data)
    if case.get("undefined"):
        assert (ret, out) == (g.MODIFIED, data)
        return
    # the real plugin's bytes directly (the recorded answers are bytes only; every recorded call emitted something)
    assert (ret, out) == (g.MODIFIED, base64.b64decode(case["out"]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_block_edges(g, n):
    data = mixed_records(n)
    for props in (N1, L1):
        (ret, out), m = same_props(g, props, data)
        assert ret == g.MODIFIED and m.counts() == (n, n)
        assert m.counters()[0] == sum(1 for i in range(n) if (i % 3 == 1 if props is N1 else i % 3)) and len(synth.unpack_all(out)) == n


@pytest.mark.parametrize("op,seed", [(nm.NEST, 20261), (nm.NEST, 20262), (nm.LIFT, 20263), (nm.LIFT, 20264)])
def test_fuzz(g, op, seed):
    r = random.Random(seed)
    rows = {"raw": 0, "built": 0, "lost": 0}
    for _ in range(30):
        props, key, prefixed = rnd_program(r, op)
        f, m = g.FilterNest(props), nm.Model(props)
        for _ in range(4):
            same(g, f, m, b"".join(rnd_record(r, op, key, prefixed) for _ in range(r.randrange(1, 50))))
            for k in m.rows:
                rows[k] += 1
        assert f.counters()[1:] == (0, 0, 0)
        f.close()
    total = sum(rows.values())
    assert total >= 2000 and rows["built"] * 4 >= total and rows["raw"] * 4 >= total, rows


def test_counted_not_matched(g):
    # Remove_prefix matches a key shorter than the prefix through the bytes behind it: undefined, the record goes out raw
    a98 = rec(synth.KV([(b"a", 98), (b"z", 1)]))
    (ret, out), m = same_props(g, [("Operation", "nest"), ("Nest_under", "n"), ("Wildcard", "*"), ("Remove_prefix", "ab")], a98)
    assert (ret, out) == (g.MODIFIED, a98) and m.counters() == (0, 0, 1, 0)
    # a prefix and a lifted map with a key that is neither STR nor BIN
    int_key = rec(synth.KV([(b"m", synth.KV([(b"s", 1), (5, b"five")]))]))
    five = int_key + rec(synth.KV([(b"m", {b"s": 1})]))
    for pfx in ("Add_prefix", "Remove_prefix"):
        (ret, out), m = same_props(g, [("Operation", "lift"), ("Nested_under", "m"), (pfx, "p_")], five)
        assert ret == g.MODIFIED and out.startswith(int_key) and len(out) > len(five) and m.counters() == (1, 0, 1, 0)
    # without a prefix the same map lifts
    (ret, out), m = same_props(g, [("Operation", "lift"), ("Nested_under", "m")], five)
    assert m.counters() == (2, 0, 0, 0)
    # compares that would need bytes past the record's end: counted, "no match"
    last = rec(synth.KV([(b"z", 1), (b"a", 98)]))                      # 'a', 'b' and the record ends: "abc*" runs out
    (ret, out), m = same_props(g, [("Operation", "nest"), ("Nest_under", "n"), ("Wildcard", "abc*"), ("Wildcard", "abX*")], last + last)
    assert (ret, out) == (g.MODIFIED, last + last) and m.counters() == (0, 4, 0, 0)       # two compares a record
    (ret, out), m = same_props(g, [("Operation", "nest"), ("Nest_under", "n"), ("Wildcard", "*"), ("Remove_prefix", "abc")], last)
    assert ret == g.MODIFIED and m.counters() == (1, 1, 0, 0)
    inner = rec(synth.KV([(b"m", synth.KV([(b"q", 1), (b"a", 98)]))]))
    (ret, out), m = same_props(g, [("Operation", "lift"), ("Nested_under", "m"), ("Remove_prefix", "abc")], inner)
    assert ret == g.MODIFIED and m.counters() == (1, 1, 0, 0)


_wide = []


def wide70k():
    if not _wide:
        _wide.append(wide_body(70000))
    return _wide[0]


SMALL = rec({"a": 1}, 2)
NEST_N = [("Operation", "nest"), ("Nest_under", "n")]
LIFT_M = [("Operation", "lift"), ("Nested_under", "m")]


def test_wide_map_with_one_matching_key(g):
    (ret, out), m = same_props(g, NEST_N + [("Wildcard", "k69999")], rec(wide70k(), 3) + SMALL)
    assert ret == g.MODIFIED and m.counters()[0] == 1


@pytest.mark.parametrize("prefix", [[], [("Add_prefix", "p_")], [("Remove_prefix", "k6")]], ids=["plain", "add", "remove"])
def test_lifted_map_of_70000_entries(g, prefix):
    data = SMALL + rec(synth.KV([(b"a", 1), (b"m", wide70k()), (b"z", 2)]), 4)
    (ret, out), m = same_props(g, LIFT_M + prefix, data)
    assert ret == g.MODIFIED and m.counters()[0] == 1


def test_nested_output_crosses_64k(g):
    data = rec(synth.KV([(b"k%d" % j, b"v" * 700) for j in range(100)] + [(b"other", 1)]), 5)
    (ret, out), m = same_props(g, NEST_N + [("Wildcard", "k*"), ("Add_prefix", "p_")], data)
    assert ret == g.MODIFIED and len(out) > 70000 and m.counters()[0] == 1


def test_call_level(g):
    recs = [rec({"k": "v%d" % i, "m": {"n": i}}, 1, i) for i in range(10)]
    data = b"".join(recs)
    lift = [("Operation", "lift"), ("Nested_under", "m")]
    # nothing matches: MODIFIED with the chunk's own bytes
    (ret, out), m = same_props(g, [("Operation", "lift"), ("Nested_under", "absent")], data)
    assert (ret, out) == (g.MODIFIED, data) and m.counts() == (10, 10) and m.counters()[0] == 0
    # a decoder error in the middle: the records in front of it come out, the counts cover only those
    bad = synth.mp([[synth.ext_ts(1, 0), {}], "not a map"])
    (ret, out), m = same_props(g, lift, b"".join(recs[:5]) + bad + b"".join(recs[5:]))
    assert ret == g.MODIFIED and len(synth.unpack_all(out)) == 5 and m.counts() == (5, 5) and m.counters()[0] == 5
    (ret, out), m = same_props(g, lift, bad + data)
    assert (ret, out) == (g.NOTOUCH, None) and m.counts() == (0, 0)
    # every record is lost (nest without a key): nothing in the encoder, NOTOUCH
    (ret, out), m = same_props(g, [("Operation", "nest"), ("Wildcard", "k")], data)
    assert (ret, out) == (g.NOTOUCH, None) and m.counts() == (10, 10)
    # the counters add up over the calls of one filter
    f, m = g.FilterNest(lift), nm.Model(lift)
    same(g, f, m, data)
    same(g, f, m, data)
    assert f.counters() == (20, 0, 0, 0)
    f.close()


def test_raw_device_chunk_and_host_buffer(g):
    data = mixed_records(1000)
    want = nm.Model(L1).filter(data)
    assert want[0] == g.MODIFIED
    L = g.lib()
    d = L.flbgpu_dev_alloc(len(data) + 16)
    L.flbgpu_memcpy_h2d(d, data, len(data))
    f = g.FilterNest(L1)
    ret, out = f.filter_dev(g.DevChunk(d, None, 0, len(data)))          # no offsets: the records are found on the device
    buf = ctypes.create_string_buffer(out.bytes)
    L.flbgpu_memcpy_d2h(buf, out.data, out.bytes)
    assert (ret, buf.raw) == want
    assert f.counts() == (1000, 1000)
    assert f.filter(data) == want                                        # flbgpu_filter_run on the host buffer
    f.close()
    L.flbgpu_dev_free(d)


def test_chain_parser_grep_lift(g):
    lines = [b'{"level":"%s","msg":"m%d","kubernetes":{"pod":"p%d","ns":"d","labels":{"app":"a"}}}' % ([b"info", b"error"][i % 2], i, i)
             for i in range(500)]
    lines[7] = b'{"level":"error","msg":"no map","kubernetes":"text"}'
    lines[9] = b'{"level":"error","msg":"nothing"}'
    blob = b"".join(rec({"log": ln}, 1700000000 + i, i) for i, ln in enumerate(lines))
    grep = [("regex", "level ^error$")]
    fp, fg, fn = g.FilterParser("log", [g.Parser(format="json")]), g.FilterGrep(grep), g.FilterNest(L1)
    r2, w2 = g.FilterChain([fp, fg]).filter(blob)
    assert r2 == g.MODIFIED and len(synth.unpack_all(w2)) == 250
    _, o1 = ob.FilterParser("log", [ob.Parser(format="json")]).filter(blob)
    assert w2 == ob.Grep(grep).filter(o1)[1]
    chain = g.FilterChain([fp, fg, fn])
    r, out = chain.filter(blob)
    m = nm.Model(L1)
    assert (r, out) == m.filter(w2) and m.counters()[0] == 248
    st = chain.last_stats()[2]
    assert (st["in_records"], st["out_records"]) == m.counts() == (250, 250)
    fn.close()

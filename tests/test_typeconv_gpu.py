"""filter_type_converter on the device (csrc/typeconv_kernels.inc through flbgpu_filter_type_converter_create) against the CPU model
(tests/typeconv_model.py) and against the recorded answers of the real plugin (tests/golden/typeconv_ref_cases.json): output bytes,
return value, record counts and the filter's own counters.  Every comparison includes the size/emit mismatch counter, which the
model holds at 0."""
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
import typeconv_model as tm
from typeconv_chunks import P4, P64, mixed_records, number_then_garbage, rec, rnd_program, rnd_record
import oracle_binding as ob
import synth

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "typeconv_ref_cases.json")))["cases"]


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
    assert f.counters() == m.counters() and f.counters()[3] == 0
    return got


def same_props(g, props, data):
    f, m = g.FilterTypeConverter(props), tm.Model(props)
    try:
        return same(g, f, m, data), m
    finally:
        f.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused") or case.get("crashed"):
        with pytest.raises(ValueError):
            g.FilterTypeConverter(props)
        return
    data = base64.b64decode(case["in"])
    (ret, out), m = same_props(g, props, data)
    if case.get("undefined"):
        assert ret == g.MODIFIED and m.counters() == (len(props), 0, len(props), 0)
        return
    # the real plugin's bytes directly (bytes only: where the call answers NOTOUCH the processor handed its input on)
    assert (out if ret == g.MODIFIED else mm.processor_output(data)) == base64.b64decode(case["out"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_block_edges(g, n):
    data = mixed_records(n)
    for props in (P4, P64):
        (ret, out), m = same_props(g, props, data)
        assert ret == g.MODIFIED and m.counts() == (n, n) and len(synth.unpack_all(out)) == n
        assert m.counters()[0] >= (n + 2) // 3 and (n < 2 or m.counters()[1] >= 1)


PAIRS = [(tm.STR, tm.T_INT), (tm.STR, tm.T_UINT), (tm.STR, tm.T_HEX), (tm.STR, tm.T_FLOAT), (tm.STR, tm.T_BOOL),
         (tm.INT, tm.T_STR), (tm.INT, tm.T_FLOAT), (tm.INT, tm.T_UINT), (tm.UINT, tm.T_STR), (tm.UINT, tm.T_FLOAT), (tm.UINT, tm.T_INT),
         (tm.FLOAT, tm.T_STR), (tm.FLOAT, tm.T_INT), (tm.FLOAT, tm.T_UINT)]


@pytest.mark.parametrize("seed", [20271, 20272, 20273, 20274])
def test_fuzz(g, seed):
    r = random.Random(seed)
    pairs, rets, nrec = {}, {g.MODIFIED: 0, g.NOTOUCH: 0}, 0
    for i in range(30):
        props, keys = rnd_program(r, i)
        f, m = g.FilterTypeConverter(props), tm.Model(props)
        for _ in range(4):
            n = r.randrange(1, 100)
            ret, _ = same(g, f, m, b"".join(rnd_record(r, keys) for _ in range(n)))
            rets[ret] += 1
            nrec += n
        assert f.counters()[2:] == (0, 0)                               # the generator stays inside the defined conversions
        for k, (done, failed) in m.pairs.items():
            p = pairs.setdefault(k, [0, 0])
            p[0] += done
            p[1] += failed
        f.close()
    assert nrec >= 4000 and rets[g.MODIFIED] >= 60
    # every conversion pair both succeeded and failed: the test cannot pass by converting nothing
    assert not [k for k in PAIRS if pairs.get(k, [0, 0])[0] == 0 or pairs.get(k, [0, 0])[1] == 0], pairs


def f64(b):
    return synth.Raw(b"\xcb" + struct.pack(">Q", b))


def test_undefined_conversions_are_counted(g):
    vals = [f64(0x7ff8000000000000), f64(0xfff8000000000001), float("inf"), float("-inf"), 2.0 ** 63, -(2.0 ** 63), -(2.0 ** 63) - 2048, 1e300,
            -1e300, 2.0 ** 64, 2.0 ** 65, -1.0, -1.5, -12345.0, synth.Raw(b"\xca" + struct.pack(">f", float("inf"))), synth.Raw(b"\xca\xff\xc0\x00\x00"),
            1.5, -0.5, 2.0 ** 63 - 1024]
    body = synth.KV([(b"s%d" % i, v) for i, v in enumerate(vals)])
    data = rec(body, 1) + rec({"s0": 1.0}, 2)
    for to, undefined in (("int", 13), ("uint", 15)):
        # int: NaN, infinities and |v| >= 2^63 (11 of the f64 values, both f32 ones); uint: as well -1.0, -1.5, -12345.0, but not 2^63
        props = [("float_key", "s%d t%d %s" % (i, i, to)) for i in range(len(vals))]
        (ret, out), m = same_props(g, props, data)
        assert ret == g.MODIFIED and m.counters() == (len(vals) + 1, 0, undefined, 0)


def table_props(nbytes):
    return [("str_key", "abcd " + "t" * (nbytes - 24 - 4 - 3) + " int")]


def test_table_at_the_limit(g):
    data = rec({"abcd": "77", "x": 1}, 1) + rec({"x": 1}, 2)
    (ret, out), m = same_props(g, table_props(32768), data)
    assert ret == g.MODIFIED and m.counters() == (1, 0, 0, 0) and len(out) > 32768
    with pytest.raises(ValueError):
        g.FilterTypeConverter(table_props(32769))


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 70000])
def test_value_string_lengths(g, n):
    props = [("str_key", "i ti int"), ("str_key", "f tf float"), ("str_key", "i tu uint"), ("str_key", "f th hex")]
    data = (rec({"a": 1}, 1) + rec(synth.KV([(b"i", number_then_garbage(b" -1234567", n)), (b"f", number_then_garbage(b"12.625e1", n))]), 2) +
            rec({"i": "5"}, 3))
    (ret, out), m = same_props(g, props, data)
    assert ret == g.MODIFIED and m.counters()[0] >= 2 + (4 if n >= 31 else 0)


@pytest.mark.parametrize("klen", [1, 2, 3, 4, 5, 7, 8, 9])
def test_converted_key_is_the_last_bytes_of_the_chunk(g, klen):
    key = ("kabcdefgh"[:klen]).encode()
    longer = key + b"x"
    # the chunk ends on the key and a one-byte value; a key one byte longer and one one byte shorter stand in front of it
    data = rec(synth.KV([(longer, 1), (key[:-1], 2), (key, 7)]), 1)
    props = [("int_key", "%s t string" % key.decode()), ("int_key", "%s t2 string" % longer.decode())]
    (ret, out), m = same_props(g, props, data)
    assert ret == g.MODIFIED and m.counters() == (2, 0, 0, 0) and out.endswith(b"\xa2t2\xa11")
    data = rec({"zz": 1}, 1) + rec(synth.KV([(key, b"9")]), 2)
    (ret, out), m = same_props(g, [("str_key", "%s t int" % key.decode())], data)
    assert ret == g.MODIFIED and out.endswith(b"\xa1t\x09")


def test_chain_with_a_dropped_row_between_live_rows(g):
    lines = [b'{"status":"%d","size":%d,"lat":%s,"msg":"m%d"}' % (200 + i % 5 * 100, i * 7, [b"0.25", b"3.0", b"1e3"][i % 3], i) for i in range(300)]
    lines[7] = b'{"status":"abc","size":"big","msg":"nothing converts"}'
    recs = [rec({"log": ln}, 1700000000 + i, i) for i, ln in enumerate(lines)]
    blob = b"".join(recs)
    # the device chunk carries a row of length 0 (a record an earlier filter dropped) behind row 4 and two more at the end
    offs, p = [0], 0
    for i, rc in enumerate(recs):
        p += len(rc)
        offs.append(p)
        if i == 4:
            offs.append(p)
    offs += [p, p]
    props = [("str_key", "status status_i int"), ("int_key", "size size_s string"), ("float_key", "lat lat_s string")]
    grep = [("regex", "size_s ^1")]
    fp, ft, fg = g.FilterParser("log", [g.Parser(format="json")]), g.FilterTypeConverter(props), g.FilterGrep(grep)
    L = g.lib()
    d = L.flbgpu_dev_alloc(len(blob) + 16)
    L.flbgpu_memcpy_h2d(d, blob, len(blob))
    ro = struct.pack("<%dQ" % len(offs), *offs)
    d_off = L.flbgpu_dev_alloc(len(ro))
    L.flbgpu_memcpy_h2d(d_off, ro, len(ro))
    chain = g.FilterChain([fp, ft, fg])
    ret, out = chain.filter_dev(g.DevChunk(d, d_off, len(offs) - 1, len(blob)))
    buf = ctypes.create_string_buffer(max(out.bytes, 1))
    L.flbgpu_memcpy_d2h(buf, out.data, out.bytes)
    # the three CPU answers composed
    _, o1 = ob.FilterParser("log", [ob.Parser(format="json")]).filter(blob)
    m = tm.Model(props)
    r2, o2 = m.filter(o1)
    r3, o3 = ob.Grep(grep).filter(o2)
    assert r2 == g.MODIFIED and ret == g.MODIFIED and buf.raw[:out.bytes] == o3
    assert ft.counters() == m.counters() and ft.counters()[3] == 0 and m.counters()[1] >= 2
    st = chain.last_stats()[1]
    assert (st["in_records"], st["out_records"]) == m.counts() == (300, 300)
    # the same through the host-level call, without the empty rows
    assert chain.filter(blob) == (g.MODIFIED, o3)
    for f in (fp, ft, fg):
        f.close()
    L.flbgpu_dev_free(d)
    L.flbgpu_dev_free(d_off)


def test_buffer_reuse_and_counters_across_calls(g):
    f, m = g.FilterTypeConverter(P4), tm.Model(P4)
    total = [0, 0]
    for n in (700, 3, 1500, 1, 64):
        ret, out = same(g, f, m, mixed_records(n))
        assert ret == g.MODIFIED and len(synth.unpack_all(out)) == n
    # a call in which nothing converts, and one the decoder stops: NOTOUCH, and the counters keep adding up
    before = f.counters()
    assert same(g, f, m, rec({"status": "abc", "size": "x"}, 1) * 5) == (g.NOTOUCH, None)
    assert f.counters() == (before[0], before[1] + 10, 0, 0)
    bad = synth.mp([[synth.ext_ts(1, 0), {}], "not a map"])
    assert same(g, f, m, mixed_records(10) + bad + mixed_records(5)) == (g.NOTOUCH, None)
    assert f.counts() == (10, 10) and f.counters()[0] > before[0]
    assert same(g, f, m, bad + mixed_records(5)) == (g.NOTOUCH, None) and f.counts() == (0, 0)
    assert same(g, f, m, mixed_records(9) + b"\xc1")[0] == g.NOTOUCH
    assert same(g, f, m, mixed_records(9))[0] == g.MODIFIED
    f.close()

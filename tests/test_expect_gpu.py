"""filter_expect on the device (csrc/expect_kernels.inc through flbgpu_filter_expect_create) against the CPU model
(tests/expect_model.py) and against the recorded answers of the real plugin (tests/golden/expect_ref_cases.json): output bytes, return
value, record counts, the filter's own counters, and the failure table entry by entry with the message of every entry.  Every
comparison includes the size/emit mismatch counter, which the model holds at 0.  Nothing here provokes a fault: every input is one the
reference itself answers."""
import base64
import ctypes
import json
import os
import struct
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import expect_model as em
import modify_model as mm
import recmod_model as rm
from expect_chunks import BIG_T, GROUP_END, GROUP_START, R, fuzz_round, kv, map_n, rec, rows, sv
import oracle_binding as ob
import synth

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "expect_ref_cases.json")))["cases"]
MODIFIED, NOTOUCH = em.Model.MODIFIED, em.Model.NOTOUCH


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def has_a_record(data):
    try:
        mm.decode_event(data, 0)
        return True
    except mm.Bad:
        return False


def expected(m, data):
    """the model's answer -- but a chunk that holds no whole record never reaches a filter of this library: the call answers NOTOUCH
    where the reference hands back an empty buffer"""
    want = m.filter(data)
    if want == (MODIFIED, b"") and not has_a_record(data):
        return (NOTOUCH, None)
    return want


def same(g, f, m, data):
    before = m.counters()
    got = f.filter(data)
    want = expected(m, data)
    assert got == want, (got[0], want[0])
    assert f.counts() == m.counts()
    assert f.counters() == m.counters() and f.counters()[3] == 0
    assert f.failures() == [x.entry() for x in m.failures]
    assert [f.failure_text(i) for i in range(len(m.failures))] == m.texts(data)
    # what the shim turns into flb_engine_exit_status(config, 255)
    assert (m.counters()[2] - before[2]) * 255 == m.exit_status
    return got


def same_props(g, props, data):
    f, m = g.FilterExpect(props), em.Model(props)
    try:
        return same(g, f, m, data), m
    finally:
        f.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused") or case.get("crashed"):
        with pytest.raises(ValueError):
            g.FilterExpect(props)
        return
    data = base64.b64decode(case["in"])
    f = g.FilterExpect(props)
    ret, out = f.filter(data)
    # the real plugin's answer directly
    if case["ret"] == MODIFIED and not has_a_record(data):
        assert (ret, out) == (NOTOUCH, None)
    else:
        assert ret == case["ret"] and out == (base64.b64decode(case["out"]) if case["out"] is not None else None)
    assert [f.failure_text(i) for i in range(len(f.failures()))] == [base64.b64decode(x) + b"\n" for x in case["exceptions"]]
    assert f.counters()[2] * 255 == case["exit_status"]
    f.close()
    same_props(g, props, data)


@pytest.mark.parametrize("action", em.ACTIONS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_block_edges(g, n, action):
    # failures at both ends of every wave and on both sides of the workgroup edge: the table's placement crosses them
    failing = sorted({x for x in (0, 62, 63, 64, 127, 128, 254, 255, 256, n - 1) if x < n})
    props = [("key_exists", "$a"), ("action", action), ("key_not_exists", "$zz")]
    (ret, out), m = same_props(g, props, rows(n, failing))
    assert ret == (MODIFIED if action == "result_key" else NOTOUCH)
    assert len(m.failures) == (1 if action == "exit" else len(failing)) and m.counts()[0] == (1 if action == "exit" else n)
    # every record failing, none failing
    (ret, out), m = same_props(g, props, rows(n, range(n)))
    assert len(m.failures) == (1 if action == "exit" else n)
    (ret, out), m = same_props(g, props, rows(n))
    assert m.failures == [] and m.counters() == (n, 0, 0, 0)
    if action == "result_key":
        assert len(synth.unpack_all(out)) == n


@pytest.mark.parametrize("pos", [0, 63, 64, 256, 256 + 63, 511, 599])
def test_exit_first_failure(g, pos):
    # the first failure in the first and in the last lane of a wave and of the second workgroup; what fails behind it is never seen
    n = 600
    (ret, out), m = same_props(g, [("action", "exit"), ("key_exists", "$a")], rows(n, [pos, pos + 1, n - 1]))
    assert ret == NOTOUCH and m.counters() == (pos + 1, 1, 1, 0) and m.failures[0].rule.no == 1


@pytest.mark.parametrize("n", [14, 15, 16])
def test_body_sizes(g, n):
    data = rec(map_n(n, ("log", "x")), 5, 6) + rec(map_n(n), 7, 8)
    (ret, out), m = same_props(g, [("action", "result_key"), ("key_exists", "$log")], data)
    assert ret == MODIFIED and [len(x[1][1]) for x in synth.unpack_all(out)] == [n + 1, n + 1]


@pytest.mark.parametrize("n", [65534, 65535])
def test_wide_bodies(g, n):
    (ret, out), m = same_props(g, [("action", "result_key"), ("key_exists", "$k7"), ("key_not_exists", "$k%d" % (n - 1))], rec(map_n(n), 5, 6))
    assert ret == MODIFIED and out[13:18] == b"\xdf" + struct.pack(">I", n + 1) and len(m.failures) == 1


@pytest.mark.parametrize("n", [0, 1, 31, 32, 255, 256, 30000])
def test_result_key_lengths(g, n):
    key = "r" * n
    (ret, out), m = same_props(g, [("action", "result_key"), ("result_key", key), ("key_exists", "$a")], rows(5, [3]))
    assert ret == MODIFIED and [x[1][1][0] for x in synth.unpack_all(out)] == [(key.encode(), v) for v in (True, True, True, False, True)]


def keyed(n, missing):
    return kv(*[("k%d" % i, i) for i in range(n) if i != missing])


@pytest.mark.parametrize("action", ["warn", "result_key"])
def test_rule_counts(g, action):
    body = kv(("a", 1))
    for nrules in (0, 1):
        props = [("key_exists", "$b")] * nrules + [("action", action)]
        (ret, out), m = same_props(g, props, rec(body, 1) + rec(kv(("b", 1)), 2))
        assert len(m.failures) == nrules
    # 64 rules (the action's among them), the failing rule being the first, the last and each one in turn
    props = [("key_exists", "$k%d" % i) for i in range(40)] + [("action", action)] + [("key_exists", "$k%d" % i) for i in range(40, 63)]
    data = b"".join(rec(keyed(63, i), 100 + i) for i in range(63)) + rec(keyed(63, -1), 500)
    (ret, out), m = same_props(g, props, data)
    assert [x.rule.no for x in m.failures] == [i if i < 40 else i + 1 for i in range(63)]


def test_group_markers(g):
    ok, bad = rec(kv(("a", 1)), 1), rec(kv(("b", 1)), 2)
    for action in em.ACTIONS:
        props = [("key_exists", "$a"), ("action", action)]
        for data in (GROUP_START + ok + bad + GROUP_END, ok + GROUP_START + bad + GROUP_END + ok, GROUP_START + GROUP_END, bad + GROUP_START + ok + GROUP_END,
                     rows(70, [64]) + GROUP_START + rows(3, [1]) + GROUP_END + GROUP_END):
            same_props(g, props, data)


def test_decoder_errors_and_times(g):
    ok, bad = rec(kv(("a", 1)), 1), rec(kv(("b", 1)), 2)
    not_a_map = synth.mp([[synth.ext_ts(1, 0), {}], "not a map"])
    late = synth.mp([BIG_T, kv(("b", "late"))])
    cut = rec(kv(("a", "long value of a cut record")), 3)
    for action in em.ACTIONS:
        props = [("key_exists", "$a"), ("action", action)]
        for data in (ok + bad + b"\xc1\xff", ok + bad + cut[:-4], bad + ok + cut[:-26], not_a_map + bad, bad + not_a_map + bad, rows(70, [3, 66]) + not_a_map + rows(5, [1]),
                     late + ok + bad, ok + late + bad, bad + late, late, ok + synth.mp([-3.0, kv(("b", 1))]) + bad, synth.mp([-1.5, kv(("b", 1))]) + bad,
                     synth.mp([1700000000, kv(("b", 1))]) + synth.mp([1700000000.25, kv(("a", 1))]), b""):
            same_props(g, props, data)


FUZZ_SEEDS = range(30411, 30431)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(g, seed):
    props, data = fuzz_round(seed)
    (ret, out), m = same_props(g, props, data)
    assert m.counts()[0] >= 1


def test_fuzz_rounds_meet_both_answers():
    # the rounds prove nothing unless every action meets calls without a failure and calls with some
    seen = set()
    for seed in FUZZ_SEEDS:
        props, data = fuzz_round(seed)
        m = em.Model(props)
        m.filter(data)
        seen.add((m.cfg.action, bool(m.failures)))
    assert seen == {(a, f) for a in (em.WARN, em.EXIT, em.RESULT_KEY) for f in (False, True)}


def dev_chunk(g, blob, offs):
    L = g.lib()
    d = L.flbgpu_dev_alloc(len(blob) + 16)
    L.flbgpu_memcpy_h2d(d, blob, len(blob))
    ro = struct.pack("<%dQ" % len(offs), *offs)
    d_off = L.flbgpu_dev_alloc(len(ro))
    L.flbgpu_memcpy_h2d(d_off, ro, len(ro))
    return g.DevChunk(d, d_off, len(offs) - 1, len(blob)), (d, d_off)


def dev_bytes(g, out):
    buf = ctypes.create_string_buffer(max(out.bytes, 1))
    g.lib().flbgpu_memcpy_d2h(buf, out.data, out.bytes)
    return buf.raw[:out.bytes]


def dev_failures(g, f):
    n, ptr = f.failures_dev()
    buf = ctypes.create_string_buffer(max(n * 40, 1))
    if n:
        g.lib().flbgpu_memcpy_d2h(buf, ptr, n * 40)
    out = []
    for i in range(n):
        in_off, val_off, ln, val_len, rule, kind, vt, _ = struct.unpack_from("<QQIIIIII", buf.raw, 40 * i)
        out.append((in_off, ln, rule, kind, vt, val_off, val_len))
    return out


def bounds_of(blob):
    offs, p = [0], 0
    while p < len(blob):
        p = mm.decode_event(blob, p)[0]
        offs.append(p)
    return offs


def test_device_chunk_with_dropped_rows(g):
    blob = rows(300, [4, 5, 250])
    b = bounds_of(blob)
    # a row of length 0 (a record an earlier filter dropped) behind row 4 and two more at the end
    offs = b[:6] + [b[5]] + b[6:] + [b[-1], b[-1]]
    chunk, mem = dev_chunk(g, blob, offs)
    for action in em.ACTIONS:
        props = [("key_val_eq", "$a v4"), ("action", action)]
        f, m = g.FilterExpect(props), em.Model(props)
        want = m.filter(blob)
        ret, out = f.filter_dev(chunk)
        assert ret == want[0] and (ret != MODIFIED or dev_bytes(g, out) == want[1])
        assert dev_failures(g, f) == f.failures() == [x.entry() for x in m.failures] and len(m.failures) >= 1
        assert [f.failure_text(i) for i in range(len(m.failures))] == m.texts(blob)
        assert f.counts() == m.counts() and f.counters() == m.counters()
        f.close()
    for d in mem:
        g.lib().flbgpu_dev_free(d)


def test_chains(g):
    n = 300
    blob = rows(n, [0, 7, 64, 299])
    chunk, mem = dev_chunk(g, blob, bounds_of(blob))
    RM = [("Record", "cluster eu-1"), ("Remove_key", "n")]
    EX = [("key_exists", "$a"), ("key_exists", "$cluster")]
    made = []

    def chain_of(*fs):
        made.extend(fs)
        return g.FilterChain(list(fs))
    # [record_modifier, expect(result_key)]: the table's offsets index record_modifier's output
    r1, o1 = rm.Model(RM).filter(blob)
    assert r1 == MODIFIED
    fe, m = g.FilterExpect(EX + [("action", "result_key")]), em.Model(EX + [("action", "result_key")])
    want = m.filter(o1)
    chain = chain_of(g.FilterRecordModifier(RM), fe)
    assert chain.filter(blob) == want and want[0] == MODIFIED
    assert fe.failures() == [x.entry() for x in m.failures] and len(m.failures) == 4 and fe.failures_input() == o1
    assert [fe.failure_text(i) for i in range(4)] == m.texts(o1)
    st = chain.last_stats()[1]
    assert (st["in_records"], st["out_records"]) == m.counts() == (n, n)
    ret, out = chain.filter_dev(chunk)
    assert ret == MODIFIED and dev_bytes(g, out) == want[1] and dev_failures(g, fe) == [x.entry() for x in m.failures]
    # [expect(result_key), record_modifier] and [expect(result_key), grep]: grep keeps the records that failed
    fe2, m2 = g.FilterExpect([("key_exists", "$a"), ("action", "result_key")]), em.Model([("key_exists", "$a"), ("action", "result_key")])
    r2, o2 = m2.filter(blob)
    want = rm.Model(RM).filter(o2)
    chain = chain_of(fe2, g.FilterRecordModifier(RM))
    assert chain.filter(blob) == want and fe2.failures() == [x.entry() for x in m2.failures] and fe2.failures_input() == blob
    ret, out = chain.filter_dev(chunk)
    assert ret == MODIFIED and dev_bytes(g, out) == want[1]
    grep = [("exclude", "a .")]
    fe3 = g.FilterExpect([("key_exists", "$a"), ("action", "result_key")])
    want = ob.Grep(grep).filter(o2)
    assert want[0] == MODIFIED and 4 <= len(synth.unpack_all(want[1])) < n
    chain = chain_of(fe3, g.FilterGrep(grep))
    assert chain.filter(blob) == want
    ret, out = chain.filter_dev(chunk)
    assert ret == MODIFIED and dev_bytes(g, out) == want[1]
    # [grep, expect(warn)]: the table's offsets index what grep kept
    keep = [("regex", "pad x")]
    r4, o4 = ob.Grep(keep).filter(blob)
    fe4, m4 = g.FilterExpect(EX[:1]), em.Model(EX[:1])
    assert m4.filter(o4) == (NOTOUCH, None) and len(m4.failures) == 2
    chain = chain_of(g.FilterGrep(keep), fe4)
    assert chain.filter(blob) == (r4, o4)
    inp = fe4.failures_input()
    assert [inp[e[0]:e[0] + e[1]] for e in fe4.failures()] == [o4[x.off:x.off + x.len] for x in m4.failures]
    assert [fe4.failure_text(i) for i in range(2)] == m4.texts(o4)
    # [record_modifier, expect(warn), grep]: warn in the middle hands record_modifier's chunk on
    fe5, m5 = g.FilterExpect(EX), em.Model(EX)
    assert m5.filter(o1) == (NOTOUCH, None)
    want = ob.Grep(keep).filter(o1)
    chain = chain_of(g.FilterRecordModifier(RM), fe5, g.FilterGrep(keep))
    assert chain.filter(blob) == want and want[0] == MODIFIED
    assert fe5.failures() == [x.entry() for x in m5.failures] and fe5.failures_input() == o1
    ret, out = chain.filter_dev(chunk)
    assert ret == MODIFIED and dev_bytes(g, out) == want[1] and dev_failures(g, fe5) == [x.entry() for x in m5.failures]
    for f in made:
        f.close()
    for d in mem:
        g.lib().flbgpu_dev_free(d)


def test_buffer_reuse_and_counters_across_calls(g):
    props = [("key_exists", "$a"), ("action", "result_key"), ("key_val_eq", "$a v3")]
    f, m = g.FilterExpect(props), em.Model(props)
    for n in (700, 3, 1500, 1, 64):
        ret, out = same(g, f, m, rows(n, [0, n // 2]))
        assert ret == MODIFIED and len(synth.unpack_all(out)) == n
    # a call without failures leaves an empty table behind the full one of the call before
    assert same(g, f, m, rec(kv(("a", "v3")), 1) * 5)[0] == MODIFIED and f.failures() == []
    f.close()

"""filter_kubernetes on the device (csrc/kube_kernels.inc through flbgpu_filter_kubernetes_create) against the CPU model
(tests/kube_model.py) and against the recorded answers of the real plugin (tests/golden/kube_ref_cases.json): output bytes, return
value, record counts and the filter's own counters.  Every comparison includes the size/emit mismatch counter, which the model holds
at 0.  Nothing here provokes a fault: every input is one the reference itself answers."""
import base64
import ctypes
import json
import os
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import kube_model as km
import modify_model as mm
import oracle_binding as ob
import synth
from kube_chunks import BIG_T, GROUP_END, GROUP_START, STOCK_TAG, alignment_chunk, blob_of, docker, fuzz_round, json_line, kv, nested, pod_meta, rec, rows

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "kube_ref_cases.json")))["cases"]
MODIFIED, NOTOUCH = km.Model.MODIFIED, km.Model.NOTOUCH
ML = [("merge_log", "on")]


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def has_a_record(data):
    """whether the chunk begins with one whole msgpack object (the host-level call's rows; the filter's decoder may still refuse it)"""
    try:
        mm.unpack(data, 0)
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


def same(f, m, data):
    got = f.filter(data)
    want = expected(m, data)
    assert got == want, (got[0], want[0])
    assert f.counts() == m.counts()
    assert f.counters() == m.counters() and f.counters()[3] == 0
    return got


def pair(g, props, pod=None, ns=None, tag=None):
    f, m = g.FilterKubernetes(props), km.Model(props)
    if tag is not None:
        assert f.set_tag(tag) == m.set_tag(tag)
    elif pod is not None or ns is not None:
        f.set_meta(pod, ns)
        m.set_meta(pod, ns)
    return f, m


def same_props(g, props, data, pod=None, ns=None, tag=None):
    f, m = pair(g, props, pod, ns, tag)
    try:
        return same(f, m, data), m
    finally:
        f.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused") or case.get("crashed"):
        with pytest.raises(ValueError):
            g.FilterKubernetes(props)
        return
    data = base64.b64decode(case["in"])
    tag_mode = km.parse(props).tag_meta
    pod, ns = (base64.b64decode(case[k]) if case.get(k) else None for k in ("pod", "ns"))
    f, m = pair(g, props, pod, ns, case["tag"] if tag_mode else None)
    ret, out = f.filter(data)
    # the real plugin's answer directly
    if case["ret"] == MODIFIED and not has_a_record(data):
        assert (ret, out) == (NOTOUCH, None)
    else:
        assert ret == case["ret"] and out == (base64.b64decode(case["out"]) if case["out"] is not None else None)
    f.close()
    f, m = pair(g, props, pod, ns, case["tag"] if tag_mode else None)
    same(f, m, data)
    f.close()


FUZZ_SEEDS = range(41001, 41021)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(g, seed):
    props, pod, ns, data = fuzz_round(seed)
    (ret, out), m = same_props(g, props, data, pod, ns)
    assert ret == MODIFIED and m.counts()[0] >= 1


def test_fuzz_rounds_meet_every_answer():
    # the rounds prove nothing unless they merge, exclude, count deviations and leave records alone
    seen = [0, 0, 0]
    for seed in FUZZ_SEEDS:
        props, pod, ns, data = fuzz_round(seed)
        m = km.Model(props)
        m.set_meta(pod, ns)
        assert m.filter(data)[0] == MODIFIED
        seen = [a + (b > 0) for a, b in zip(seen, m.counters())]
    assert min(seen) >= 2


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_block_edges(g, n):
    edge = sorted({x for x in (0, 62, 63, 64, 127, 128, 254, 255, 256, n - 1) if x < n})
    pod = pod_meta() + km.props_array(False, True)
    # stderr rows (excluded) at both ends of every wave and on both sides of the workgroup edge; plain rows beside them
    (ret, out), m = same_props(g, ML, rows(n, stderr=edge, plain=[x + 1 for x in edge]), pod)
    assert ret == MODIFIED and m.counters()[1] == len(edge) and len(synth.unpack_all(out)) == n - len(edge)
    (ret, out), m = same_props(g, ML + [("keep_log", "off")], rows(n), pod, blob_of(7))
    assert m.counters() == (n, 0, 0, 0) and len(synth.unpack_all(out)) == n
    # every record excluded: an empty MODIFIED
    (ret, out), m = same_props(g, ML, rows(n, stderr=range(n)), pod)
    assert (ret, out) == (MODIFIED, b"") and m.counts() == (n, 0)


@pytest.mark.parametrize("nblob", [1, 3, 4, 5, 63, 64, 65])
def test_blob_sizes_and_alignments(g, nblob):
    # the alignment chunk puts the tail at every destination address mod 4; with a namespace entry behind the pod's the tail's
    # own length shifts the next record as well
    for ns in (None, blob_of(1), blob_of(nblob)):
        f, m = pair(g, ML, blob_of(nblob), ns)
        assert f.layout()["in_lds"] and f.layout()["tail_bytes"] == len(m.tail()[0])
        ret, out = same(f, m, alignment_chunk())
        assert ret == MODIFIED
        same(f, m, rows(130, stderr=(3,), plain=(0, 129)))
        f.close()
    f, m = pair(g, ML, None, blob_of(nblob))
    same(f, m, alignment_chunk())
    f.close()


def test_alignment_chunk_meets_every_residue():
    m = km.Model(ML)
    m.set_meta(blob_of(5), None)
    ret, out = m.filter(alignment_chunk())
    tail = m.tail()[0]
    starts, p = set(), 0
    while p < len(out):
        end = mm.decode_event(out, p)[0]
        assert out[end - len(tail):end] == tail
        starts.add((end - len(tail)) % 4)
        p = end
    assert starts == {0, 1, 2, 3}


def test_large_blob_from_hbm(g):
    # a tail over the default LDS budget is read from HBM / L2
    pod = pod_meta(400, 9000)
    f, m = pair(g, ML, pod, blob_of(40))
    assert not f.layout()["in_lds"] and f.layout()["tail_bytes"] > 15360
    same(f, m, alignment_chunk())
    same(f, m, rows(200, stderr=(0, 199), plain=(64,)))
    f.close()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_lds_budget_boundary(delta):
    # the switch is read at create: a fresh process for each budget.  tail = "kubernetes" (11 bytes) + the pod blob
    nblob = 37
    budget = 11 + nblob + delta
    env = dict(os.environ, FLBGPU_KUBE_LDS_BLOB=str(budget))
    r = subprocess.run([sys.executable, os.path.join(HERE, "kube_lds_child.py"), str(budget), str(nblob), "1" if delta >= 0 else "0"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout.decode().strip().endswith("ok"), r.stderr.decode()[-800:]


def test_only_the_last_record_of_a_wave_is_kept(g):
    pod = pod_meta() + km.props_array(True, False)
    (ret, out), m = same_props(g, ML, rows(192, stderr=(63, 127, 191)), pod)
    assert m.counts() == (192, 3) and m.counters()[1] == 189
    (ret, out), m = same_props(g, ML, rows(192, stderr=(0, 64, 128)), pod)
    assert m.counts() == (192, 3)


def test_deferred_rows_first_and_last_in_a_workgroup(g):
    # nesting past the register walker and a decimal that needs the exact conversion: the exact instantiation takes those rows
    hard = ['{"a":' + "3." + "1" * 40 + ',"s":"t\\n"}', nested(70), nested(65), nested(64), nested(63), '{"d":1.7976931348623157e308,"e":4.9e-324,"f":0.1e-400}']
    where = {0: 0, 63: 1, 64: 2, 255: 3, 256: 4, 511: 5, 512: 0, 599: 1}
    data = b"".join(docker(i, hard[where[i]] if i in where else json_line(i)) for i in range(600))
    for props in (ML, ML + [("keep_log", "off"), ("merge_log_key", "deep")]):
        (ret, out), m = same_props(g, props, data, blob_of(33), blob_of(6))
        assert ret == MODIFIED and m.counters()[0] == 600


def test_times_and_decoder_errors(g):
    a, b = rec(kv(("log", '{"a":1}')), 1), rec(kv(("nolog", "b")), 2)
    late = synth.mp([BIG_T, kv(("log", "late"))])
    not_a_map = synth.mp([[synth.ext_ts(1, 0), {}], "not a map"])
    cut = rec(kv(("log", "long value of a cut record")), 3)
    for data in (late + a + b, a + late + b, a + b + late, late, rows(70) + late + rows(3), a + b + b"\xc1\xff", a + b + cut[:-4], not_a_map + a, a + not_a_map + late,
                 a + late + not_a_map, rows(70) + not_a_map + rows(5), GROUP_START + a + GROUP_END + b, GROUP_START + GROUP_END, b"",
                 synth.mp([1700000000, kv(("log", '{"a":1}'))]) + synth.mp([1700000000.25, kv(("x", 1))]), a + synth.mp([-3.0, kv(("b", 1))]) + b):
        same_props(g, ML, data, blob_of(9))


def test_merge_log_key_lengths(g):
    for n in (0, 1, 31, 32, 255, 256, 32767):
        (ret, out), m = same_props(g, ML + [("merge_log_key", "k" * n)], rows(5, plain=(2,)), blob_of(5))
        assert ret == MODIFIED and m.counters()[0] == 4


def test_tag_mode(g):
    props = ML + [("use_tag_for_meta", "on")]
    f, m = g.FilterKubernetes(props), km.Model(props)
    data = rows(70, plain=(3,))
    # before the first set_tag, and after one that failed: NOTOUCH
    assert same(f, m, data) == (NOTOUCH, None)
    assert f.set_tag(STOCK_TAG) == m.set_tag(STOCK_TAG) == 0
    assert same(f, m, data)[0] == MODIFIED
    assert f.set_tag("kube.var.log.containers.nomatch") == m.set_tag("kube.var.log.containers.nomatch") == -1
    assert same(f, m, data) == (NOTOUCH, None)
    assert f.set_tag(STOCK_TAG) == m.set_tag(STOCK_TAG) == 0
    assert same(f, m, data)[0] == MODIFIED
    f.close()


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


def bounds_of(blob):
    offs, p = [0], 0
    while p < len(blob):
        p = mm.decode_event(blob, p)[0]
        offs.append(p)
    return offs


def test_chain_behind_grep_and_in_front_of_modify(g):
    n = 300
    blob = rows(n, stderr=(5, 64, 299), plain=(0, 63, 128))
    chunk, mem = dev_chunk(g, blob, bounds_of(blob))
    grep = [("exclude", "log plain")]
    MOD = [("Add", "cluster eu-1"), ("Remove", "time")]
    pod = pod_meta() + km.props_array(False, True)
    r1, o1 = ob.Grep(grep).filter(blob)
    assert r1 == MODIFIED
    fk, m = pair(g, ML, pod, blob_of(12))
    r2, o2 = m.filter(o1)
    want = mm.Model(MOD).filter(o2)
    assert r2 == MODIFIED and want[0] == MODIFIED and m.counts() == (n - 3, n - 6)
    fs = [g.FilterGrep(grep), fk, g.FilterModify(MOD)]
    chain = g.FilterChain(fs)
    assert chain.filter(blob) == want
    st = chain.last_stats()[1]
    assert (st["in_records"], st["out_records"]) == m.counts() and fk.counters() == m.counters() and fk.counters()[3] == 0
    ret, out = chain.filter_dev(chunk)
    assert ret == MODIFIED and dev_bytes(g, out) == want[1]
    # the filter alone on the device chunk, with rows an earlier filter dropped (length 0) among them
    b = bounds_of(blob)
    offs = b[:6] + [b[5]] + b[6:] + [b[-1], b[-1]]
    chunk2, mem2 = dev_chunk(g, blob, offs)
    m2 = km.Model(ML)
    m2.set_meta(pod, blob_of(12))
    want2 = m2.filter(blob)
    ret, out = fk.filter_dev(chunk2)
    assert ret == want2[0] == MODIFIED and dev_bytes(g, out) == want2[1] and fk.counts() == m2.counts()
    for f in fs:
        f.close()
    for d in mem + mem2:
        g.lib().flbgpu_dev_free(d)


def test_two_calls_with_a_set_meta_between(g):
    f, m = pair(g, ML)
    for n, pod, ns in ((700, None, None), (3, blob_of(5), None), (1500, pod_meta() + km.props_array(True, False), blob_of(9)), (1, None, blob_of(3)),
                       (64, pod_meta(400, 9000), None), (65, blob_of(64), blob_of(64))):
        f.set_meta(pod, ns)
        m.set_meta(pod, ns)
        ret, out = same(f, m, rows(n, stderr=(0, n // 2), plain=(n - 1,)))
        assert ret == MODIFIED
    # a refused entry leaves the metadata of the call before
    with pytest.raises(ValueError):
        f.set_meta(b"\x81\xa1k", None)
    assert same(f, m, rows(10))[0] == MODIFIED
    f.close()

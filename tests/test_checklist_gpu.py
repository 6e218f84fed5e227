"""filter_checklist on the device (csrc/checklist_kernels.inc through flbgpu_filter_checklist_create) against the CPU model
(tests/checklist_model.py) and against the recorded answers of the real plugin (tests/golden/checklist_ref_cases.json): output bytes,
return value, record counts and the filter's own counters.  Every comparison includes the size/emit mismatch counter, which the
model holds at 0."""
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
import checklist_model as cm
import recmod_model as rm
from checklist_chunks import GROUP_END, GROUP_START, LIKE_EDGES, LIST, MISSING, fuzz_round, kv, rec, sv, third_list, third_records
import oracle_binding as ob
import synth

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "checklist_ref_cases.json")))["cases"]
RAN_BUT_REFUSED = {"ld_nul_at_line_start"}
REC = [("record", "flag new"), ("record", "hit true")]


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def on_disk(props, lst, tmp_path):
    path = str(tmp_path / "list.txt")
    if lst is not None:
        with open(path, "wb") as f:
            f.write(lst)
    sub = {LIST: path, MISSING: str(tmp_path / "no_such_file")}
    return [(k, sub.get(v, v)) for k, v in props]


def same(g, f, m, data):
    got = f.filter(data)
    want = m.filter(data)
    assert got == want, (got[0], want[0])
    assert f.counts() == m.counts()
    assert f.counters() == m.counters() and f.counters()[3] == 0
    return got


def same_props(g, props, lst, data, tmp_path):
    props = on_disk(props, lst, tmp_path)
    f, m = g.FilterChecklist(props), cm.Model(props)
    try:
        return same(g, f, m, data), m
    finally:
        f.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case, tmp_path):
    props = [tuple(p) for p in case["props"]]
    lst = base64.b64decode(case["list"]) if case["list"] is not None else None
    if case.get("refused") or case.get("crashed") or case["name"] in RAN_BUT_REFUSED:
        with pytest.raises(ValueError):
            g.FilterChecklist(on_disk(props, lst, tmp_path))
        return
    (ret, out), m = same_props(g, props, lst, base64.b64decode(case["in"]), tmp_path)
    # the real plugin's answer directly
    assert ret == case["ret"] and out == (base64.b64decode(case["out"]) if case["out"] is not None else None)


@pytest.mark.parametrize("partial", [False, True], ids=["exact", "partial"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_block_edges(g, n, partial, tmp_path):
    props = [("file", LIST), ("mode", "partial" if partial else "exact")] + REC
    (ret, out), m = same_props(g, props, third_list(partial), third_records(n), tmp_path)
    assert ret == g.MODIFIED and m.counts() == (n, n) and len(synth.unpack_all(out)) == n
    assert m.counters() == ((n + 2) // 3, 0, 0, 0)


def lookups(values):
    return b"".join(rec(kv(("i", i), ("log", sv(v))), 1700000000 + i, i) for i, v in enumerate(values))


@pytest.mark.parametrize("n", [0, 1, 2, 511, 512, 513])
def test_exact_table_sizes(g, n, tmp_path):
    # 2 * n crosses a slot-count step between 511, 512 and 513 entries
    entries = [b"entry-%d-%s" % (i, b"x" * (i % 9)) for i in range(n)]
    values = entries + [b"entry-%d" % i for i in range(40)] + [b"", b"e"] + entries[:3]
    (ret, out), m = same_props(g, [("file", LIST)] + REC, b"".join(e + b"\n" for e in entries), lookups(values), tmp_path)
    assert m.counters()[0] == n + min(n, 3) and ret == (g.MODIFIED if n else g.NOTOUCH)


def test_exact_dense_table_chains_and_wraps(g, tmp_path, monkeypatch):
    monkeypatch.setenv("FLBGPU_CHECKLIST_DENSE", "1")
    entries = [b"k%03d-%s" % (i, bytes([97 + i % 26]) * (i % 13)) for i in range(100)]
    near = []
    for e in entries:
        near += [e[:-1] + bytes([e[-1] ^ 1]), e[:-1], e + b"-"]       # the same length with the last byte changed, a true prefix, one byte longer
    near = [v for v in near if v not in entries]
    assert len(near) >= 290
    # 100 entries in 128 slots: long probe chains, and chains that wrap around the end of the table
    assert ";slots=128;" in g.checklist_parse_check(on_disk([("file", LIST)], b"".join(e + b"\n" for e in entries), tmp_path))
    (ret, out), m = same_props(g, [("file", LIST)] + REC, b"".join(e + b"\n" for e in entries), lookups(entries + near), tmp_path)
    assert ret == g.MODIFIED and m.counters()[0] == 100


@pytest.mark.parametrize("fold", ["off", "on"])
def test_exact_value_lengths(g, fold, tmp_path):
    lens = [1, 3, 4, 5, 2045]
    entries = [bytes([65 + i]) * n for i, n in enumerate(lens)]
    values = [b""]
    for e in entries:
        values += [e, e[:-1] + b"!", e + e[-1:], e.lower(), e[:-1]]
    values += [entries[-1] + b"E", b"E" * 70000, entries[3] + b"\0"]     # 2046 bytes, 70 000 bytes, a NUL behind an entry
    (ret, out), m = same_props(g, [("file", LIST), ("ignore_case", fold)] + REC, b"".join(e + b"\n" for e in entries), lookups(values), tmp_path)
    # the entry itself, and with ignore_case its lower-case twin; one byte short of "A" is the empty value, never found
    assert ret == g.MODIFIED and m.counters()[0] == (10 if fold == "on" else 5)


def test_partial_buckets(g, tmp_path):
    lst = b"abc\nac\n%X\n_b%z\n\xc3\xa9t\n% \nAbd\n"
    values = [b"abcd", b"ab", b"acid", b"qqX", b"abX", b"zbyyz", b"zbyy", b"\xc3\xa9t\xc3\xa9", b"\xc3\xa8t", b"q q", b"qq", b"", b"Abd", b"abd", b"X",
              b"\xe9t", b"a", b"\xffX", b"\0X"]
    (ret, out), m = same_props(g, [("file", LIST), ("mode", "partial")] + REC, lst, lookups(values), tmp_path)
    # literal buckets (abcd, acid, Abd), a first byte whose bucket is empty (qqX, q q), the `any` bucket where the literal one fails
    # (abX), '_' first (zbyyz), a byte >= 0x80 first, X alone, 0xff first
    assert ret == g.MODIFIED and m.counters()[0] == 10
    (ret, out), m = same_props(g, [("file", LIST), ("mode", "partial"), ("ignore_case", "true")] + REC, lst, lookups(values), tmp_path)
    # folded: the list's Abd and %X, the values' first bytes (Abd, abd and ABX now meet abd and %x)
    assert ret == g.MODIFIED and m.counters()[0] == 11
    (ret, out), m = same_props(g, [("file", LIST), ("mode", "partial"), ("ignore_case", "true")] + REC, b"Hit\n", lookups([b"HIT!", b"hIt", b"hi"]), tmp_path)
    assert m.counters()[0] == 2


@pytest.mark.parametrize("i", range(len(LIKE_EDGES)))
def test_like_edges_on_the_device(g, i, tmp_path):
    value, entry, want = LIKE_EDGES[i]
    # a record in front that few entries match (those that begin with '%' or '_', and U+FFFD: 0xfe alone reads as that)
    filler = cm.like(b"\xfe never", entry)
    (ret, out), m = same_props(g, [("file", LIST), ("mode", "partial")] + REC, entry + b"\n", lookups([b"\xfe never", value]), tmp_path)
    assert m.counters()[0] == want + filler and ret == (g.MODIFIED if want or filler else g.NOTOUCH)


@pytest.mark.parametrize("partial", [False, True], ids=["exact", "partial"])
@pytest.mark.parametrize("seed", [20311, 20312, 20313, 20314])
def test_fuzz(g, seed, partial, tmp_path):
    props, lst, data = fuzz_round(seed, partial)
    (ret, out), m = same_props(g, [("file", LIST)] + props, lst, data, tmp_path)
    n, matched = m.counts()[0], m.counters()[0]
    # the round proves nothing unless both answers are common
    assert n >= 100 and matched * 5 >= n and (n - matched) * 5 >= n, (n, matched)


def test_group_markers_dropped_rows_and_a_decoder_error(g, tmp_path):
    hit, no = kv(("log", "hit-0")), kv(("log", "nope"))
    bad = synth.mp([[synth.ext_ts(1, 0), {}], "not a map"])
    props = [("file", LIST)] + REC
    for data in (GROUP_START + rec(no, 1) + GROUP_END + rec(no, 2) + GROUP_START + rec(hit, 3) + GROUP_START + GROUP_END + rec(no, 4) + GROUP_END,
                 rec(hit, 1) + rec(no, 2) + bad + rec(hit, 3), bad + rec(hit, 3), rec(no, 1) + rec(no, 2) + b"\xc1", third_records(70) + bad + third_records(5)):
        same_props(g, props, third_list(False), data, tmp_path)
    # a first record the encoder refuses: the output stays empty until the next match, which emits everything in front of it
    late = synth.mp([synth.Raw(b"\xcf" + struct.pack(">Q", 2 ** 33)), hit])
    (ret, out), m = same_props(g, props, third_list(False), late + rec(no, 2) + GROUP_START + rec(hit, 3) + rec(no, 4), tmp_path)
    assert ret == g.MODIFIED and m.counters()[:2] == (2, 1) and out.startswith(late)
    # ... also when that match is refused as well: the raw span alone is the output
    (ret, out), m = same_props(g, props, third_list(False), late + rec(no, 2) + late, tmp_path)
    assert ret == g.MODIFIED and m.counters()[:2] == (2, 2) and out == late + rec(no, 2) and m.counts() == (3, 2)
    (ret, out), m = same_props(g, props, third_list(False), late + rec(no, 2), tmp_path)
    assert ret == g.NOTOUCH and m.counters()[:2] == (1, 1) and m.counts() == (2, 2)


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


@pytest.mark.parametrize("partial", [False, True], ids=["exact", "partial"])
def test_chains(g, partial, tmp_path):
    n = 300
    blob = third_records(n)
    offs = [0]
    # the record boundaries, and a row of length 0 (a record an earlier filter dropped) behind row 4 and two more at the end
    p = 0
    bounds = []
    while p < len(blob):
        end = cm.mm.decode_event(blob, p)[0]
        bounds.append(end)
        p = end
    for i, e in enumerate(bounds):
        offs.append(e)
        if i == 4:
            offs.append(e)
    offs += [bounds[-1], bounds[-1]]
    props = on_disk([("file", LIST), ("mode", "partial" if partial else "exact")] + REC, third_list(partial), tmp_path)
    RM = [("Record", "cluster eu-1"), ("Remove_key", "n")]
    grep = [("regex", "flag ^new$")]
    chunk, mem = dev_chunk(g, blob, offs)
    # [record_modifier, checklist]
    fr, fc = g.FilterRecordModifier(RM), g.FilterChecklist(props)
    r1, o1 = rm.Model(RM).filter(blob)
    m = cm.Model(props)
    want = m.filter(o1)
    assert r1 == g.MODIFIED and want[0] == g.MODIFIED
    chain = g.FilterChain([fr, fc])
    assert chain.filter(blob) == want
    st = chain.last_stats()[1]
    assert (st["in_records"], st["out_records"]) == m.counts() == (n, n)
    ret, out = chain.filter_dev(chunk)
    assert ret == g.MODIFIED and dev_bytes(g, out) == want[1]
    assert fc.counters() == (2 * m.counters()[0], 0, 0, 0)
    # [checklist, grep]: grep keeps the matched records
    fc2, fg = g.FilterChecklist(props), g.FilterGrep(grep)
    m2 = cm.Model(props)
    r2, o2 = m2.filter(blob)
    want = ob.Grep(grep).filter(o2)
    assert want[0] == g.MODIFIED and len(synth.unpack_all(want[1])) == n // 3
    chain = g.FilterChain([fc2, fg])
    assert chain.filter(blob) == want
    ret, out = chain.filter_dev(chunk)
    assert ret == g.MODIFIED and dev_bytes(g, out) == want[1]
    assert fc2.counters() == (2 * m2.counters()[0], 0, 0, 0)
    for f in (fr, fc, fc2, fg):
        f.close()
    for d in mem:
        g.lib().flbgpu_dev_free(d)


def test_buffer_reuse_and_counters_across_calls(g, tmp_path):
    props = on_disk([("file", LIST)] + REC, third_list(False), tmp_path)
    f, m = g.FilterChecklist(props), cm.Model(props)
    for n in (700, 3, 1500, 1, 64):
        ret, out = same(g, f, m, third_records(n))
        assert ret == g.MODIFIED and len(synth.unpack_all(out)) == n
    before = f.counters()
    assert same(g, f, m, rec(kv(("log", "nope")), 1) * 5 + rec(kv(("log", 7)), 2)) == (g.NOTOUCH, None)
    assert f.counters() == (before[0], 0, before[2] + 1, 0) and f.counts() == (6, 6)
    assert same(g, f, m, third_records(9))[0] == g.MODIFIED
    f.close()

"""filter_rewrite_tag on the device (csrc/rtag_kernels.inc through flbgpu_filter_rewrite_tag_create) against the recorded answers of
the real plugin (tests/golden/rtag_ref_cases.json) and against the CPU model (tests/rtag_model.py): return value, output bytes, the
emitted (tag, bytes) list, record counts and the filter's own counters.  Every comparison includes the size / emit mismatch counter,
which the model holds at 0.  The patterns come from fixed lists, so the regex corner counter stays 0."""
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
import recmod_model as rmm
import rtag_model as rm
from rtag_chunks import GROUP_END, GROUP_START, P1, P16, kv, mixed_records, rec
import oracle_binding as ob

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "rtag_ref_cases.json")))["cases"]


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def pair(g, props, tag=b"", refuse=None):
    """the device filter and the model with the same tag and the same emitter: refuse(index of the emission in the call) -> bool"""
    f, m = g.FilterRewriteTag(props, tag), rm.Model(props, tag, (lambda i, t, b: refuse(i)) if refuse else None)
    f.calls = []
    if refuse:
        def emitter(t, b):
            f.calls.append((t, b))
            return -1 if refuse(len(f.calls) - 1) else 0
        f.set_emitter(emitter)
    return f, m


def same(g, f, m, data):
    del f.calls[:]
    before = f.counters()
    got = f.filter(data)
    want = m.filter(data)
    assert got == want, (got[0], want[0])
    assert f.emitted() == m.emitted
    assert f.counts() == m.counts()
    assert f.counters() == m.counters() and f.counters()[2] == 0
    assert f.counters()[0] - before[0] == len(m.emitted)
    assert f.regex_corners() == 0
    return got


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused"):
        with pytest.raises(ValueError):
            g.FilterRewriteTag(props)
        return
    data, tag = base64.b64decode(case["in"]), base64.b64decode(case["tag"])
    f, m = pair(g, props, tag, (lambda i: i in case["refuse"]) if case["refuse"] else None)
    try:
        ret, out = same(g, f, m, data)
        # the real plugin's answer directly
        em = [(base64.b64decode(t), base64.b64decode(b), r) for t, b, r in case["emitter"]]
        assert ret == case["ret"] and out == (base64.b64decode(case["out"]) if case["out"] is not None else None)
        assert f.emitted() == [(t, b) for t, b, r in em if not r]
        if case["refuse"]:
            assert f.calls == [(t, b) for t, b, r in em]                # the callback saw every emission, in record order
        assert f.counters()[:2] == (sum(1 for e in em if not e[2]), sum(1 for e in em if e[2]))
    finally:
        f.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_block_edges(g, n):
    data = mixed_records(n)
    for props in (P1, P16):
        f, m = pair(g, props, b"app.web.prod")
        ret, out = same(g, f, m, data)
        assert ret == g.MODIFIED and m.counts()[0] == n and len(m.emitted) >= 1 and (n < 9 or len(m.emitted) >= n // 5)
        f.close()


def test_none_matched_and_all_matched(g):
    data = b"".join(rec(kv(("log", "line %d" % i), ("n", i)), 100 + i) for i in range(257))
    f, m = pair(g, [("Rule", "$log ^never$ t false")], b"t")
    assert same(g, f, m, data) == (g.NOTOUCH, None) and f.counts() == (257, 257) and f.counters() == (0, 0, 0, 0)
    f.close()
    f, m = pair(g, [("Rule", "$log ^line t.$n false")], b"t")
    assert same(g, f, m, data) == (g.MODIFIED, b"") and f.counts() == (257, 0) and len(f.emitted()) == 257
    assert f.emitted()[256][0] == b"t.256"
    f.close()


def test_tag_lengths_in_one_call(g):
    tags = [b"", b"x", b"t" * 300, b"", b"yy", b"", b"z" * 300]
    data = b"".join(rec(kv(("log", "go"), ("t", t)), i) for i, t in enumerate(tags))
    f, m = pair(g, [("Rule", "$log ^go$ $t true")])
    ret, out = same(g, f, m, data)
    assert (ret, out) == (g.MODIFIED, data) and [t for t, _ in f.emitted()] == tags and f.counters()[3] == sum(len(t) for t in tags)
    f.close()


CAPTURES = [("Rule", "$log ^(\\S+)\\s+([^\\s!]+)(!)?\\s(.*)$ $2.$1|$3|$4|$0 false"), ("Rule", "$msg (?<a>\\d+)-(?<b>[a-zé]+) $TAG.$2.$1.$0 true")]


@pytest.mark.parametrize("force", ["", "1", "2"])
def test_capture_template_on_both_engines(g, force, monkeypatch):
    if force:
        monkeypatch.setenv("FLBGPU_RX_FORCE_NFA", force)
    vals = [("log", "GET index done in 5 ms"), ("log", "café crème € and more"), ("msg", "id 42-abc."), ("msg", "ça 7-été été"),
            ("log", "one two"), ("log", "x" * 70 + " y ! " + "z" * 200), ("msg", "nothing"), ("log", "späße ÿ! " + "ü" * 33), ("msg", "9-é")]
    data = b"".join(rec(kv((k, v), ("i", i)), i) for i, (k, v) in enumerate(vals * 15))
    f, m = pair(g, CAPTURES, b"cap")
    ret, out = same(g, f, m, data)
    assert ret == g.MODIFIED and len(m.emitted) == 15 * 7
    assert m.emitted[1][0] == "crème.café||€ and more|café crème € and more".encode() and m.emitted[3][0] == "cap.été.7.7-été".encode()
    f.close()


@pytest.mark.parametrize("which", ["first", "last", "every64th", "all"])
def test_refused_emissions(g, which):
    n = 300
    data = b"".join(rec(kv(("log", "m%d" % i if i % 3 else "x"), ("n", i)), i) for i in range(n))
    nem = sum(1 for i in range(n) if i % 3)
    refuse = {"first": lambda i: i == 0, "last": lambda i: i == nem - 1, "every64th": lambda i: i % 64 == 0, "all": lambda i: True}[which]
    for keep in ("false", "true"):
        f, m = pair(g, [("Rule", "$log ^m tag.$n %s" % keep)], b"t", refuse)
        ret, out = same(g, f, m, data)
        nref = sum(1 for i in range(nem) if refuse(i))
        assert len(f.calls) == nem and f.counters()[:2] == (nem - nref, nref)
        assert ret == (g.NOTOUCH if which == "all" else g.MODIFIED)
        if which != "all":
            assert f.counts() == (n, n if keep == "true" else n - nem + nref)
        f.close()


def test_chain_behind_grep_and_in_front_of_record_modifier(g):
    data = mixed_records(600)
    grep, rmod = [("exclude", "stream ^stdout$")], [("Record", "host h1")]
    props = [("Rule", "$log (?<what>error|fatal) $TAG.$1 false"), ("Rule", "$level ^warn$ w.$m['n'] true")]
    fg, fr, fm = g.FilterGrep(grep), g.FilterRewriteTag(props, b"chain"), g.FilterRecordModifier(rmod)
    seen = []
    fr.set_emitter(lambda t, b: seen.append((t, b)) or 0)
    chain = g.FilterChain([fg, fr, fm])
    ret, out = chain.filter(data)
    r1, o1 = ob.Grep(grep).filter(data)
    m = rm.Model(props, b"chain")
    r2, o2 = m.filter(o1)
    r3, o3 = rmm.Model(rmod).filter(o2)
    assert (r1, r2, r3) == (g.MODIFIED,) * 3 and (ret, out) == (g.MODIFIED, o3)
    assert fr.emitted() == m.emitted == seen and len(seen) >= 60
    assert fr.counts() == m.counts() and fr.counters() == m.counters() and fr.counters()[2] == 0
    # a second instance in the same chain keeps its own list
    fr2 = g.FilterRewriteTag([("Rule", "$host ^h1$ second false")], b"x")
    ret, out = g.FilterChain([fg, fr, fm, fr2]).filter(data)
    assert (ret, out) == (g.MODIFIED, b"") and fr.emitted() == m.emitted and [t for t, _ in fr2.emitted()] == [b"second"] * fr2.counts()[0]
    assert fr2.counts()[0] == m.counts()[1] and b"".join(b for _, b in fr2.emitted()) == o3
    for f in (fg, fr, fm, fr2):
        f.close()


def test_device_level_call_hands_device_pointers(g):
    recs = [rec(kv(("log", "m%d" % i if i % 2 else "x"), ("n", i)), i) for i in range(130)]
    recs.insert(3, GROUP_START)
    recs.insert(5, GROUP_END)
    blob = b"".join(recs)
    offs = [0]
    for rc in recs:
        offs.append(offs[-1] + len(rc))
    L = g.lib()
    d = L.flbgpu_dev_alloc(len(blob) + 16)
    L.flbgpu_memcpy_h2d(d, blob, len(blob))
    ro = struct.pack("<%dQ" % len(offs), *offs)
    d_off = L.flbgpu_dev_alloc(len(ro))
    L.flbgpu_memcpy_h2d(d_off, ro, len(ro))
    props = [("Rule", "$log ^m(\\d+)$ d.$1.$TAG[1] false")]
    refused_nothing = []
    f, m = g.FilterRewriteTag(props, b"dev.level"), rm.Model(props, b"dev.level")
    f.set_emitter(lambda t, b: refused_nothing.append(t) or -1)        # the device-level call asks nobody
    ret, out = f.filter_dev(g.DevChunk(d, d_off, len(offs) - 1, len(blob)))
    want = m.filter(blob)
    buf = ctypes.create_string_buffer(max(out.bytes, 1))
    L.flbgpu_memcpy_d2h(buf, out.data, out.bytes)
    assert (ret, buf.raw[:out.bytes]) == want and not refused_nothing
    count, d_recs, d_tags, tag_bytes = f.emitted_dev()
    assert count == len(m.emitted) == 65 and tag_bytes == sum(len(t) for t, _ in m.emitted)
    table = (g.RtagEmittedRec * count)()
    L.flbgpu_memcpy_d2h(table, d_recs, ctypes.sizeof(table))
    tags = ctypes.create_string_buffer(tag_bytes)
    L.flbgpu_memcpy_d2h(tags, d_tags, tag_bytes)
    got = [(tags.raw[r.tag_off:r.tag_off + r.tag_len], blob[r.in_off:r.in_off + r.len]) for r in table]
    assert got == m.emitted
    assert f.counts() == m.counts() and f.counters() == m.counters() and f.counters()[2] == 0
    f.close()
    L.flbgpu_dev_free(d)
    L.flbgpu_dev_free(d_off)


def test_buffer_reuse_and_counters_across_calls(g):
    f, m = pair(g, P16, b"a.b.c")
    for n in (700, 3, 1500, 1, 64):
        assert same(g, f, m, mixed_records(n))[0] in (g.MODIFIED, g.NOTOUCH)
    bad = rec("not a map", 1)
    assert same(g, f, m, mixed_records(10) + bad + mixed_records(5)) == (g.NOTOUCH, None)
    assert f.counts() == (10, 10) and len(f.emitted()) >= 3            # the emissions in front of the error stand
    assert same(g, f, m, bad + mixed_records(5)) == (g.NOTOUCH, None) and f.counts() == (0, 0) and f.emitted() == []
    assert same(g, f, m, mixed_records(9) + b"\xc1")[0] == g.NOTOUCH and len(f.emitted()) >= 3
    f.set_tag(b"other")
    m.tag = b"other"
    assert same(g, f, m, mixed_records(9))[0] == g.MODIFIED and any(t.startswith(b"other.") for t, _ in f.emitted())
    f.close()

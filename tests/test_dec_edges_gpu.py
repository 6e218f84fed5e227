"""Decode_Field / Decode_Field_As on the device (csrc/dec_dev.inc, k_parser_dec, the sizing in run_parser_dev) at its scratch, grid and
rule edges: the named cases of tests/dec_chunks.py (tests/test_dec_chunks.py proves on the CPU that each sits on its edge and that the
oracle's answers are the reference's), one test per group, return code and bytes against the oracle with no tolerance, the record counts
of the call, and -- through FilterParser.dec_launch(), the read-only view of the last call's decoder launch -- the lanes and the room per
scratch region the call really used.  Only grid/second_trip/default allocates in the GB range (the default scratch budget)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import oracle_binding as ob
import dec_chunks as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def first_diff(a, b):
    a, b = a or b"", b or b""
    n = min(len(a), len(b))
    i = next((k for k in range(n) if a[k] != b[k]), n)
    return i, len(a), len(b), a[max(0, i - 40):i + 40], b[max(0, i - 40):i + 40]


def _no_fault(g, ret, what):
    """a device fault ends the session (nothing more is started on a faulted device)"""
    err = g.last_error()
    if ret != g.MODIFIED and ("illegal memory access" in err or "hardware exception" in err or "unspecified launch failure" in err):
        pytest.exit("device fault in %r: %s" % (what, err), returncode=3)


def ids(group):
    return [c.name for c in dc.cases(group)]


def run(g, c, monkeypatch):
    """the case through FilterParser.filter: (the decoder launch, the filter's counts) after the bytes and the return code were compared"""
    monkeypatch.delenv("FLBGPU_DEC_BUDGET_MB", raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    gps = [g.Parser(**p) for p in c.parsers]
    f = g.FilterParser(c.key, gps, c.reserve, c.preserve)
    try:
        ret, out = f.filter(c.data)
        _no_fault(g, ret, c.name)
        wret, wout = c.want()
        assert ret == wret, (c.name, ret, wret, g.last_error())
        assert out == wout, (c.name, first_diff(wout, out))
        assert f.counts() == (ob.count_records(c.data), ob.count_records(wout or b"")), (c.name, f.counts())
        return f.dec_launch()
    finally:
        f.close()
        for p in gps:
            p.close()


def case(group, name):
    return next(c for c in dc.cases(group) if c.name == name)


@pytest.mark.parametrize("name", ids("scratch"))
def test_scratch(g, monkeypatch, name):
    """MODIFIED with the reference's bytes on both sides of the first room; the room in use holds the largest decoded map, and was grown
    exactly where three times the record plus 4 KB do not hold it"""
    c = case("scratch", name)
    dl = run(g, c, monkeypatch)
    print(name, dl, "largest map", c.largest_map(), "first room", c.first_room())
    assert dl["cap"] >= c.largest_map() and dl["rows"] >= 1
    if c.notes["past"]:
        assert dl["passes"] >= 2 and dl["overflow"] >= 1 and dl["cap"] > c.first_room()
    else:
        assert dl["passes"] == 1 and dl["overflow"] == 0


@pytest.mark.parametrize("name", ids("grid"))
def test_grid(g, monkeypatch, name):
    c = case("grid", name)
    dl = run(g, c, monkeypatch)
    n = len(c.recs)
    print(name, dl, "rows", n)
    assert dl["rows"] == n and dl["overflow"] == 0 and dl["lanes"] % 64 == 0
    if c.notes.get("trip"):
        assert dl["lanes"] < n                                            # some lane takes a second row
        if not c.env:
            assert (1 << 30) < dl["lanes"] * 6 * dl["cap"] <= (1 << 31)    # the default budget, halved into
    else:
        assert n <= dl["lanes"] < n + 64


@pytest.mark.parametrize("name", ids("widths"))
def test_header_widths(g, monkeypatch, name):
    run(g, case("widths", name), monkeypatch)


@pytest.mark.parametrize("name", ids("rules"))
def test_rule_bookkeeping(g, monkeypatch, name):
    run(g, case("rules", name), monkeypatch)


def test_one_key_or_rule_too_many_is_refused_at_create(g):
    for name, msg in (("rules/max_keys", "more than %d keys with decoders" % dc.MAX_DEC_KEYS), ("rules/max_rules", "more than %d decoder rules for one key" % dc.MAX_DEC_RULES)):
        c = case("rules", name)
        with pytest.raises(ValueError) as e:
            g.Parser(**dict(c.parsers[0], decoders=c.notes["over"]))
        assert msg in str(e.value)


@pytest.mark.parametrize("name", ids("time"))
def test_format_json_time_in_the_decoded_map(g, monkeypatch, name):
    c = case("time", name)
    dl = run(g, c, monkeypatch)
    assert dl["rows"] == len(c.recs) and len(c.out_records()) == len(c.recs) - 1      # the refused time: sized, not written, not counted


@pytest.mark.parametrize("name", ids("record"))
def test_around_the_record(g, monkeypatch, name):
    run(g, case("record", name), monkeypatch)


def _from_device(g, o):
    buf = ctypes.create_string_buffer(max(int(o.bytes), 1))
    if o.bytes:
        g.lib().flbgpu_memcpy_d2h(buf, o.data, int(o.bytes))
    return buf.raw[:int(o.bytes)]


def test_call_paths(g, monkeypatch):
    """the same chunk through FilterParser.filter, filter_dev and a [parser with decoders, grep] chain (which must take the unfused
    kernels: the fused pair has no decoders)"""
    c = case("paths", "paths/mixed")
    run(g, c, monkeypatch)
    wret, wout = c.want()
    n = len(c.recs)
    L = g.lib()
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(r) for r in c.recs), dtype=np.uint64, count=n), out=off[1:])
    d_data, d_off = L.flbgpu_dev_alloc(len(c.data) + 16), L.flbgpu_dev_alloc(off.nbytes)
    assert d_data and d_off, g.last_error()
    gps = [g.Parser(**p) for p in c.parsers]
    fp, fg = g.FilterParser(c.key, gps), g.FilterGrep(dc.GREP)
    try:
        L.flbgpu_memcpy_h2d(d_data, c.data, len(c.data)); L.flbgpu_memcpy_h2d(d_off, off.ctypes.data, off.nbytes)
        chunk = g.DevChunk(d_data, d_off, n, len(c.data))
        ret, o = fp.filter_dev(chunk)
        _no_fault(g, ret, "filter_dev")
        got = _from_device(g, o)
        assert (ret, int(o.n)) == (wret, n) and got == wout, first_diff(wout, got)
        assert fp.counts() == (n, ob.count_records(wout)) and fp.dec_launch()["rows"] == (n + 2) // 3
        goff = np.zeros(n + 1, dtype=np.uint64)
        L.flbgpu_memcpy_d2h(goff.ctypes.data, o.row_off, goff.nbytes)
        assert [int(x) for x in goff] == [s for s, _, _ in c.out_records()] + [len(wout)]
        # the chain
        gret, gout = ob.Grep(dc.GREP).filter(wout)
        kept = ob.count_records(gout)
        stats = [dict(ret=wret, in_records=n, out_records=n, out_bytes=len(wout)), dict(ret=gret, in_records=n, out_records=kept, out_bytes=len(gout))]
        chain = g.FilterChain([fp, fg])
        fp.profile(True)
        ret, out = chain.filter(c.data)
        prof = fp.profile_read()
        _no_fault(g, ret, "chain")
        assert (ret, out) == (gret, gout), first_diff(gout, out)
        assert chain.last_stats() == stats
        assert "k_parser_dec_size" in prof and "k_parser_dec_emit" in prof and "k_parser_emit" in prof and not any(k.startswith("k_pg_") for k in prof), sorted(prof)
        ret, o = chain.filter_dev(chunk)
        _no_fault(g, ret, "chain, device")
        got = _from_device(g, o)
        assert ret == gret and got == gout, first_diff(gout, got)
        assert chain.last_stats() == stats
    finally:
        fg.close(); fp.close()
        for p in gps:
            p.close()
        L.flbgpu_dev_free(d_data); L.flbgpu_dev_free(d_off)

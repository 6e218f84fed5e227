"""The msgpack -> JSON formatter on the device (csrc/kernels_fmt.hip k_fmt_size / k_fmt_groups / k_fmt_emit, fmt_dev.inc, packfmt.cpp,
numconv.hpp fmt_g16) on the named chunks of tests/fmt_chunks.py: the staging area of k_fmt_emit at exact fit, one byte over and on the
direct path at every alignment, split batches, rows that print nothing, the flush's 16-byte seams, string tails at the chunk's end, the
second trip of both grid-stride loops, the tile seams and carried values of k_fmt_groups, the 1000-skipped-rows guard, the order in which
a refused row, a NULL row and the skip limit end the walk, and a value per row for floats, dates and strings.  Every expected byte, NULL
result, row offset and count is the CPU oracle's; tests/test_fmt_chunks.py asserts on the CPU that each chunk sits on its edge.
Each chunk runs through the one-shot call, a reused JsonFormatter and JsonFormatter.format_dev on an uploaded chunk (with its row offsets
and without), and the profile says whether the group pass ran."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import fmt_chunks as fc
import test_fmt_chunks as tfc
from fmt_chunks import JSON, LINES

pytestmark = pytest.mark.gpu
FAULTS = ("illegal memory access", "hardware exception", "unspecified launch failure")


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


class Formatters(dict):
    """one JsonFormatter per configuration, reused across the chunks of a test"""

    def __init__(self, g):
        super().__init__()
        self.g = g

    def get(self, cfg):
        key = tuple(sorted((k, v) for k, v in cfg.items()))
        if key not in self:
            self[key] = self.g.JsonFormatter(cfg["json_format"], cfg["date_format"], cfg["date_key"], cfg["escape_unicode"], cfg["nan_to_null"])
        return self[key]

    def close(self):
        for f in self.values():
            f.close()
        self.clear()


def first_diff(a, b):
    if a is None or b is None:
        return "%s / %s" % ("NULL" if a is None else "%d bytes" % len(a), "NULL" if b is None else "%d bytes" % len(b))
    n = min(len(a), len(b))
    x, y = np.frombuffer(a, dtype=np.uint8, count=n), np.frombuffer(b, dtype=np.uint8, count=n)
    d = np.flatnonzero(x != y)
    i = int(d[0]) if len(d) else n
    return "first difference at byte %d of %d / %d: %r / %r" % (i, len(a), len(b), a[max(i - 24, 0):i + 24], b[max(i - 24, 0):i + 24])


def _call(fn, what):
    """a device fault ends the session (nothing more is started on a faulted device)"""
    try:
        return fn()
    except RuntimeError as e:
        if any(w in str(e) for w in FAULTS):
            pytest.exit("device fault in %r: %s" % (what, e), returncode=3)
        raise


def _profile_ok(c, prof, what, indexed):
    """indexed: the call found the rows itself (a host chunk, a device chunk without row offsets), so it saw none behind a refused row"""
    e = c.expect()
    groups = e["groups_indexed"] if indexed else e["groups"]
    want = 2 if groups else 1
    assert ("k_fmt_groups" in prof) == groups and prof["k_fmt_size"][1] == want, (c.name, what, {k: v[1] for k, v in prof.items()})
    assert ("k_fmt_emit" in prof) == (e["out"] is not None and e["n"] > 0 and int(e["row_off"][-1]) > 0), (c.name, what, sorted(prof))


def run_dev(g, f, c, with_off):
    e = c.expect()
    L = g.lib()
    what = (c.name, "device", "row offsets" if with_off else "no row offsets")
    off = c.in_off()
    d_data = L.flbgpu_dev_alloc(len(c.blob) + 16)
    d_off = L.flbgpu_dev_alloc(off.nbytes) if with_off else None
    assert d_data and (d_off or not with_off), g.last_error()
    try:
        L.flbgpu_memcpy_h2d(d_data, c.blob, len(c.blob))
        if with_off:
            L.flbgpu_memcpy_h2d(d_off, off.ctypes.data, off.nbytes)
        f.profile(True)
        rc, o = _call(lambda: f.format_dev(g.DevChunk(d_data, d_off, c.n if with_off else 0, len(c.blob))), what)
        prof = f.profile_read()
        assert g.last_error() == "", (what, g.last_error())
        if e["out"] is None:
            assert rc == -1, what
        else:
            want = e["out"]
            assert rc == 0 and int(o.bytes) == len(want) and int(o.n) == e["n"], (what, rc, int(o.bytes), len(want), int(o.n), e["n"])
            got = ctypes.create_string_buffer(len(want))
            L.flbgpu_memcpy_d2h(got, o.data, len(want))
            assert got.raw == want, (what, first_diff(got.raw, want))
            if e["n"] > 0:
                goff = np.zeros(e["n"] + 1, dtype=np.uint64)
                L.flbgpu_memcpy_d2h(goff.ctypes.data, o.row_off, goff.nbytes)
                assert np.array_equal(goff, e["row_off"]), (what, "row offsets", int(np.argmax(goff != e["row_off"])))
                if c.cfg["json_format"] == JSON:
                    assert want[-1:] == b"]" and int(goff[-1]) == len(want) - 1, what
        _profile_ok(c, prof, what, not with_off)
    finally:
        L.flbgpu_dev_free(d_data)
        if d_off:
            L.flbgpu_dev_free(d_off)


def run_chunk(g, F, c):
    """the chunk through the one-shot call, the reused formatter's host call and its device call"""
    e, cfg = c.expect(), c.cfg
    want = e["out"]
    got = g.msgpack_to_json_format(c.blob, cfg["json_format"], cfg["date_format"], cfg["date_key"], cfg["escape_unicode"], cfg["nan_to_null"])
    err = g.last_error()
    if any(w in err for w in FAULTS):
        pytest.exit("device fault in %r: %s" % (c.name, err), returncode=3)
    assert got == want, (c.name, "one-shot", first_diff(got, want), err)
    assert err == "", (c.name, "one-shot", err)
    f = F.get(cfg)
    f.profile(True)
    got = _call(lambda: f.format(c.blob), (c.name, "host"))         # (raises where a NULL comes with a message)
    prof = f.profile_read()
    assert got == want, (c.name, "host", first_diff(got, want))
    assert g.last_error() == "", (c.name, "host", g.last_error())
    _profile_ok(c, prof, "host", True)
    run_dev(g, f, c, True)
    run_dev(g, f, c, False)


def run_family(g, name, pick=lambda c: True):
    F = Formatters(g)
    cs = [c for c in tfc.chunks(name) if pick(c)]
    assert cs
    for c in cs:
        run_chunk(g, F, c)
    F.close()


# ------------------------------------------------------------------------------------------ (a) staging and batches
@pytest.mark.parametrize("fmt", fc.ALL_FMT)
def test_stg_edge(g, fmt):
    run_family(g, "stg_edge", lambda c: c.cfg["json_format"] == fmt)


@pytest.mark.parametrize("esc", (1, 0))
def test_direct_rows(g, esc):
    run_family(g, "direct_rows", lambda c: c.cfg["escape_unicode"] == esc)


def test_batch_split(g):
    run_family(g, "batch_split")


def test_zero_rows(g):
    run_family(g, "zero_rows")


def test_tail_waves(g):
    run_family(g, "tail_waves")


def test_flush_seams(g):
    run_family(g, "flush_seams")


@pytest.mark.parametrize("esc", (1, 0))
def test_str_tails(g, esc):
    run_family(g, "str_tails", lambda c: c.cfg["escape_unicode"] == esc)


# ------------------------------------------------------------------------------------------ (b) the grid
def _cus(g):
    cus = int(g.lib().flbgpu_device_cus())
    return cus if cus > 0 else 256


_grid = {}


def emit_chunk(g):
    if "emit" not in _grid:
        _grid["emit"] = fc.emit_second_trip(_cus(g))
    return _grid["emit"]


def test_emit_second_trip(g):
    c = emit_chunk(g)
    assert c.n == _cus(g) * 8 * 256 + 64 * 3 + 5
    F = Formatters(g)
    run_chunk(g, F, c)
    F.close()


def test_size_second_trip(g):
    c = fc.size_second_trip(_cus(g))
    assert c.n == _cus(g) * 32 * 256 + 64 + 3
    F = Formatters(g)
    run_chunk(g, F, c)
    F.close()


# ------------------------------------------------------------------------------------------ (c) groups and the skip guard
def test_group_edges(g):
    run_family(g, "group_edges")


def test_skip_runs(g):
    run_family(g, "skip_runs")


def test_walk_order(g):
    run_family(g, "walk_order")


# ------------------------------------------------------------------------------------------ (d) values
@pytest.mark.parametrize("which", ("floats/64/0", "floats/64/1", "floats/32/0", "floats/32/1"))
def test_floats(g, which):
    run_family(g, "floats", lambda c: c.name == which)


@pytest.mark.parametrize("df", range(5))
def test_dates(g, df):
    run_family(g, "dates", lambda c: c.cfg["date_format"] == df)


@pytest.mark.parametrize("which", ("pairs", "seam", "sampled"))
def test_strings(g, which):
    run_family(g, "strings", lambda c: c.name.split("/")[1] == which)


# ------------------------------------------------------------------------------------------ object reuse
def test_object_reuse(g):
    """one formatter over a chunk of the emit pass's second trip, then 63 rows, groups, a chunk without markers, an empty chunk and
    oversized rows: stale group rows, slow words, offsets and counters of an earlier call would show in a later one"""
    cfg = fc.CFG(LINES)
    f = g.JsonFormatter(LINES, cfg["date_format"], cfg["date_key"], 1, 0)
    pick = lambda name, k: [c for c in tfc.chunks(name) if c.cfg == cfg][k]
    seq = [emit_chunk(g), pick("tail_waves", 1), pick("group_edges", 0), pick("plain", 0), None, pick("direct_rows", 0), pick("group_edges", 1),
           pick("skip_runs", 0), pick("plain", 0)]
    for c in seq:
        if c is None:
            f.profile(True)
            assert _call(lambda: f.format(b""), "empty") is None and g.last_error() == "" and f.profile_read() == {}
            continue
        f.profile(True)
        got = _call(lambda: f.format(c.blob), c.name)
        prof = f.profile_read()
        assert got == c.expect()["out"], (c.name, first_diff(got, c.expect()["out"]))
        _profile_ok(c, prof, "reuse", True)
        run_dev(g, f, c, True)
    f.close()

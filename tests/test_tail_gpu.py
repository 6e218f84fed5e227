"""in_tail's line packing on the device (csrc/tail_kernels.inc through flbgpu_tail_run / flbgpu_tail_run_dev) against the oracle
(oracle/oflb.c oflb_tail_process) and against the plain Python restatement (tests/tail_model.py), on the named texts of
tests/tail_chunks.py: the staging area of k_tl_emit, the second trip of the grid-stride loops, the 64-byte and 16 KB edges of the
mask pass, every byte value next to a newline, leading NULs, and msgpack's header sizes.  tests/test_tail_lines.py asserts on the
CPU that each text reaches its edge, that the model equals the oracle and the oracle the reference's real encoder.
The device chunk is read row by row: one row per newline, empty where the reference skips the line."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import oracle_binding as ob
import tail_chunks as tc
import tail_model as tm

pytestmark = pytest.mark.gpu
TS = dict(sec=1700000000, nsec=5)


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def tail_of(g, c):
    return g.TailLines(**{k: v for k, v in c.items() if k != "stream_offset"})


class Uploaded:
    """a text in device memory, `shift` bytes into its allocation"""

    def __init__(self, g, text, shift=0):
        self.L, self.n = g.lib(), len(text)
        self.base = self.L.flbgpu_dev_alloc(len(text) + 32)
        assert self.base, g.last_error()
        self.ptr = self.base + shift
        if text:
            self.L.flbgpu_memcpy_h2d(self.ptr, text, len(text))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.L.flbgpu_dev_free(self.base)


def download(g, chunk):
    """-> (row offsets as a list of n + 1 ints, the chunk's bytes)"""
    L, n, nb = g.lib(), int(chunk.n), int(chunk.bytes)
    if n == 0:
        assert nb == 0
        return [0], b""
    off = np.zeros(n + 1, dtype=np.uint64)
    L.flbgpu_memcpy_d2h(off.ctypes.data, chunk.row_off, off.nbytes)
    buf = ctypes.create_string_buffer(nb) if nb else None
    if nb:
        L.flbgpu_memcpy_d2h(buf, chunk.data, nb)
    return off, (buf.raw if nb else b"")


def check_dev(g, t, up, c, rows, processed, what):
    """process_dev on an uploaded text against the model's rows"""
    lines, chunk, proc = t.process_dev(up.ptr, up.n, stream_offset=c.get("stream_offset", 0), **TS)
    off, data = download(g, chunk)
    assert (lines, proc, int(chunk.n)) == (sum(1 for r in rows if r), processed, len(rows)), what
    want_off = np.concatenate(([0], np.cumsum([len(r) for r in rows], dtype=np.uint64))) if rows else [0]
    assert int(off[0]) == 0 and int(off[-1]) == int(chunk.bytes) == len(data), what
    if data != b"".join(rows) or not np.array_equal(np.asarray(off, dtype=np.uint64), np.asarray(want_off, dtype=np.uint64)):
        for i, r in enumerate(rows):                      # the first row that differs, only on failure
            got = data[int(off[i]):int(off[i + 1])]
            assert got == r, (what, "row %d of %d" % (i, len(rows)), len(got), len(r), got[:48], r[:48], got[-24:], r[-24:])
        assert False, (what, "row table")
    return data


@pytest.mark.parametrize("group", [n for n in tc.GROUPS if n != "many_lines"])
def test_named_texts(g, group):
    tails = {}
    try:
        for label, text, cfgs in tc.group(group):
            with Uploaded(g, text) as up:
                for c in cfgs:
                    key = tuple(sorted((k, v) for k, v in c.items() if k != "stream_offset"))
                    t = tails.get(key) or tails.setdefault(key, tail_of(g, c))
                    what = (group, label, c)
                    want = ob.tail_process(text, **TS, **c)
                    got = t.process(text, stream_offset=c.get("stream_offset", 0), **TS)
                    assert (got[0], got[2]) == (want[0], want[2]), what
                    assert got[1] == want[1], what
                    rows, processed = tm.records(text, **TS, **c)
                    assert check_dev(g, t, up, c, rows, processed, what) == want[1], what
    finally:
        for t in tails.values():
            t.close()


def test_unaligned_text_pointer(g):
    """a text pointer that is not 16-byte aligned takes the byte loop of k_tl_count, and the copies start at any address"""
    for c in (tc.D, tc.NOSKIP):
        t = tail_of(g, c)
        try:
            for grp in ("neighbours", "edges"):
                for label, text, _ in tc.group(grp):
                    rows, processed = tm.records(text, **TS, **c)
                    with Uploaded(g, text) as up:
                        aligned = check_dev(g, t, up, c, rows, processed, (grp, label, c, 0))
                    for k in (1, 4, 15):
                        with Uploaded(g, text, k) as up:
                            assert check_dev(g, t, up, c, rows, processed, (grp, label, c, k)) == aligned
        finally:
            t.close()


def test_many_lines(g):
    """more lines than one trip of k_tl_size's and k_tl_emit's grid-stride loops covers on this device; the offset key passes 2^32
    inside the text"""
    (_, text, cfgs), = tc.group("many_lines")
    cus = g.lib().flbgpu_device_cus()
    nl = text.count(b"\n")
    assert cus > 0 and tm.second_trips(nl, cus) == (True, True), (nl, cus)
    assert nl > tm.SIZE_BLOCKS * 256 and nl > cus * tm.EMIT_BLOCKS_PER_CU * 256
    with Uploaded(g, text) as up:
        for c in cfgs:
            t = tail_of(g, c)
            try:
                want = ob.tail_process(text, **TS, **c)
                got = t.process(text, stream_offset=c.get("stream_offset", 0), **TS)
                assert (got[0], got[2]) == (want[0], want[2]) and got[1] == want[1], c
                if c is cfgs[-1]:
                    rows, processed = tm.records(text, **TS, **c)
                    assert check_dev(g, t, up, c, rows, processed, ("many lines", c)) == want[1]
            finally:
                t.close()


def test_object_reuse(g):
    """one object from a large text to small ones and back: masks, positions and sizes of the earlier call stay in its buffers"""
    many = tc.group("many_lines")[0][1]
    staging = tc.group("staging")[0][1]
    skipped = b"\n\r\n" * 5000
    t = g.TailLines()
    try:
        for text in (many, b"a\nb", skipped, b"\0" * 100, b"", staging, b"a\nb"):
            want = ob.tail_process(text, **TS)
            got = t.process(text, **TS)
            assert (got[0], got[2]) == (want[0], want[2]) and got[1] == want[1], (len(text), got[0], want[0], got[2], want[2])
            if text is skipped:
                assert got == (0, b"", 15000)
        with Uploaded(g, skipped) as up:            # every line skipped: 15000 / 3 * 2 rows, all empty
            lines, chunk, proc = t.process_dev(up.ptr, up.n, **TS)
            off, data = download(g, chunk)
            assert (lines, proc, int(chunk.n), int(chunk.bytes), data) == (0, 15000, 10000, 0, b"") and not np.any(off)
    finally:
        t.close()


def test_create_limits(g):
    text = b"hello\nworld\r\n"
    for c in (tc.K1, tc.K2, tc.K3):
        t = tail_of(g, c)
        assert t.process(text, stream_offset=c["stream_offset"], **TS) == ob.tail_process(text, **TS, **c)
        t.close()
    long = "x" * 256
    for kw in (dict(key=long), dict(path_key=long, path="p"), dict(path_key="k", path=long), dict(offset_key=long),
               dict(key="a" * 255, path_key="b" * 255, path="c" * 255, offset_key="d" * 255)):      # 4 * 257 bytes > pre[1024]
        with pytest.raises(ValueError):
            g.TailLines(**kw)
        assert "in_tail" in g.last_error()


def test_lines_feed_the_chain_across_trips(g):
    """the row table at a size where both grid-stride loops wrap, empty rows included, is what the filters take: filter_grep keeps
    the CR LF lines of the many-lines text"""
    text = tc.group("many_lines")[0][1]
    L = g.lib()
    t = g.TailLines()
    try:
        with Uploaded(g, text) as up:
            lines, chunk, processed = t.process_dev(up.ptr, up.n, **TS)
            fg = g.FilterGrep([tc.CRLF_RULE])
            r, o = g.FilterChain([fg]).filter_dev(chunk)
            host = ctypes.create_string_buffer(int(o.bytes))
            L.flbgpu_memcpy_d2h(host, ctypes.c_void_p(o.data), int(o.bytes))
        n, ev, _ = ob.tail_process(text, **TS)
        ret, want = ob.Grep([tc.CRLF_RULE]).filter(ev)
        assert (lines, processed) == (n, len(text)) and r == ret == g.MODIFIED
        assert ob.count_records(want) == text.count(b"ab\r\n") > 180000
        assert host.raw == want
    finally:
        t.close()

"""The stream processor's aggregation kernels (csrc/sp_kernels.inc, csrc/sp_select.inc, the host half csrc/sp.cpp) at their staging, key,
multiplicity, dictionary, value and grid edges: the named cases of tests/sp_chunks.py (tests/test_sp_chunks.py proves on the CPU that each
sits on its edge and that the oracle's answers are the reference's), one test per group.  The record count and the bytes of every do /
do_dev and of the timer against the oracle with no tolerance (the one-ULP allowance of tests/test_sp_gpu.py is not used here: the
float sums of these cases are exact in binary64 in every partial sum); where the oracle refuses (the reference's answer depends on
arrival order) the device raises at the same step and says so.  StreamTask.stats() -- the read-only view of the dictionary and of the
last call -- proves the paths that have a counter: dictionary growths, rows redone by k_sp_generic, the first row that does not decode,
the CU count the grids were sized by.  Only the grid group allocates more than a few MB."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import sp_chunks as sc
import sp_synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    L = m.lib()
    L.flbgpu_dev_alloc.restype = ctypes.c_void_p
    L.flbgpu_dev_alloc.argtypes = [ctypes.c_size_t]
    L.flbgpu_dev_free.argtypes = [ctypes.c_void_p]
    L.flbgpu_memcpy_h2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.flbgpu_memcpy_d2h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return m


def first_diff(a, b):
    n = min(len(a), len(b))
    i = next((k for k in range(n) if a[k] != b[k]), n)
    return i, len(a), len(b), a[max(0, i - 40):i + 40], b[max(0, i - 40):i + 40]


def _no_fault(g, what):
    """a device fault ends the session (nothing more is started on a faulted device)"""
    err = g.last_error()
    if "illegal memory access" in err or "hardware exception" in err or "unspecified launch failure" in err:
        pytest.exit("device fault in %r: %s" % (what, err), returncode=3)


class OnDevice:
    """a sp_chunks.Dev resident in HBM"""

    def __init__(self, g, d):
        self.L = g.lib()
        off = np.asarray(d.off, dtype=np.uint64)
        self.d_data, self.d_off = self.L.flbgpu_dev_alloc(len(d.data) + 16), self.L.flbgpu_dev_alloc(off.nbytes)
        assert self.d_data and self.d_off, g.last_error()
        if d.data:
            self.L.flbgpu_memcpy_h2d(self.d_data, d.data, len(d.data))
        self.L.flbgpu_memcpy_h2d(self.d_off, off.ctypes.data, off.nbytes)
        self.chunk = g.DevChunk(self.d_data, self.d_off, len(d.rows), len(d.data))

    def free(self):
        self.L.flbgpu_dev_free(self.d_data); self.L.flbgpu_dev_free(self.d_off)


def run(g, c, monkeypatch):
    """the case's steps on the device, each against the oracle's; -> StreamTask.stats() after every do / do_dev"""
    for k in ("FLBGPU_L2M_INIT_CAP", "FLBGPU_L2M_INIT_ARENA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)                                          # (read at flbgpu_sp_create)
    want = c.want()
    t = g.StreamTask(c.sql, str_conv=c.str_conv, tag="t")
    held, stats = [], []
    try:
        for i, s in enumerate(c.steps):
            w = want[i]
            try:
                if s is sc.TIMER:
                    got = t.timer()
                elif isinstance(s, sc.Dev):
                    held.append(OnDevice(g, s))
                    got = t.do_dev(held[-1].chunk)
                else:
                    got = t.do(s)
            except RuntimeError as e:
                _no_fault(g, c.name)
                assert w == sc.REFUSED, (c.name, i, str(e))
                assert "depends on arrival order" in str(e), (c.name, str(e))
                break
            assert w != sc.REFUSED, (c.name, i, "the device answered what depends on arrival order in the reference", got)
            if s is sc.TIMER:
                assert got == w, (c.name, i, first_diff(w, got))
            else:
                assert got[0] == w[0], (c.name, i, got[0], w[0])
                assert got[1] == w[1], (c.name, i, first_diff(w[1], got[1]))
                stats.append(t.stats())
        return stats
    finally:
        t.close()
        for h in held:
            h.free()


def ids(group):
    return [c.name for c in sc.cases(group)]


def case(group, name):
    return next(c for c in sc.cases(group) if c.name == name)


@pytest.mark.parametrize("name", ids("staging"))
def test_staging(g, monkeypatch, name):
    c = case("staging", name)
    (st,) = run(g, c, monkeypatch)
    rows = sum(1 for r in c.steps[0].rows if r)
    assert st["first_bad"] is None and st["attempts"] == 1 and st["rows_in"] == rows
    if c.notes["deferred"]:
        assert st["deferred"] == sum(1 for i, r in enumerate(c.steps[0].rows) if r and sc.dec_row(i)) > 0       # those left the tile for k_sp_generic
    else:
        assert st["deferred"] == 0


@pytest.mark.parametrize("name", ids("keys"))
def test_keys(g, monkeypatch, name):
    c = case("keys", name)
    run(g, c, monkeypatch)
    if "over" in c.notes:
        with pytest.raises(ValueError):                                    # one past the limit: refused at create, never answered
            g.StreamTask(c.notes["over"])


@pytest.mark.parametrize("name", ids("multiplicity"))
def test_multiplicity(g, monkeypatch, name):
    run(g, case("multiplicity", name), monkeypatch)


@pytest.mark.parametrize("name", ids("dictionary"))
def test_dictionary(g, monkeypatch, name):
    c = case("dictionary", name)
    stats = run(g, c, monkeypatch)
    assert len(stats) == len(c.notes["grows"])
    for st, (lo, hi) in zip(stats, c.notes["grows"]):
        assert lo <= st["grows"] and (hi is None or st["grows"] <= hi), (name, st)
        assert st["slots"] >= 2 * st["groups"]
    assert stats[-1]["attempts"] >= 1
    if "first_bad" in c.notes:
        assert stats[0]["first_bad"] == c.notes["first_bad"] and stats[0]["rows_in"] == c.notes["first_bad"] and stats[1]["first_bad"] is None
    else:
        assert all(st["first_bad"] is None for st in stats)
        assert all(st["attempts"] == 1 + st["grows"] - (stats[i - 1]["grows"] if i else 0) for i, st in enumerate(stats))


@pytest.mark.parametrize("name", ids("values"))
def test_values(g, monkeypatch, name):
    c = case("values", name)
    stats = run(g, c, monkeypatch)
    if c.notes.get("deferred"):
        assert stats[0]["deferred"] > 0


_GRID = {}


def _grid(g):
    cus = int(g.lib().flbgpu_device_cus())
    assert cus > 0
    if cus not in _GRID:
        _GRID[cus] = sc.grid_cases(cus)
    return cus, _GRID[cus]


@pytest.mark.parametrize("name", sc.GRID_NAMES)
def test_grid(g, monkeypatch, name):
    cus, cs = _grid(g)
    c = next(x for x in cs if x.name == name)
    c.check()                                                              # the predicate again, for this device's CU count
    (st,) = run(g, c, monkeypatch)
    assert st["cus"] == cus and st["first_bad"] is None
    if c.notes.get("deferred"):
        assert st["deferred"] == 2
        assert len(c.steps[0].rows) > 2 * st["cus"] * sc.SP_BLOCK


def test_select_second_trip(g):
    """k_sp_select's grid-stride loop: 4096 x 256 rows + 300 (BASELINE configs[4]'s record shape, device resident).  Head and tail against
    the oracle, the whole through the properties tests/test_sp_gpu.py::test_select_at_size_device_resident uses"""
    import osp
    n = sc.SELECT_GRID[0] * sc.SELECT_GRID[1] + 300
    data, off = sp_synth.config4_chunk(n)
    q = "SELECT status, host AS h, latency FROM STREAM:x WHERE status >= 400;"
    L = g.lib()
    d_d, d_o = L.flbgpu_dev_alloc(data.nbytes + 16), L.flbgpu_dev_alloc(off.nbytes)
    assert d_d and d_o
    t = g.StreamTask(q)
    try:
        L.flbgpu_memcpy_h2d(d_d, data.ctypes.data, data.nbytes); L.flbgpu_memcpy_h2d(d_o, off.ctypes.data, off.nbytes)
        try:
            ret, out = t.do_dev(g.DevChunk(d_d, d_o, n, data.nbytes))
        except RuntimeError:
            _no_fault(g, "select")
            raise
        raw = data.reshape(n, -1)
        RL = raw.shape[1]
        st = raw[:, 22].astype(np.uint32) * 256 + raw[:, 23]
        keep = st >= 400
        assert ret == int(keep.sum()) == t.stats()["rows_in"] and t.stats()["first_bad"] is None
        one = len(osp.Task(q).do(raw[int(np.nonzero(keep)[0][0])].tobytes())[1])
        assert len(out) == ret * one
        head = 4000
        want = osp.Task(q).do(data[:RL * head].tobytes())
        assert out[:len(want[1])] == want[1] and want[0] == int(keep[:head].sum())
        tail = 600                                                         # the 300 rows of the second trip and the 300 before them
        want = osp.Task(q).do(data[RL * (n - tail):].tobytes())
        assert want[0] == int(keep[n - tail:].sum()) > 0 and int(keep[n - 300:].sum()) > 0 and out[len(out) - len(want[1]):] == want[1]
    finally:
        t.close()
        L.flbgpu_dev_free(d_d); L.flbgpu_dev_free(d_o)

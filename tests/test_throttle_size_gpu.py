"""filter_throttle_size on the device (csrc/throttle_kernels.inc through flbgpu_filter_throttle_size_create) against the recorded
answers of the real plugin (tests/golden/throttle_size_ref_cases.json) and against the CPU model (tests/throttle_model.py): return
value and output bytes of every step, the counters and the windows' view after every call.  The admission kernel's two paths run over
the same input in child processes (tests/throttle_child.py) under FLBGPU_TSZ_WAVE_MIN=1 and =100000 and must give the same bytes and
the same windows; dictionary growth, colliding hashes and the grid-stride trips get a child each too.  Nothing here provokes a fault:
every input is one the reference itself answers."""
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
import modify_model as mm
import recmod_model as rm
import oracle_binding as ob
import throttle_child as tch
import throttle_chunks as tc
import throttle_model as tm
from throttle_chunks import NL, T0, kv, named, rec

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "throttle_size_ref_cases.json")))["cases"]
CHILD = os.path.join(HERE, "throttle_child.py")
SWITCHES = ("FLBGPU_TSZ_WAVE_MIN", "FLBGPU_TSZ_DICT_SLOTS", "FLBGPU_TSZ_HASH_BITS", "FLBGPU_LANE_MAX_BLOCKS")


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def steps_of(case):
    return [(s[0], base64.b64decode(s[1]) if s[0] == "chunk" else s[1]) for s in case["steps"]]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(g, case):
    res, _state = tch.drive(g, "throttle_size", [tuple(p) for p in case["props"]], steps_of(case))        # (against the model, state included)
    if not case.get("deviates"):
        assert res == [(s[2], base64.b64decode(s[3]) if s[3] is not None else None) for s in case["steps"] if s[0] == "chunk"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_block_edges(g, n):
    """n rows of one name, then of n names: 40 bytes each against 1000 a window, so the 26th row of the one name is the first to go"""
    one = b"".join(named("a", 40, 1 + i) for i in range(n))
    many = b"".join(named("n%d" % i, 40 + 30 * (i % 40), 1 + i) for i in range(n))
    res, (c, view) = tch.drive(g, "throttle_size", tch.ADMIT_PROPS, [("now", T0), ("tick", T0), ("chunk", one), ("chunk", many), ("chunk", many)])
    assert c["dropped"] >= max(0, n - 25) and b"a" in view
    assert res[0][0] == (tm.NOTOUCH if n <= 25 else tm.MODIFIED)


def child(workload, env):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, CHILD, workload], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    lines = r.stdout.decode().strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "ok", r.stderr.decode()[-1500:]
    return json.loads(lines[-2])


def test_admit_paths_agree(g):
    """segments of 1, 63, 64, 65, 129 and 600 rows; the first row that does not fit at lane 0, 31, 63 and at the first lane of the second
    trip; behind the saturation the next row that fits at lane 0 and 63 of a later trip, in none, and in the last partial trip -- under
    the default threshold here, and in a child each with every segment on the wave path and with every segment on a lane"""
    steps = tch.admit_steps()
    res, state = tch.drive(g, "throttle_size", tch.ADMIT_PROPS, steps)
    here = tch.digest(res, state)
    assert here["dropped"] > 0 and here["kept"] > 0
    assert child("admit", {"FLBGPU_TSZ_WAVE_MIN": "1"}) == here
    assert child("admit", {"FLBGPU_TSZ_WAVE_MIN": "100000"}) == here


def test_thousand_names_under_two_blocks():
    d = child("names1000", {"FLBGPU_LANE_MAX_BLOCKS": "2"})
    assert d["dropped"] > 0 and d["kept"] > 0 and d == child("names1000", {})


def test_dictionary_growth_inside_a_call():
    """16 slots and 100 names: the extraction runs again behind every growth, and no load is applied twice (the windows equal the model's)"""
    d = child("names100", {"FLBGPU_TSZ_DICT_SLOTS": "16"})
    assert d["grows"] >= 3
    wide = child("names100", {})
    same = lambda x: {k: v for k, v in x.items() if k not in ("grows", "names")}
    assert wide["grows"] == 0 and same(d) == same(wide)


def test_dead_names_are_dropped_at_a_growth():
    """six names die, a hundred new ones make the dictionary grow, the six come back in the last call: a dictionary that never grows
    holds them all along (106 names, the old ids found again); one that grew dropped the dead six and entered them anew at the end
    -- and the twenty or so of the hundred that never got a window, being dead at every growth, were dropped on the way as well"""
    wide = child("deadnames", {})
    assert wide["grows"] == 0 and wide["names"] == 106
    d = child("deadnames", {"FLBGPU_TSZ_DICT_SLOTS": "16"})
    assert d["grows"] >= 3 and d["names"] <= 106
    same = lambda x: {k: v for k, v in x.items() if k not in ("grows", "names")}
    assert same(d) == same(wide)


def test_names_count_after_a_growth():
    """the observable: after the old names died, ONE growth with only new names leaves the new names in the dictionary and no old one"""
    d = child("deadgrow", {"FLBGPU_TSZ_DICT_SLOTS": "16"})
    assert d["grows"] == 1 and d["names"] == 8                            # six dead ones gone: without the drop it would be 14


def test_colliding_hashes():
    d = child("names40", {"FLBGPU_TSZ_HASH_BITS": "3"})
    assert d == child("names40", {})


def test_tick_from_a_second_thread(g):
    """a caller's timer thread ticks while the main thread runs calls: the entries serialise themselves and select the filter's device.
    The records are all exempt and the 40 windows were filled before, so the state after 50 ticks and 50 calls does not depend on how
    the two threads interleaved, and equals the model's"""
    import threading
    props = tch.ADMIT_PROPS
    f, m = g.FilterThrottleSize(props), tm.ThrottleSize(props)
    try:
        f.set_now(T0); m.set_now(T0)
        fill = b"".join(named("n%d" % i, 100 + i, 1 + i) for i in range(40))
        assert f.filter(fill) == m.filter(fill)
        exempt = b"".join(rec(kv(("log", "x" * 20), ("i", i)), 1 + i) for i in range(300))
        errors = []

        def ticker():
            try:
                for i in range(50):
                    f.tick(T0 + 1 + i)
            except Exception as e:                                        # noqa: BLE001
                errors.append(e)
        t = threading.Thread(target=ticker)
        t.start()
        for _ in range(50):
            assert f.filter(exempt) == (tm.NOTOUCH, None)
        t.join()
        assert not errors
        for i in range(50):
            m.tick(T0 + 1 + i)
        for _ in range(50):
            m.filter(exempt)
        tch.same_state(f, m, "throttle_size")
        assert f.windows() == m.view() and len(m.view()) == 40
    finally:
        f.close()


def test_large_window_starts_with_fewer_names(g):
    """window 65536: a megabyte of panes a name, so the filter starts with room for 256 names instead of 32768 (34 GB)"""
    props = [("rate", "10"), ("window", "65536"), ("interval", "1"), ("window_time_duration", "1")] + NL
    res, (c, view) = tch.drive(g, "throttle_size", props, [("now", T0), ("chunk", named("a", 600000) + named("a", 60000) + named("b", 1))])
    assert res[0][0] == tm.MODIFIED and c["live"] == 2 and len(view[b"a"]["panes"]) == 65536


def test_call_answers(g):
    f = g.FilterThrottleSize([("rate", "10"), ("window", "5")] + NL)
    try:
        f.set_now(T0)
        a, ex = named("a", 30), rec(kv(("log", "x" * 500)), 9)
        assert f.filter(a + ex + ex) == (tm.NOTOUCH, None) and f.counts() == (3, 3)                     # all kept
        assert f.filter(named("a", 30) + named("b", 51)) == (tm.MODIFIED, b"") and f.counts() == (2, 0)  # all dropped: an empty buffer
        assert f.filter(ex + a + ex + named("a", 20) + ex) == (tm.MODIFIED, ex + ex + named("a", 20) + ex)
        c = f.counters()
        assert (c["records"], c["kept"], c["dropped"], c["exempt"], c["live"], c["created"]) == (10, 7, 3, 5, 1, 1)
    finally:
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


def test_device_chunk_with_dropped_rows(g):
    blob = b"".join(named("n%d" % (i % 3), 100 + i, 1 + i) for i in range(300))
    b = bounds_of(blob)
    offs = b[:6] + [b[5]] + b[6:] + [b[-1], b[-1]]            # rows of length 0: records an earlier filter dropped
    chunk, mem = dev_chunk(g, blob, offs)
    f, m = g.FilterThrottleSize(tch.ADMIT_PROPS), tm.ThrottleSize(tch.ADMIT_PROPS)
    try:
        f.set_now(T0); m.set_now(T0)
        want = m.filter(blob)
        ret, out = f.filter_dev(chunk)
        assert ret == want[0] == tm.MODIFIED and dev_bytes(g, out) == want[1] and out.n == len(offs) - 1
        tch.same_state(f, m, "throttle_size")
    finally:
        f.close()
        for d in mem:
            g.lib().flbgpu_dev_free(d)


def test_chain_grep_throttle_record_modifier(g):
    blob = b"".join(rec(kv(("n", "p%d" % (i % 4)), ("log", "x" * (50 + i)), ("lvl", "debug" if i % 5 == 0 else "info")), 1 + i) for i in range(200))
    grep, RM = [("exclude", "lvl debug")], [("Record", "cluster eu-1")]
    m = tm.ThrottleSize(tch.ADMIT_PROPS)
    m.set_now(T0)
    r1, o1 = ob.Grep(grep).filter(blob)
    r2, o2 = m.filter(o1)
    want = rm.Model(RM).filter(o2)
    assert r1 == r2 == tm.MODIFIED and 0 < len(o2) < len(o1)
    ft = g.FilterThrottleSize(tch.ADMIT_PROPS)
    ft.set_now(T0)
    fs = [g.FilterGrep(grep), ft, g.FilterRecordModifier(RM)]
    try:
        assert g.FilterChain(fs).filter(blob) == want
        tch.same_state(ft, m, "throttle_size")
    finally:
        for f in fs:
            f.close()


FUZZ_SEEDS = list(range(8))


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(g, seed):
    props, steps = tc.fuzz_round(seed)
    m = tm.ThrottleSize(props)
    for st in steps:
        m.set_now(st[1]) if st[0] == "now" else m.tick(st[1]) if st[0] == "tick" else m.filter(st[1])
    assert m.n_kept - m.n_exempt > 0 and m.n_dropped > 0 and m.n_exempt > 0                                # the round holds all three
    tch.drive(g, "throttle_size", props, steps)

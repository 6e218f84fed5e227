"""Child process of tests/test_throttle_size_gpu.py, and its helpers: the test switches of filter_throttle_size (FLBGPU_TSZ_WAVE_MIN,
FLBGPU_TSZ_DICT_SLOTS, FLBGPU_TSZ_HASH_BITS) are read when a filter is created and FLBGPU_LANE_MAX_BLOCKS once per process, so every
setting gets a process of its own.  argv: <workload>; the parent sets the environment.  The workload runs through the product and
through the CPU model (tests/throttle_model.py), step by step: return value, output bytes, counters and the windows' view must agree.
Prints one JSON line -- a digest of every output and of the final view, which the parent compares between settings -- and "ok"."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import throttle_model as tm
from throttle_chunks import NL, T0, named, rec, kv

CAP = 1000                                          # rate 100 x window 10
ADMIT_PROPS = [("rate", "100"), ("window", "10"), ("interval", "1"), ("window_time_duration", "100")] + NL


def drive(g, kind, props, steps, check=True):
    """the steps through product and model: the product's [(ret, out)] per chunk step, the filter's final counters and view"""
    f = (g.FilterThrottleSize if kind == "throttle_size" else g.FilterThrottle)(props)
    m = (tm.ThrottleSize if kind == "throttle_size" else tm.Throttle)(props)
    res = []
    try:
        for st in steps:
            if st[0] == "now":
                f.set_now(st[1]); m.set_now(st[1])
            elif st[0] == "tick":
                f.tick(st[1]); m.tick(st[1])
            else:
                ret, out = f.filter(bytes(st[1]))
                want = m.filter(bytes(st[1]))
                res.append((ret, out))
                if check:
                    assert (ret, out) == want, (len(res), ret, want[0], len(out or b""), len(want[1] or b""))
                    same_state(f, m, kind)
        return res, (f.counters(), f.windows() if kind == "throttle_size" else None)
    finally:
        f.close()


def same_state(f, m, kind):
    if kind == "throttle_size":
        c = f.counters()
        grows = c.pop("grows")
        assert c.pop("names") >= c["live"]
        assert c == m.counters(), (c, m.counters(), grows)
        assert f.windows() == m.view()
    else:
        assert f.counters() == (m.n_in, m.n_kept, m.n_dropped)


def admit_loads(n, p, zeros):
    """n loads: rows in front of p fit, row p never fits, the row behind it fills the window to the byte, then only a load of 0 fits --
    the rows of `zeros`"""
    loads = [1] * n
    if p < n:
        loads[p] = CAP + 1
        if p + 1 < n:
            loads[p + 1] = CAP - p
    for q in zeros:
        if p + 1 < q < n:
            loads[q] = 0
    return loads


def admit_segments():
    segs = []
    for n in (1, 63, 64, 65, 129, 600):
        for p in (0, 31, 63, 64):
            if p >= n:
                continue
            for zeros in ((), (128, 191), (n - 1,), (70,)):
                segs.append(admit_loads(n, p, zeros))
        segs.append([1] * n)                                           # everything fits
        segs.append([CAP + 1] * n)                                     # nothing ever does: no window is created
        segs.append([CAP + 1] * (n - 1) + [7])                         # ... until the last row
    return segs


def admit_steps():
    """every segment under a name of its own, the names' rows interleaved; a second call finds the windows of the first"""
    segs = admit_segments()
    rows, i = [], 0
    while any(i < len(s) for s in segs):
        rows += [named("s%d" % k, s[i], 1 + i) for k, s in enumerate(segs) if i < len(s)]
        i += 1
    chunk = b"".join(rows)
    return [("now", T0), ("tick", T0), ("chunk", chunk), ("tick", T0 + 1), ("chunk", chunk)]


def many_names_steps(names, seed=7):
    import random
    rnd = random.Random(seed)
    rows = []
    for k in range(names):
        rows += [(k, rnd.choice([0, 300, 400, 700, 1001])) for _ in range(1 + k % 3)]
    rnd.shuffle(rows)
    chunk = b"".join(named("name-%d" % k, load, 1 + i) for i, (k, load) in enumerate(rows))
    return [("now", T0), ("tick", T0), ("chunk", chunk), ("chunk", chunk), ("tick", T0 + 200), ("now", T0 + 200), ("chunk", chunk)]


def dead_names_steps():
    """six names go stale and are deleted; a hundred new ones then make the dictionary grow: the dead names are not carried over"""
    first = b"".join(named("old-%d" % k, 10, 1 + k) for k in range(6))
    return [("now", T0), ("tick", T0), ("chunk", first), ("tick", T0 + 150), ("tick", T0 + 300), ("now", T0 + 300)] + many_names_steps(100)[2:] + \
           [("chunk", first)]


def dead_grow_steps():
    """under 16 slots (room for 8 names): six names die, then eight new ones arrive in one call -- one growth, to room for 16"""
    first = b"".join(named("old-%d" % k, 10, 1 + k) for k in range(6))
    fresh = b"".join(named("new-%d" % k, 10, 1 + k) for k in range(8))
    return [("now", T0), ("tick", T0), ("chunk", first), ("tick", T0 + 150), ("now", T0 + 150), ("chunk", fresh)]


WORKLOADS = {"admit": admit_steps, "deadnames": dead_names_steps, "deadgrow": dead_grow_steps, "names1000": lambda: many_names_steps(1000), "names100": lambda: many_names_steps(100), "names40": lambda: many_names_steps(40)}


def digest(res, state):
    h = hashlib.sha256()
    for ret, out in res:
        h.update(b"%d:" % ret + (out if out is not None else b"-"))
    return dict(outputs=h.hexdigest(), view=hashlib.sha256(repr(sorted(state[1].items())).encode()).hexdigest(), grows=state[0]["grows"], names=state[0]["names"],
                dropped=state[0]["dropped"], kept=state[0]["kept"])


def main():
    import flbamd_loader
    g = flbamd_loader.load()
    g.init(0)
    res, state = drive(g, "throttle_size", ADMIT_PROPS, WORKLOADS[sys.argv[1]]())
    print(json.dumps(digest(res, state)))
    print("ok")


if __name__ == "__main__":
    main()

"""The histogram sum in the reference's order (csrc/kernels_seqsum.hip) at the boundaries of its paths.

cmetrics adds every observation to a binary64 in record order, per series (cmt_metric_hist_sum_add); the device reproduces those
bits with a stable radix sort by series, an integer shortcut (k_ss_ints + k_ss_fold_small), a lane fold for runs <= 256 and a wave
fold (512 at a time with its own integer shortcut, then 64 at a time) for longer ones.  A result is the reference's bits or it is
wrong: every comparison here is on bit patterns, none has a tolerance.

Most cases hand columns straight to the kernels through flbgpu_seqsum_dev (start sums, series ids and series counts the filter
cannot produce); the cases marked "filter" go through FilterLogToMetrics and compare with the cmetrics-pinned oracle.  The
reference of the direct cases is ref_fold below, which test_ref_fold_is_the_oracles_fold (no GPU) pins on that oracle."""
import math, struct
import numpy as np
import pytest
import oracle_binding as ob
from synth import v2_record
import flbamd_loader

gpu = pytest.mark.gpu
P52, P53 = 2 ** 52, 2 ** 53
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


def bits(x):
    return struct.pack("<d", x)


def same_f64(a, b):
    return bits(a) == bits(b) or (math.isnan(a) and math.isnan(b))


def ref_fold(sid, vals, seq0):
    """seq0[s] + the values of series s one after the other in input order, per series: np.add.accumulate is strictly sequential
    (bit-equal to a Python `acc += v` loop, checked over 100 000 wide-range values), np.sum is pairwise and is NOT that fold --
    it is never used here.  A sid >= len(seq0) is no observation; a series without observations keeps its start's bits."""
    sid = np.asarray(sid, dtype=np.uint32)
    vals = np.asarray(vals, dtype=np.float64)
    out = np.array(seq0, dtype=np.float64)
    ns = len(out)
    keep = np.flatnonzero(sid < ns)
    order = keep[np.argsort(sid[keep], kind="stable")]
    ssid, svals = sid[order], vals[order]
    cut = np.searchsorted(ssid, np.arange(ns + 1, dtype=np.uint64))
    with np.errstate(all="ignore"):
        for s in np.flatnonzero(cut[1:] > cut[:-1]):
            out[s] = np.add.accumulate(np.concatenate((out[s:s + 1], svals[cut[s]:cut[s + 1]])))[-1]
    return out


def run_dev(g, sid, vals, seq0):
    sid = np.ascontiguousarray(sid, dtype=np.uint32)
    vb = np.ascontiguousarray(vals, dtype=np.float64).view(np.uint64)
    seq = np.array(seq0, dtype=np.float64)
    assert len(sid) == len(vb)
    assert g.lib().flbgpu_seqsum_dev(sid.ctypes.data, vb.ctypes.data, len(sid), len(seq), seq.ctypes.data) == 0, g.last_error()
    return seq


def assert_same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want)))
    assert len(bad) == 0, "%s: %d of %d series differ, first %d: device %r (%s) reference %r (%s)" % (
        what, len(bad), len(want), bad[0], float(got[bad[0]]), bits(float(got[bad[0]])).hex(), float(want[bad[0]]), bits(float(want[bad[0]])).hex())


def check_dev(g, sid, vals, seq0, what=""):
    want = ref_fold(sid, vals, seq0)
    assert_same(run_dev(g, sid, vals, seq0), want, what)
    return want


def order_matters(sid, vals, seq0, want, limit=64):
    """the number of series (among the first `limit` with observations) whose sequential sum is not the correctly rounded one: a case
    over non-associative values that has none would pass with any order of summation"""
    sid, vals = np.asarray(sid), np.asarray(vals, dtype=np.float64)
    n = 0
    for s in np.unique(sid[sid < len(seq0)])[:limit]:
        try:
            n += not same_f64(math.fsum([float(seq0[s])] + vals[sid == s].tolist()), float(want[s]))
        except (OverflowError, ValueError):
            pass
    return n


def decimals(rng, n):
    return rng.uniform(-1000, 1000, n) * 10.0 ** rng.integers(-6, 17, n)


def wide(rng, n):
    """the value mix of test_l2m_gpu.py::test_histogram_exact_sum: random exponents 900..1150, decimals, integers, subnormals, +-1e300,
    +-2^1000, +-0.0 (finite values only)"""
    out = np.empty(n, dtype=np.float64)
    t = rng.random(n)
    for i in range(n):
        if t[i] < 0.5:
            v = NAN
            while not math.isfinite(v):
                v = struct.unpack("<d", struct.pack("<Q", (int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))) & 0x800FFFFFFFFFFFFF
                                                    | int(rng.integers(900, 1150)) << 52))[0]
        elif t[i] < 0.7: v = float(rng.uniform(-1e6, 1e6))
        elif t[i] < 0.8: v = float(int(rng.integers(-10 ** 15, 10 ** 15)))
        elif t[i] < 0.9: v = struct.unpack("<d", struct.pack("<Q", int(rng.integers(0, P52)) | int(rng.integers(0, 2)) << 63))[0]
        else: v = [1e300, -1e300, 5e-324, 0.0, -0.0, 2.0 ** 1000, -2.0 ** 1000][int(rng.integers(0, 7))]
        out[i] = v
    return out


def interleave(rng, runs):
    """runs: one value array per series -> (sid, vals) with the series mixed at random, every series' own order kept (the sort's
    stability is then what brings record order back)"""
    sid = rng.permutation(np.repeat(np.arange(len(runs), dtype=np.uint32), [len(r) for r in runs]))
    vals = np.empty(len(sid), dtype=np.float64)
    for s, r in enumerate(runs):
        vals[sid == s] = r
    return sid, vals


def ints_with_magnitude(rng, n, total):
    """n non-negative integers below 2^52 (as Python ints) whose sum is exactly `total`"""
    base = total // n
    assert 0 < base and 2 * base < P52
    v = [base] * n
    for i in range(0, n - 1, 2):
        d = int(rng.integers(0, base))
        v[i] += d; v[i + 1] -= d
    v[-1] += total - sum(v)
    assert sum(v) == total and all(0 <= x < P52 for x in v)
    return v


# --------------------------------------------------------------------------------------------------- the reference itself (no GPU)
def test_ref_fold_is_the_oracles_fold():
    """ref_fold against the oracle's filter_log_to_metrics (pinned on the real cmetrics): ~3 000 non-associative observations over three
    series in three chunks, the histogram sums bit for bit -- what the GPU cases lean on is itself pinned."""
    rng = np.random.default_rng(5)
    n = 3000
    vals = np.concatenate((decimals(rng, n - 600), wide(rng, 600)))[rng.permutation(n)]
    sid = rng.integers(0, 3, n).astype(np.uint32)
    sid[:3] = [0, 1, 2]                                     # (first appearance in series order)
    recs = [v2_record(1, 0, {"k": "abc"[s], "v": float(v)}) for s, v in zip(sid, vals)]
    o = ob.L2M("histogram", [("label_field", "k")], value_field="v")
    for a, b in ((0, 1100), (1100, 1101), (1101, n)):
        o.filter(b"".join(recs[a:b]))
    osn = o.snapshot()[2]
    assert [s["labels"] for s in osn] == [(b"a",), (b"b",), (b"c",)] and sum(s["count"] for s in osn) == n
    want = ref_fold(sid, vals, np.zeros(3))
    for s in range(3):
        assert same_f64(osn[s]["sum"], float(want[s])), (s, osn[s]["sum"], float(want[s]))
        loop = 0.0
        for v in vals[sid == s]: loop += float(v)
        assert same_f64(loop, float(want[s]))
    assert order_matters(sid, vals, np.zeros(3), want) >= 1
    # a series without observations, and ids past the series count, leave the start alone
    w2 = ref_fold([5, 1, 7], [1.0, 2.0, NAN], [-0.0, 0.5, 3.0])
    assert bits(float(w2[0])) == bits(-0.0) and w2[1] == 2.5 and w2[2] == 3.0


# --------------------------------------------------------------------------------------------------- run lengths: lane / wave / 512 / 64
RUN_LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 383, 384, 385, 511, 512, 513, 575, 576, 577,
               767, 768, 769, 1023, 1024, 1025, 1087, 1088, 1089, 1279, 1535, 1536, 1537, 2047, 2048, 2049, 2560 + 37, 4096 + 5]


@gpu
@pytest.mark.parametrize("starts", ["zero", "drawn-1", "drawn-2"])
def test_run_length_boundaries(g, starts):
    """one call, a series per run length around SS_SMALL (256), the wave loop's 512 and its tail's 64; decimals over 23 decades, the
    series interleaved at random; from 0.0 and from start sums drawn from {0.0, 0.1, -2^60, 1e300}"""
    rng = np.random.default_rng(101)
    sid, vals = interleave(rng, [decimals(rng, n) for n in RUN_LENGTHS])
    if starts == "zero":
        seq0 = np.zeros(len(RUN_LENGTHS))
    else:
        seq0 = np.random.default_rng(int(starts[-1])).choice([0.0, 0.1, -2.0 ** 60, 1e300], len(RUN_LENGTHS))
    want = check_dev(g, sid, vals, seq0, starts)
    assert order_matters(sid, vals, seq0, want) >= 10


# --------------------------------------------------------------------------------------------------- one heavy run of mixed 512-blocks
def mixed_blocks(p):
    """one series, block by block (positions are those of the sorted run: the series is alone in its call)"""
    rng = np.random.default_rng(200 + p)
    small = lambda: rng.integers(-1000, 1000, 512).astype(np.float64)
    blocks = []
    blocks.append(small())                                             # 0: integers, small sum: the shortcut
    b = small(); b[p] = 0.5; blocks.append(b)                          # 1: one 0.5 at position p: the chain
    blocks.append(small())                                             # 2: integers, but the running sum is x.5: the chain
    b = small(); b[(p + 1) % 512] = -0.5; blocks.append(b)             # 3: the running sum is an integer again (chain)
    blocks.append(small())                                             # 4: integers, integer running sum: the shortcut again
    acc = sum(float(x) for x in np.concatenate(blocks))
    assert acc == math.floor(acc) and abs(acc) < 1e7
    # 5: integers that take |acc| + sum|v| over 2^53: the partial sums reach 2^53 - 3, then 509 ones -- the chain sticks at 2^53,
    #    the integers' sum is 2^53 + 506
    b = np.ones(512); b[0] = P52 - 1; b[1] = 2 ** 51; b[2] = P53 - 3 - (P52 - 1) - 2 ** 51 - acc; blocks.append(b)
    assert 0 < b[2] < P52 and int(acc) + sum(int(x) for x in b) == P53 + 506
    b = small(); b[p] = -float(P53); blocks.append(b)                  # 6: back to a small integer through a value that is no "integer" here
    blocks.append(small())                                             # 7: integers, integer running sum: the shortcut once more
    b = small(); b[p] = INF; blocks.append(b)                          # 8: +Inf
    blocks.append(small())                                             # 9: integers on an infinite sum
    b = small(); b[511 - p] = -INF; blocks.append(b)                   # 10: -Inf: NaN from here on
    blocks.append(small())                                             # 11: a last block of integers
    blocks.append(rng.integers(-1000, 1000, 100).astype(np.float64))   # the 64-wide tail
    return np.concatenate(blocks)


@gpu
@pytest.mark.parametrize("p", [0, 63, 64, 511])
def test_mixed_blocks_in_one_heavy_run(g, p):
    vals = mixed_blocks(p)
    sid = np.zeros(len(vals), dtype=np.uint32)
    # every prefix that ends on a block boundary is a case of its own: what a block hands to the next one is checked directly
    for nblocks in range(1, 14):
        n = 512 * nblocks if nblocks < 13 else len(vals)
        want = check_dev(g, sid[:n], vals[:n], [0.0], "p=%d, %d blocks" % (p, nblocks))
        if nblocks == 6:
            assert float(want[0]) == float(P53)                          # (not the integers' sum: the chain's rounding)
            assert order_matters(sid[:n], vals[:n], [0.0], want) == 1
        if nblocks == 8: assert abs(float(want[0])) < 1e6 and float(want[0]) == math.floor(float(want[0]))
        if nblocks in (9, 10): assert float(want[0]) == INF
        if nblocks >= 11: assert math.isnan(float(want[0]))
    # and with a start sum that is not an integer: no block may take the shortcut
    check_dev(g, sid[:512 * 5], vals[:512 * 5], [0.25], "p=%d from 0.25" % p)


# --------------------------------------------------------------------------------------------------- the integer shortcut's limits
def shortcut_cases():
    rng = np.random.default_rng(300)
    n = 5000                                                            # 2 whole 2048-blocks and a third that the next series shares
    f = lambda ints: np.array([float(x) for x in ints])
    flip = lambda v: v * rng.choice([-1.0, 1.0], len(v))
    c = {}
    for start in (0, 12345, -12345):
        c["mag 2^53-1-|start|, start %d" % start] = (float(start), f(ints_with_magnitude(rng, n, P53 - 1 - abs(start))) * (-1.0 if start < 0 else 1.0))
        c["mag 2^53-|start|, start %d" % start] = (float(start), f(ints_with_magnitude(rng, n, P53 - abs(start))) * (-1.0 if start < 0 else 1.0))
        # three past the limit, ending on 1, 1, 1: the chain stops at 2^53, the integers' sum is 2^53 + 3
        c["mag 2^53+3-|start| ending 1 1 1, start %d" % start] = (float(start), f(ints_with_magnitude(rng, n - 3, P53 - abs(start)) + [1, 1, 1]) * (-1.0 if start < 0 else 1.0))
        c["mixed signs, mag 2^53-1-|start|, start %d" % start] = (float(start), flip(f(ints_with_magnitude(rng, n, P53 - 1 - abs(start)))))
        c["mixed signs, mag 2^53-|start|, start %d" % start] = (float(start), flip(f(ints_with_magnitude(rng, n, P53 - abs(start)))))
    c["mag 2^52-1"] = (0.0, f(ints_with_magnitude(rng, n, P52 - 1)))
    c["mag 2^52"] = (0.0, f(ints_with_magnitude(rng, n, P52)))
    c["a value of 2^52, then 2^52-1, then ones"] = (0.0, f([P52, P52 - 1] + [1] * (n - 2)))
    c["2^52-1 first, ones behind it"] = (0.0, f([P52 - 1] + [1] * (n - 1)))
    c["negative integers and -0.0"] = (0.0, np.where(rng.random(n) < 0.3, -0.0, -rng.integers(0, 10 ** 9, n).astype(np.float64)))
    c["all -0.0 from -0.0"] = (-0.0, np.full(n, -0.0))
    c["all -0.0 from 0.0"] = (0.0, np.full(n, -0.0))
    c["-0.0 and one 0.0 from -0.0"] = (-0.0, np.where(np.arange(n) == 4000, 0.0, -0.0))
    c["integers that cancel from -0.0"] = (-0.0, f([7, -7] * (n // 2)))
    c["start 2^52, ones"] = (float(P52), np.ones(n))
    c["start 2^52, mag 2^52+3 ending 1 1 1"] = (float(P52), f(ints_with_magnitude(rng, n - 3, P52) + [1, 1, 1]))
    c["start 2^53, ones"] = (float(P53), np.ones(n))
    c["start -2^53, minus ones"] = (float(-P53), -np.ones(n))
    c["start 0.5, integers around 2^51"] = (0.5, rng.integers(-2 ** 51, 2 ** 51, n).astype(np.float64))
    c["start 0.5, small integers"] = (0.5, rng.integers(-1000, 1000, n).astype(np.float64))
    c["start -(2^52-1), mag 2^52+4 ending -1 -1 -1"] = (-float(P52 - 1), -f(ints_with_magnitude(rng, n - 3, P52 + 1) + [1, 1, 1]))
    c["start -(2^52-1), mag 2^52"] = (-float(P52 - 1), -f(ints_with_magnitude(rng, n, P52)))
    c["3000 x (2^52-1)"] = (0.0, np.full(3000, float(P52 - 1)))
    c["3000 integers of 52 bits"] = (0.0, rng.integers(2 ** 51, P52, 3000).astype(np.float64))
    c["start NaN, integers"] = (NAN, rng.integers(0, 100, n).astype(np.float64))
    c["start +Inf, integers"] = (INF, rng.integers(0, 100, n).astype(np.float64))
    return c


SHORTCUT = shortcut_cases()


@gpu
@pytest.mark.parametrize("name", list(SHORTCUT))
def test_integer_shortcut_limits(g, name):
    """k_ss_ints + k_ss_fold_small: a long run of integers at the limits of "every partial sum is exact", alone and with a second
    series behind it whose first observations share a 2048-block with its end (the per-element atomics carry part of both)"""
    start, v0 = SHORTCUT[name]
    rng = np.random.default_rng(301)
    want = check_dev(g, np.zeros(len(v0), dtype=np.uint32), v0, [start], name + " (alone)")
    if "ending" in name or "then ones" in name or name in ("start 2^53, ones", "start -2^53, minus ones", "3000 integers of 52 bits"):
        exact = int(start) + sum(int(x) for x in v0)
        assert float(want[0]) != float(exact), name                     # (the integers' sum is another number: the case can fail)
    for second, s1 in ((rng.integers(0, 1000, 700).astype(np.float64), 7.0), (decimals(rng, 700), 0.1), (np.full(700, float(P52 - 1)), float(P52 - 1))):
        sid, vals = interleave(rng, [v0, second])
        check_dev(g, sid, vals, [start, s1], name + " (two series)")
        sid, vals = interleave(rng, [second, v0])                      # ... and as the series behind the boundary
        check_dev(g, sid, vals, [s1, start], name + " (two series, swapped)")


@gpu
@pytest.mark.parametrize("n", [1, 2, 64, 256, 257, 512, 700])
def test_negative_zero_survives(g, n):
    """-0.0 + -0.0 is -0.0: a sum that starts at -0.0 and only ever sees -0.0 keeps its sign in every path (the integer shortcuts work
    on integers, which have no -0)"""
    got = run_dev(g, np.zeros(n, dtype=np.uint32), np.full(n, -0.0), [-0.0])
    assert bits(float(got[0])) == bits(-0.0), got
    got = run_dev(g, np.zeros(n, dtype=np.uint32), np.full(n, -0.0), [0.0])
    assert bits(float(got[0])) == bits(0.0), got


# --------------------------------------------------------------------------------------------------- the sum of magnitudes wraps
BIG = float(P52 - 1)                                                   # 4503599627370495.0


@gpu
def test_magnitude_wrap_one_series(g):
    """4097 x (2^52 - 1): the 64-bit sum of the magnitudes is 2^52 - 4097 modulo 2^64 -- "small" --, the partial sums left the exact
    integers after the second observation.  (Before the fix: 4.5e15 where the reference has 1.845124767333692e19.)"""
    assert 4097 * (P52 - 1) % 2 ** 64 < P52
    vals = np.full(4097, BIG)
    want = check_dev(g, np.zeros(4097, dtype=np.uint32), vals, [0.0])
    assert float(want[0]) == 1.845124767333692e19                       # (equal values: no order to tell apart; the mixed-sign case has one)


@gpu
def test_magnitude_wrap_two_series(g):
    rng = np.random.default_rng(400)
    sid, vals = interleave(rng, [np.full(4097, BIG), np.full(4097, -BIG)])
    want = check_dev(g, sid, vals, [0.0, 0.0])
    assert float(want[0]) == 1.845124767333692e19 and float(want[1]) == -1.845124767333692e19


@gpu
def test_magnitude_wrap_mixed_signs(g):
    """+-(2^52 - 2^k), k < 31: 4097 of them have a magnitude sum of 2^64 + 2^52 - (at most 2^43): it wraps to below 2^52 (asserted)"""
    rng = np.random.default_rng(401)
    mags = [P52 - 2 ** int(k) for k in rng.integers(0, 31, 4097)]
    assert sum(mags) >= 2 ** 64 and sum(mags) % 2 ** 64 < P52
    vals = np.array([float(m) for m in mags]) * rng.choice([-1.0, 1.0], 4097)
    sid = np.zeros(4097, dtype=np.uint32)
    want = check_dev(g, sid, vals, [0.0])
    assert order_matters(sid, vals, [0.0], want) == 1
    # the same behind another series, so that its first and last 2048-blocks are shared ones
    sid2, vals2 = interleave(rng, [np.ones(1000), vals, np.ones(1000)])
    check_dev(g, sid2, vals2, [0.0, 0.0, 0.0])


@gpu
def test_magnitude_wrap_through_the_filter(g):
    """filter: one chunk of 4097 records {"v": 4503599627370495.0}"""
    data = v2_record(1, 0, {"v": BIG}) * 4097
    o = ob.L2M("histogram", [], value_field="v")
    f = g.FilterLogToMetrics("histogram", [], value_field="v")
    assert o.filter(data) == f.filter(data)[0]
    a, b = f.snapshot(), o.snapshot()[2]
    f.close()
    assert len(a) == len(b) == 1 and a[0]["count"] == b[0]["count"] == 4097
    assert b[0]["sum"] == 1.845124767333692e19
    assert same_f64(a[0]["sum"], b[0]["sum"]), (a[0]["sum"], b[0]["sum"])


# --------------------------------------------------------------------------------------------------- series counts: the sort's key bits
SERIES_SEED = 519                # (one with which the few observations of nseries 1 and 2 are order-sensitive too)


@gpu
@pytest.mark.parametrize("nseries", [1, 2, 255, 256, 257, 65535, 65536, 65537])
def test_series_counts_around_the_key_bits(g, nseries):
    """three to five decimals per series in random interleaving; ids nseries, nseries + 1 and 0xFFFFFFFF (no observations: huge values and
    NaN that would show in any series they leaked into); series without observations, among them a NaN and a -0.0 start, come back
    bit-identical.  The sorted keys are 0 .. nseries: 2^k - 1, 2^k and 2^k + 1 series are where the number of key bits changes."""
    rng = np.random.default_rng(SERIES_SEED + nseries % 1000)
    for variant in range(2 if nseries < 4 else 1):
        counts = rng.integers(3, 6, nseries)
        counts[rng.random(nseries) < 0.1] = 0
        counts[[0, nseries - 1]] = 5                                    # (the lowest and the highest id have observations)
        seq0 = decimals(rng, nseries)
        if nseries >= 4:
            counts[[1, nseries - 2]] = 0
            seq0[1], seq0[nseries - 2] = NAN, -0.0
        elif variant == 1:                                              # one or two series: a call whose first series has nothing
            counts[0] = 0
            seq0[0] = NAN if nseries == 1 else -0.0
        sid = np.repeat(np.arange(nseries, dtype=np.uint32), counts)
        vals = decimals(rng, len(sid))
        junk_sid = np.array([nseries, nseries + 1, 0xFFFFFFFF, nseries, 0xFFFFFFFF, nseries + 1, nseries], dtype=np.uint32)
        junk_val = np.array([1e308, NAN, INF, -1e308, 1.7e308, -INF, NAN])
        sid, vals = np.concatenate((sid, junk_sid)), np.concatenate((vals, junk_val))
        perm = rng.permutation(len(sid))
        sid, vals = sid[perm], vals[perm]
        got = run_dev(g, sid, vals, seq0)
        want = ref_fold(sid, vals, seq0)
        assert_same(got, want, "nseries %d" % nseries)
        empty = np.flatnonzero(counts == 0)
        assert np.array_equal(got.view(np.uint64)[empty], seq0.view(np.uint64)[empty])      # untouched: the very bits, a NaN's too
        if variant == 0:
            assert order_matters(sid, vals, seq0, want, limit=400) >= 1


# --------------------------------------------------------------------------------------------------- the grids' second trips
@gpu
def test_second_trip_of_keys_and_runs(g):
    """n = 4096 blocks x 256 + 300: k_ss_keys and k_ss_runs go round their grid-stride loops a second time"""
    rng = np.random.default_rng(600)
    n = 1048576 + 300
    sid = rng.integers(0, 5, n).astype(np.uint32)
    sid[-300:] = np.arange(300) % 5                                     # (every series has observations in the second trip)
    vals = decimals(rng, n)
    want = check_dev(g, sid, vals, np.zeros(5))
    assert order_matters(sid, vals, np.zeros(5), want) >= 1


@gpu
def test_second_trip_of_the_integer_pass(g):
    """n = 4096 blocks x 2048 + 2048 + 17: k_ss_ints starts a second trip (its LDS scratch used again), whose first block is shared by
    the last two series and whose second one is a short block of the last series alone; runs of millions of small integers, and a
    series of decimals in front of them"""
    rng = np.random.default_rng(601)
    n = 8388608 + 2048 + 17
    counts = [300000, 5000000, n - 300000 - 5000000 - 1000, 1000]
    sid = np.repeat(np.arange(4, dtype=np.uint32), counts)
    rng.shuffle(sid)
    vals = rng.integers(0, 1000, n).astype(np.float64)
    dec = sid == 0
    vals[dec] = decimals(rng, int(dec.sum()))
    seq0 = np.array([0.1, 3.0, 0.0, 1e6])
    want = check_dev(g, sid, vals, seq0)
    assert order_matters(sid, vals, seq0, want, limit=1) == 1


# --------------------------------------------------------------------------------------------------- order
@gpu
def test_order_sensitivity(g):
    """20 000 observations over 4 series, the value mix of test_histogram_exact_sum, as generated and reversed: each order has its own bits"""
    rng = np.random.default_rng(700)
    n = 20000
    sid = rng.integers(0, 4, n).astype(np.uint32)
    vals = wide(rng, n)
    fwd = check_dev(g, sid, vals, np.zeros(4), "as generated")
    rev = check_dev(g, sid[::-1].copy(), vals[::-1].copy(), np.zeros(4), "reversed")
    assert any(not same_f64(float(a), float(b)) for a, b in zip(fwd, rev))
    assert order_matters(sid, vals, np.zeros(4), fwd) >= 1


# --------------------------------------------------------------------------------------------------- filter level, the wave path
def filter_chunks(with_error):
    rng = np.random.default_rng(802)                                    # (all three series order-sensitive, with and without the error)
    n = 9000
    sid = rng.integers(0, 3, n).astype(np.uint32)
    sid[:3] = [0, 1, 2]
    vals = wide(rng, n)
    recs = [v2_record(1, 0, {"k": "abc"[s], "v": float(v)}) for s, v in zip(sid, vals)]
    spans = [(0, 4000), (4000, 4001), (4001, 4001), (4001, 9000)]
    chunks = [b"".join(recs[a:b]) for a, b in spans]
    seen = np.ones(n, dtype=bool)
    if with_error:                                                      # rows 2600 .. 3999 of the first chunk lie behind a byte that is no msgpack
        chunks[0] = b"".join(recs[:2600]) + b"\xc1" + b"".join(recs[2600:4000])
        seen[2600:4000] = False
    return chunks, sid[seen], vals[seen]


@gpu
@pytest.mark.parametrize("with_error", [False, True])
def test_filter_heavy_path_sum_order_1(g, with_error):
    """filter: 9 000 records in chunks of 4 000, 1, 0 and 4 999 over 3 series (runs of ~1 300 and ~1 700: the wave loop), msgpack
    float64 of the wide value mix; `sum` against the oracle bit for bit; observations behind a decode error are not added"""
    chunks, sid, vals = filter_chunks(with_error)
    props = [("label_field", "k")]
    o = ob.L2M("histogram", props, value_field="v")
    f = g.FilterLogToMetrics("histogram", props, value_field="v")
    for c in chunks:
        assert o.filter(c) == f.filter(c)[0]
    a, b = f.snapshot(), o.snapshot()[2]
    f.close()
    want = ref_fold(sid, vals, np.zeros(3))
    assert [s["labels"] for s in a] == [s["labels"] for s in b] == [(b"a",), (b"b",), (b"c",)]
    assert sum(s["count"] for s in b) == len(sid)
    for s in range(3):
        assert a[s]["count"] == b[s]["count"]
        assert same_f64(b[s]["sum"], float(want[s]))
        assert same_f64(a[s]["sum"], b[s]["sum"]), (s, a[s]["sum"], b[s]["sum"])
    assert order_matters(sid, vals, np.zeros(3), want) == 3


@gpu
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("with_error", [False, True])
def test_filter_heavy_path_sum_order_2(g, with_error, world):
    """filter: the same records with sum_order 2 -- every rank keeps its observations, the flush folds them rank after rank
    (chain_begin / seq_replay / chain_end); the observations behind the decode error are not kept either"""
    chunks, sid, vals = filter_chunks(with_error)
    props = [("label_field", "k")]
    o = ob.L2M("histogram", props, value_field="v")
    ranks = []
    for r in range(world):
        f = g.FilterLogToMetrics("histogram", props, value_field="v")
        f.set_sum_order(2)
        f.set_index_base(r << 40)
        ranks.append(f)
    for i, c in enumerate(chunks):                                      # (two ranks: the first two chunks, then the last two)
        assert o.filter(c) == ranks[i * world // len(chunks)].filter(c)[0]
    allk, seen = [], set()
    for f in ranks:
        for k in f.export()[0]:
            if k not in seen:
                seen.add(k); allk.append(k)
    G = ranks[0].chain_begin(allk)
    for f in ranks:
        G = f.seq_replay(allk, G)
    for f in ranks:
        f.chain_end(allk, G)
        f.close()
    b = {s["labels"]: s["sum"] for s in o.snapshot()[2]}
    want = ref_fold(sid, vals, np.zeros(3))
    assert len(allk) == 3
    for k, x in zip(allk, G):
        lab = tuple(k.split(b"\0")[:-1])
        assert same_f64(b[lab], float(want[b"abc".index(lab[0])]))
        assert same_f64(x, b[lab]), (world, lab, x, b[lab])

"""The named cases of tests/l2m_chunks.py sit on the edges they are named for (each case's predicate, computed from the case alone), the
module's constants are those of the device code, and its plain models -- the stale rule, the bucket rule, the gauge rule, the
first-appearance order, the rounding of the exact sum -- agree with oracle_binding.L2M (pinned on the real cmetrics by
tests/test_l2m_refplugin.py) on every case that can be written as records.  tests/test_l2m_edges_gpu.py runs the cases on the device.

No case may be skipped, filtered out or marked as an expected failure: a case that cannot be built fails the test."""
import math
import os
import random
import re
import struct
import sys
from fractions import Fraction

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import l2m_chunks as lc
import oracle_binding as ob

CSRC = os.path.join(os.path.dirname(HERE), "fluent-bit_amd", "csrc")
CUS = (256, 64, 304)             # the grid-stride cases are built from the device's CU count: MI355X's and two others


def same_f64(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b) or (math.isnan(a) and math.isnan(b))


def test_constants_are_those_of_the_device_code():
    dev = open(os.path.join(CSRC, "dev.hpp")).read()
    k = open(os.path.join(CSRC, "l2m_kernels.inc")).read()

    def num(src, pat):
        m = re.search(pat, src)
        assert m, pat
        return tuple(int(x, 0) for x in m.groups())
    assert num(k, r"constexpr int L2M_BLOCK = (\d+);") == (lc.L2M_BLOCK,)
    assert num(k, r"constexpr int L2M_TILE = (\d+);") == (lc.L2M_TILE,)
    assert num(k, r"constexpr int L2M_ST_BLOCK = (\d+), L2M_ST_ITEMS = (\d+), L2M_ST_TILE = L2M_ST_BLOCK \* L2M_ST_ITEMS;") == (lc.L2M_ST_BLOCK, lc.L2M_ST_ITEMS)
    assert num(k, r"__launch_bounds__\((\d+)\) k_l2m_stale_spine") == (lc.L2M_SPINE,)
    assert num(k, r"for \(uint64_t base = 0; base < ntiles; base \+= (\d+)\)") == (lc.L2M_SPINE,)
    assert num(k, r"constexpr int L2M_AGG_BLOCK = (\d+);") == (lc.L2M_AGG_BLOCK,)
    assert num(k, r"constexpr int L2M_AGG_SLOTS = (\d+);") == (lc.L2M_AGG_SLOTS,)
    assert num(k, r"for \(int probe = 0; probe < (\d+); probe\+\+\)") == (lc.L2M_AGG_PROBES,)
    assert num(k, r"uint32_t h = \(key \* (\d+)u\) >> (\d+);") == (2654435761, 20) and 1 << (32 - 20) == lc.L2M_AGG_SLOTS
    assert num(k, r"if \(grid > (\d+)\) grid = (\d+);") == (lc.L2M_GENERIC_GRID, lc.L2M_GENERIC_GRID)
    assert "uint64_t grid = (uint64_t) cus * 2;" in k                 # extract and aggregate: 2 x CUs workgroups
    assert num(dev, r"constexpr int L2M_NLIMB = (\d+);") == (lc.L2M_NLIMB,)
    assert num(dev, r"constexpr int L2M_W_FIRST = (\d+), L2M_W_LASTIDX = (\d+), L2M_W_LASTVAL = (\d+), L2M_W_COUNT = (\d+), L2M_W_SPECIAL = (\d+),\s*"
                    r"L2M_W_LIMB = (\d+), L2M_W_BUCKET = L2M_W_LIMB \+ L2M_NLIMB;") == \
        (lc.L2M_W_FIRST, lc.L2M_W_LASTIDX, lc.L2M_W_LASTVAL, lc.L2M_W_COUNT, lc.L2M_W_SPECIAL, lc.L2M_W_LIMB)
    assert "return mode == L2M_HISTOGRAM ? L2M_W_BUCKET + nb + 1 : L2M_W_SPECIAL;" in dev
    assert num(dev, r"L2M_SID_NONE = (0x[0-9A-Fa-f]+)u;") == (lc.NONE,) and num(dev, r"L2M_SID_DEFER = (0x[0-9A-Fa-f]+)u;") == (lc.DEFER,)
    assert num(dev, r"L2M_SID_STALE = (0x[0-9A-Fa-f]+)u;") == (lc.STALE,)
    assert num(dev, r"enum \{ L2M_COUNTER = (\d), L2M_GAUGE = (\d), L2M_HISTOGRAM = (\d) \};") == (lc.COUNTER, lc.GAUGE, lc.HISTOGRAM)
    d = open(os.path.join(CSRC, "l2m_dev.inc")).read()
    assert "h *= 0x9E3779B97F4A7C15ull; h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;" in d and "return h < 2 ? h + 2 : h;" in d
    assert "uint64_t h = 0xcbf29ce484222325ull;" in d and "h = (h ^ b) * 0x100000001b3ull;" in d


# ------------------------------------------------------------------------------------------ predicates
def all_column_cases(cus):
    return lc.stale_cases() + lc.agg_cases(cus) + [lc.gauge_later_range_case()]


def test_case_names_are_unique():
    names = [c.name for c in all_column_cases(256)] + [c.name for c in record_cases(256)]
    assert len(names) == len(set(names))


def test_stale_cases_are_on_their_edges():
    cs = lc.stale_cases()
    for c in cs:
        c.check()
    T = lc.L2M_ST_TILE
    assert {c.n for c in cs} >= {1, T - 1, T, T + 1, 1024 * T - T, 1024 * T, 1024 * T + T}
    assert any((c.n + T - 1) // T == 1025 for c in cs)                        # tile count is 1025
    assert {c.first_bad for c in cs if c.name.startswith("stale/first_bad/")} >= {0, T, T + 10, 2 * T + 5}


@pytest.mark.parametrize("cus", CUS)
def test_aggregate_cases_are_on_their_edges(cus):
    cs = lc.agg_cases(cus)
    for c in cs:
        c.check()
    G = 2 * cus * lc.L2M_AGG_BLOCK
    for mode in lc.MODE_NAMES.values():
        assert {len(c.calls[0][0]) for c in cs if c.name.startswith("agg/%s/n=" % mode)} == {1, 255, 256, 257, G - 1, G, G + 1}
    lc.gauge_later_range_case().check()
    by = {c.name: c for c in cs}
    # the chains walk the running sum through the signs the carry has to survive
    assert lc.chain_sign_walk(by["agg/histogram/chain/pos_neg_zero_pos"]) == [1, -1, 0, 1]
    assert lc.chain_sign_walk(by["agg/histogram/chain/neg_small_from_large"]) == [-1, -1, 0, 1]
    fin = lambda name: lc._model_of(by["agg/histogram/chain/" + name]).final(0)["sum"]
    assert fin("twice_dbl_max") == math.inf and fin("negative_overflow") == -math.inf and fin("overflow_then_back") == 1.0
    assert fin("just_under_the_rounding_overflow") == lc.DBL_MAX and fin("exactly_the_rounding_overflow") == math.inf
    assert fin("exactly_the_rounding_overflow_negative") == -math.inf and fin("top_digit_many_dbl_max") == lc.DBL_MAX
    assert fin("tie_to_even_down") == 1.0 and fin("tie_to_even_up") == 1.0 + 2.0 ** -51
    big = 2.0 ** (32 * 61 - 1074)
    assert fin("sticky_60_limbs_below") == math.nextafter(big, math.inf) and fin("sticky_negative") == -math.nextafter(big, math.inf)
    assert 0 < fin("subnormal_result") < 2.0 ** -1022 and fin("smallest_subnormals_add_up") == 7 * 5e-324


def record_cases(cus):
    return lc.extract_fit_cases() + lc.extract_single_cases() + lc.extract_end_cases() + lc.extract_count_cases() + \
        [lc.second_trip_rows(cus)] + lc.extract_dev_cases(cus) + [lc.generic_case()]


def test_record_cases_are_on_their_edges():
    cs = record_cases(256)
    for c in cs:
        c.check()
    fit = [c.name for c in cs if c.name.startswith("extract/fit/")]
    assert len(fit) == 48 and all("extract/fit/align=%d/%s" % (a, w) in fit for a in range(16) for w in ("exact", "one_over", "one_under"))
    # the fit test's both sides, stated on the bytes: the wave's 64 records plus align are exactly L2M_TILE / one more / one less
    for c in cs:
        m = re.match(r"extract/fit/align=(\d+)/(\w+)", c.name)
        if m:
            lens = [len(r) for r in c.recs]
            assert len(lens) == 128 and sum(lens[:64]) % 16 == int(m.group(1))
            assert sum(lens[64:]) + int(m.group(1)) == lc.L2M_TILE + {"exact": 0, "one_over": 1, "one_under": -1}[m.group(2)]


def test_wrap_keys_have_two_keys_at_home_in_the_last_slot():
    ks = lc.wrap_keys(16)
    assert len(set(ks)) == len(ks) and [lc.home_slot(k, 16) for k in ks[:2]] == [15, 15]


# ------------------------------------------------------------------------------------------ the models against the oracle
def oracle_of(mode, props, chunks, value_field="v"):
    o = ob.L2M(lc.MODE_NAMES[mode], props, value_field=None if mode == lc.COUNTER else value_field)
    for c in chunks:
        o.filter(c)
    return o.snapshot()


def test_aggregate_model_is_the_oracle_s():
    ran = 0
    for c in lc.agg_cases(256):
        if not c.records:
            continue
        props = [("label_field", "k")] + [("bucket", repr(b)) for b in c.bounds]
        keys, bounds, sn = oracle_of(c.mode, props, lc.as_records(c))
        m = lc._model_of(c)
        assert bounds == c.bounds, c.name
        order = m.order()
        assert [s["labels"] for s in sn] == [(b"s%d" % s,) for s in order], c.name         # first-appearance order
        for s, o in zip(order, sn):
            f = m.final(s)
            if c.mode != lc.HISTOGRAM:
                assert same_f64(f["value"], o["value"]), (c.name, s, f, o)                   # the count / the gauge rule
                continue
            assert f["buckets"] == o["buckets"] and f["count"] == o["count"], (c.name, s, f, o)   # the bucket rule
            if c.exact or math.isnan(o["sum"]):
                assert same_f64(f["sum"], o["sum"]), (c.name, s, f, o)
        ran += 1
    assert ran >= 40


def test_stale_model_is_the_oracle_s():
    ran = 0
    for c in lc.stale_cases():
        if c.n > 3 * lc.L2M_ST_TILE:
            continue
        keys, bounds, sn = oracle_of(lc.GAUGE, [("label_field", "k")], [lc.stale_as_records(c)])
        sid, val = lc.stale_model(c.sid, c.val, c.first_bad)
        want = [((b"r%d" % i,), lc.b2f(val[i])) for i in range(min(c.n, c.first_bad)) if sid[i] < lc.STALE]
        assert [(s["labels"], s["value"]) for s in sn] == want, c.name
        assert not any(s & lc.STALE and s not in (lc.NONE, lc.DEFER) for s in sid[:min(c.n, c.first_bad)]), c.name
        ran += 1
    assert ran >= 15


# ------------------------------------------------------------------------------------------ the rounding model
def test_rounding_model_is_fsum_where_fsum_does_not_overflow():
    rng = random.Random(5)
    pools = [[1.0, 2.0 ** -53, 2.0 ** -52, -1.0, 2.0 ** -105, 1e16, -1e16, 3.0],
             [5e-324, -5e-324, 2.0 ** -1022, -2.0 ** -1023, 2.0 ** -1074 * 3, 1e-310],
             [lc.DBL_MAX, -lc.DBL_MAX, 2.0 ** 970, 2.0 ** 969, -2.0 ** 970, 1.0, 2.0 ** 1023],
             [x for x in lc.HIST_VALUES if math.isfinite(x)]]
    ran = 0
    for it in range(3000):
        pool = pools[it % 4]
        vals = [rng.choice(pool) for _ in range(rng.randrange(1, 9))]
        if it % 5 == 0:
            vals += [struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64) & 0xFFEFFFFFFFFFFFFF))[0] for _ in range(3)]
        vals = [v for v in vals if math.isfinite(v)]
        exact = sum((Fraction(v) for v in vals), Fraction(0))
        got = lc.round_fraction(exact)
        assert sum(lc.to_units(v) for v in vals) == exact * Fraction(2) ** 1074
        try:
            want = math.fsum(vals)
        except OverflowError:
            continue                                                 # (fsum gives up on partials it cannot hold; the model does not)
        assert same_f64(got, want) or (got == 0 and want == 0), (vals, got, want)
        ran += 1
    assert ran > 2000
    assert lc.round_fraction(Fraction(2) ** 1024 - Fraction(2) ** 970) == math.inf
    assert lc.round_fraction(Fraction(2) ** 1024 - Fraction(2) ** 970 - 1) == lc.DBL_MAX
    assert lc.round_fraction(-(Fraction(2) ** 1024)) == -math.inf
    assert lc.round_fraction(Fraction(1, 2 ** 1075)) == 0.0 and lc.round_fraction(Fraction(3, 2 ** 1075)) == 2 * 5e-324
    assert lc.round_fraction(Fraction(1, 3)) == 1 / 3 and lc.round_fraction(Fraction(1, 10)) == 0.1

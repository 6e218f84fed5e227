"""The named cases of tests/sp_chunks.py sit on the edges they are named for (each case's predicate, computed from the chunk and the
oracle's answer alone; a float-typed sum must be exact in binary64 in every partial sum, proved with fractions.Fraction, so that the
device test can compare bytes), the oracle's answers are the reference's (oracle/_ref/ref_sp: the reference's own flb_sp) and the
committed digests of tests/golden/sp_edges_kat.json -- the check that travels to where the reference is not.
tests/test_sp_edges_gpu.py runs the same cases on the device.

No case may be skipped, filtered out or marked as an expected failure: a case that cannot be built fails the test."""
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_sp
import sp_chunks as sc
from sp_chunks import osp

CSRC = os.path.join(os.path.dirname(HERE), "fluent-bit_amd", "csrc")
GROUPS = list(sc.GROUPS)


def test_limits_are_those_of_the_device_code():
    dev = open(os.path.join(CSRC, "dev.hpp")).read()
    ker = open(os.path.join(CSRC, "sp_kernels.inc")).read()
    sel = open(os.path.join(CSRC, "sp_select.inc")).read()
    for name in ("SP_MAX_KEYS", "SP_MAX_GB", "SP_MAX_SRC", "SP_MAX_SUB", "SP_MAX_LEAF", "SP_MAX_OPS", "SP_SRC_MAX", "L2M_NLIMB"):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, dev).group(1)) == sc.LIM[name], name
    for name in ("SP_FAST_KEYS", "SP_BLOCK", "SP_TILE"):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, ker).group(1)) == sc.LIM[name], name
    assert sc.LIM["SP_SRC_ADD"] == sc.LIM["SP_A_LIMB"] + sc.LIM["L2M_NLIMB"] and sc.LIM["SP_VT_MANY"] == 63
    assert sc.LIM["SP_TILE"] % 16 == 0 and sc.LIM["SP_BLOCK"] % 64 == 0
    # the launch shapes the grid cases are derived from
    assert "if (b > %d) b = %d;" % (sc.SELECT_GRID[0], sc.SELECT_GRID[0]) in sel and "dim3(%d), 0, st, a);" % sc.SELECT_GRID[1] in sel
    assert "if (grid > %d) grid = %d;" % (sc.GENERIC_GRID[0], sc.GENERIC_GRID[0]) in ker and "k_sp_generic, dim3((unsigned) grid), dim3(%d)" % sc.GENERIC_GRID[1] in ker
    assert "k_sp_normalize, dim3(%d), dim3(%d)" % sc.NORMALIZE_GRID in ker
    assert "uint64_t grid = (uint64_t) cus * 2;" in ker


def test_case_names_are_unique_and_every_group_has_cases():
    names = [c.name for c in sc.all_cases()]
    assert len(names) == len(set(names)) and all(sc.cases(g) for g in GROUPS)
    assert all(c.name.startswith(g + "/") for g in GROUPS for c in sc.cases(g))
    assert tuple(c.name for c in sc.cases("grid")) == sc.GRID_NAMES


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_is_on_its_edge(group):
    for c in sc.cases(group):
        c.check()


def test_staging_cases_cover_tile_and_direct_at_every_named_place():
    cs = {c.name: c for c in sc.cases("staging")}
    for dec in ("", "dec/"):
        for k in (1, 2, 63):
            for al in (0, 1, 15):
                exact, over = (sc.tile_plan(cs["staging/%sfit/k%d/a%d/%s" % (dec, k, al, w)].steps[0].off)[0][0] for w in ("exact", "over"))
                assert exact[1:] == (k + 1, "tile", sc.SP_TILE) and over[1] == k and over[2] == "tile"
        assert [sc.tile_plan(cs["staging/%sdirect/lane%d" % (dec, l)].steps[0].off)[0].count((l, 1, "direct", 0)) for l in (0, 31, 63)] == [1, 1, 1]
        assert sorted(len(cs["staging/%stail/mod%d" % (dec, m)].steps[0].data) % 16 for m in (1, 8, 15)) == [1, 8, 15]
    assert sum(1 for c in cs.values() if c.notes["deferred"]) == len(cs) // 2


def test_key_pairs_straddle_the_fast_walk_and_answer_the_same():
    cs = [c for c in sc.cases("keys") if "pair" in c.notes]
    for p in sorted({c.notes["pair"] for c in cs}):
        a, b = [c for c in cs if c.notes["pair"] == p]
        assert len(sc.osp_keys(a.sql)) == sc.LIM["SP_FAST_KEYS"] == len(sc.osp_keys(b.sql)) - 1
        assert a.want() == b.want() and a.steps[0] == b.steps[0]
    for c in sc.cases("keys"):
        if "over" in c.notes:
            osp.parse(c.notes["over"])                                     # the reference's grammar takes it: the limit is the device's


def test_multiplicity_counts_and_what_the_old_clamps_would_have_answered():
    names = [c.name for c in sc.cases("multiplicity")]
    for n in sc.MULTS:
        assert all("multiplicity/%s/%d" % (k, n) in names for k in ("agg", "select", "float", "groupby"))
    assert sc.MULTS == (1, 2, 63, 64, 65, 255, 256, 65535, 65536)
    c = next(c for c in sc.cases("multiplicity") if c.name == "multiplicity/agg/64")
    assert c.rows_out(0)[0][b"SUM(b)"] == 3 * 64 + 5 != 3 * 63 + 5           # six count bits clamped at 63
    c = next(c for c in sc.cases("multiplicity") if c.name == "multiplicity/agg/65536")
    assert c.rows_out(0)[0][b"SUM(b)"] == 3 * 65536 + 5                       # (65536 & 0xFFFF == 0: the record's key would have gone unseen)


def test_wrap_cases_follow_the_arrival_order_and_nothing_is_refused():
    """the same values, the float first or last: the reference's int64 wraps ahead of the float only -- two answers, 2^64 apart"""
    assert not any(sc.REFUSED in c.want() for c in sc.all_cases())
    by = {c.name: c for c in sc.cases("values")}
    first = lambda n: by[n].rows_out(0)[0][b"SUM(v)"]
    assert first("values/wrap/before_float") == -(2.0 ** 63) + 2.0 ** 40 and first("values/wrap/float_first") == 2.0 ** 63 + 2.0 ** 40
    blind = sorted(c.name for c in sc.all_cases() if c.notes.get("f32"))
    assert blind == ["grid/normalize_second_trip", "values/float/carry_out_of_every_digit", "values/float/subnormal"]


def test_limit_cases_hold_exactly_the_limit_and_one_more():
    for c in sc.cases("keys"):
        if "over" in c.notes:
            what = c.name.rsplit("/", 1)[1]
            n = sc.LIM[c.notes["limit"]]
            assert (sc.plan_counts(c.sql)[what], sc.plan_counts(c.notes["over"])[what]) == (n, n + 1), c.name
            assert all(sc.plan_counts(c.sql)[k] <= sc.LIM[v] for k, v in sc.LIMIT_OF.items()), c.name


def test_the_scaled_answer_is_the_oracle_s_at_small_repeat_counts():
    """grid/second_trip repeats one integer-only block: its answer is built from the oracle's for one block and for the tail"""
    for repeat in (1, 2, 5):
        c = sc.ScaledCase("grid/probe", repeat, None, {})
        t = osp.Task(sc.GRID_SQL)
        assert [t.do(c.steps[0].oracle_bytes()), t.timer()] == c.want(), repeat


def _ref_answers(c):
    r = ref_sp.RefSp(c.sql, str_conv=c.str_conv)
    try:
        assert r.ok, c.name
        return c.run(r)
    finally:
        r.close()


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.skipif(not ref_sp.available(), reason="oracle/_ref/ref_sp not built (no reference tree)")
def test_oracle_answers_are_the_reference_binary_s(group):
    """every case the reference binary can take (all but grid/second_trip, whose answer is scaled: its small repeat counts stand in)"""
    cs = [c for c in sc.cases(group) if c.ref]
    if group == "grid":
        cs += [sc.ScaledCase("grid/probe/%d" % r, r, None, {}) for r in (1, 3)]
    for c in cs:
        assert _ref_answers(c) == c.want(), c.name


def test_oracle_answers_are_the_committed_digests():
    kat = json.load(open(os.path.join(HERE, "golden", "sp_edges_kat.json")))
    cs = sc.all_cases()
    assert [k["case"] for k in kat["cases"]] == [c.name for c in cs]
    for k, c in zip(kat["cases"], cs):
        assert c.digest() == k, c.name

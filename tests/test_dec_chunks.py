"""The named cases of tests/dec_chunks.py sit on the edges they are named for (each case's predicate, computed from the chunk and the
oracle's answer alone), the oracle's answers are the reference's (oracle/_ref/ref_filters: the real filter_parser over the real
flb_parser_decoder.c) and the committed digests of tests/golden/dec_edges_kat.json -- the check that travels to where the reference is
not --, and a search over the oracle finds nothing that fills the decoders' scratch faster than the named worst cases.
tests/test_dec_edges_gpu.py runs the same cases on the device.

No case may be skipped, filtered out or marked as an expected failure: a case that cannot be built fails the test."""
import hashlib
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dec_chunks as dc
import ref_filters as rf

GROUPS = list(dc.GROUPS)


def test_limits_are_those_of_the_device_code():
    src = open(os.path.join(os.path.dirname(HERE), "fluent-bit_amd", "csrc", "dev.hpp")).read()
    m = re.search(r"constexpr int MAX_DEC_KEYS = (\d+), MAX_DEC_RULES = (\d+);", src)
    assert (int(m.group(1)), int(m.group(2))) == (dc.MAX_DEC_KEYS, dc.MAX_DEC_RULES)


def test_case_names_are_unique_and_every_group_has_cases():
    names = [c.name for c in dc.all_cases()]
    assert len(names) == len(set(names)) and all(dc.cases(g) for g in GROUPS)
    assert sum(1 for c in dc.cases("rules") if c.name.startswith("rules/random/")) == 60
    assert any(c.notes.get("bogus") for c in dc.cases("rules"))            # an action word the reference takes for "no action"


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_is_on_its_edge(group):
    for c in dc.cases(group):
        c.check()


def test_scratch_cases_cover_both_sides_of_the_first_room():
    cs = dc.cases("scratch")
    past = [c.name for c in cs if c.notes["past"]]
    assert any("field_json+as_json" in n for n in past) and any("/field_json/" in n for n in past) and "scratch/one_large" in past
    for c in cs:
        big = c.notes["big"]
        assert len(c.recs[big]) == c.max_row()
        if not c.notes["past"] and c.name.endswith(("/200", "/330", "/500")):
            assert c.max_row() <= 1024 + 64, c.name                          # (the line is 1 KB or less; the event around it adds its header)


def test_second_trip_cases_have_fewer_lanes_than_rows_at_any_halving():
    for c in dc.cases("grid"):
        if c.notes.get("trip"):
            assert len(c.recs) > 128 and all(r + 129 < len(c.recs) or r + 65 < len(c.recs) for r in c.notes["long"])
    default = [c for c in dc.cases("grid") if c.notes.get("trip") and not c.env]
    assert len(default) == 1 and default[0].max_row() > 932 * 1024             # 128 lanes x 6 regions x (3 x row + 4 KB) > 2^31


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.skipif(not rf.available(), reason="oracle/_ref/ref_filters not built (no reference tree)")
def test_oracle_answers_are_the_reference_binary_s(group):
    cs = dc.cases(group)
    got = rf.run([rf.parser_case(c.key, c.parsers, c.data, c.reserve, c.preserve) for c in cs])
    for c, (ret, out) in zip(cs, got):
        assert (ret, out) == (c.want()[0], c.out()), c.name


def test_oracle_answers_are_the_committed_digests():
    kat = json.load(open(os.path.join(HERE, "golden", "dec_edges_kat.json")))
    cs = dc.all_cases()
    assert [k["case"] for k in kat["cases"]] == [c.name for c in cs]
    for k, c in zip(kat["cases"], cs):
        assert hashlib.sha256(c.data).hexdigest() == k["chunk_sha256"], c.name
        assert (c.want()[0], hashlib.sha256(c.out()).hexdigest(), len(c.out())) == (k["ret"], k["sha256"], k["bytes"]), c.name


# ------------------------------------------------------------------------------------------ the search behind the named worst cases
def test_no_json_token_fills_the_scratch_faster_than_the_named_one():
    """all 69 906 array elements of up to 4 characters under a plain Decode_Field json, the 40 that grow most again under every rule
    order of the scratch cases: none grows the output by more per byte than `1e5,`"""
    toks = dc.json_tokens()
    assert dc.WORST_JSON in toks
    g = dc.json_growth(toks, "field_json")
    worst = g[toks.index(dc.WORST_JSON)]
    assert abs(worst - 3.25) < 1e-9 and max(g) <= worst                      # the string itself + a 9-byte double per 4 bytes of text
    top = [t for _, t in sorted(zip(g, toks), reverse=True)[:40]]
    if dc.WORST_JSON not in top:
        top.append(dc.WORST_JSON)
    for rs, ratio in (("as_json", 2.25), ("field_json+as_json", 4.5), ("as_escaped+field_json", 3.25)):
        g = dc.json_growth(top, rs)
        worst = g[top.index(dc.WORST_JSON)]
        assert abs(worst - ratio) < 1e-9 and max(g) <= worst, rs


@pytest.mark.parametrize("fmt,named,ratio", [("logfmt", dc.WORST_LOGFMT, 5.5), ("ltsv", dc.WORST_LTSV, 11 / 3)])
def test_no_kv_pair_fills_the_parser_s_map_faster_than_the_named_one(fmt, named, ratio):
    """`a=<up to 3 characters of a number>` streams (and logfmt's bare key) under Types a:float"""
    pieces = dc.kv_pieces(fmt)
    g = dc.kv_growth(pieces, fmt)
    worst = g[pieces.index(named)]
    assert abs(worst - ratio) < 1e-9 and max(g) <= worst

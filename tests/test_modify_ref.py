"""The CPU model of filter_modify (tests/modify_model.py) against the answers of the real plugin, recorded by tools/gen_modify_golden.py
into tests/golden/modify_ref_cases.json: refusal and output bytes, every entry.  The file holds bytes only (the reference's processor
does not hand the callback's return code on) behind the processor's own pass over the unit's buffer (mm.processor_output): where the model
answers NOTOUCH that buffer is the input.  And the generator of tests/modify_chunks.py against the model alone: what the device fuzz relies on."""
import base64
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import modify_chunks as mc
import modify_model as mm

CASES = json.load(open(os.path.join(HERE, "golden", "modify_ref_cases.json")))["cases"]
REQUIRED = ["rule_remove_012", "rule_remove_wildcard_012", "rule_remove_regex_012", "rule_move_to_start_012", "rule_move_to_end_012",
            "rule_rename_grid", "rule_hard_rename_grid", "rule_copy_grid", "rule_hard_copy_grid", "rule_add_012", "rule_set_012",
            "rename_onto_existing_key", "copy_two_sources", "hard_copy_target_before_and_behind", "hard_rename_two_targets",
            "set_over_duplicates", "move_to_start_stable", "move_to_end_stable", "prefix_remove_wildcard", "prefix_move_to_start",
            "prefix_move_to_end", "three_tokens_set_is_rename",
            "cond_key_exists", "cond_key_does_not_exist", "cond_a_key_matches", "cond_no_key_matches", "cond_key_value_equals",
            "cond_key_value_does_not_equal", "cond_key_value_matches", "cond_key_value_does_not_match",
            "cond_matching_keys_have_matching_values", "cond_matching_keys_do_not_have_matching_values",
            "cond_key_twice_last_wins", "cond_key_bin_only", "cond_equals_value_types", "cond_matches_value_types",
            "cond_a_key_matches_key_types", "cond_accessor_ends_on_index", "cond_accessor_ends_on_key", "cond_two_one_false",
            "keys_remove", "keys_rename_other", "keys_remove_regex_true", "keys_remove_regex_k", "keys_move_to_end",
            "key_nul_remove", "key_nul_wildcard", "body_map16", "body_map32", "non_canonical_entries", "non_canonical_none_applied",
            "non_canonical_metadata",
            "prefix_short_key_before_rule", "prefix_short_key_after_set", "prefix_short_key_through_entries",
            "prefix_short_key_through_entries_after_set", "prefix_short_key_repack_changes_bytes_after_set",
            "legacy_rows", "group_markers", "bad_time", "non_map_body_first", "non_map_body_middle", "garbage_reserved_byte",
            "garbage_cut_record", "garbage_cut_on_field_boundary", "garbage_cut_behind_header", "nothing_applies", "empty_map_add",
            "property_names_other_case", "unknown_property", "four_tokens", "repeated_rule_name"]
# no case the reference leaves undefined is recorded: none may have died
UNDEFINED = []


def test_the_recorded_set_is_complete():
    names = [c["name"] for c in CASES]
    assert not [n for n in REQUIRED + UNDEFINED if n not in names]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert sorted(c) in (["in", "name", "out", "props"], ["in", "name", "props", "refused"]), c["name"]
        assert c.get("refused") is True or c.get("out") is not None, c["name"]
    refused = [c["name"] for c in CASES if c.get("refused")]
    assert sorted(refused) == ["four_tokens", "one_token_two_token_rule", "rule_add_if_not_present_012", "two_tokens_one_token_rule", "unknown_condition",
                               "unknown_property"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_plugin(case):
    props = [tuple(p) for p in case["props"]]
    data = base64.b64decode(case["in"])
    if case.get("refused"):
        with pytest.raises(ValueError):
            mm.Model(props)
        return
    m = mm.Model(props)
    ret, out = m.filter(data)
    assert m.stats.get("overread", 0) == 0                   # every recorded compare is defined
    want = base64.b64decode(case["out"])
    assert mm.processor_output(out if ret == m.MODIFIED else data) == want


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_front_end_reproduces_the_plugin(case):
    """the product's configuration front end (host only): it starts where the real filter started"""
    g = flbamd_loader.load()
    props = [tuple(p) for p in case["props"]]
    if case.get("refused"):
        with pytest.raises(ValueError):
            g.modify_parse_check(props)
    else:
        assert g.modify_parse_check(props) == mm.describe(mm.parse(props))


def test_the_fuzz_generator_meets_its_floors():
    """the model alone over the chunks tests/test_modify_gpu.py::test_fuzz draws"""
    rows = {"rebuilt": 0, "raw": 0}
    rules, true, false = {}, {}, {}
    noncanon = 0
    for seed in mc.FUZZ_SEEDS:
        r = random.Random(seed)
        for _ in range(40):
            props = mc.rnd_program(r)
            m = mm.Model(props)                               # no drawn program is refused
            for _ in range(3):
                data = b"".join(mc.rnd_record(r) for _ in range(r.randrange(1, 61)))
                m.filter(data)
                noncanon += mc.noncanonical_key_headers(data)
            assert m.stats.get("overread", 0) == 0, props
            for k in rows:
                rows[k] += m.stats.get(k, 0)
            for acc, key in ((rules, "rule_applied"), (true, "cond_true"), (false, "cond_false")):
                for t, n in m.stats.get(key, {}).items():
                    acc[t] = acc.get(t, 0) + n
    total = rows["rebuilt"] + rows["raw"]
    assert rows["rebuilt"] * 4 >= total and rows["raw"] * 4 >= total, rows
    assert all(rules.get(t, 0) >= 20 for t in range(11)), rules
    assert all(true.get(t, 0) >= 20 and false.get(t, 0) >= 20 for t in range(10)), (true, false)
    assert noncanon >= 100

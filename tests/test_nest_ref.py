"""The CPU model of filter_nest (tests/nest_model.py) against the answers of the real plugin, recorded by tools/gen_nest_golden.py into
tests/golden/nest_ref_cases.json: refusal and output bytes, every entry.  The file holds bytes only (the reference's processor does not
hand the callback's return code on): where the model answers NOTOUCH the processor handed its input through, the records its
decoder takes."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import modify_model as mm
import nest_model as nm

CASES = json.load(open(os.path.join(HERE, "golden", "nest_ref_cases.json")))["cases"]
REQUIRED = ["rt_single", "rt_multi_nest", "rt_multi_lift", "rt_add_prefix",
            "operation_prefix_words", "unknown_property", "both_prefixes", "last_key_wins", "nest_under_on_lift", "no_wildcards",
            "nest_without_key", "lift_without_key",
            "nest_exact_and_prefix", "nest_star", "nest_bin_key_with_prefix", "nest_bin_key_no_prefix", "nest_remove_prefix_partial",
            "nest_short_key_overread_hit", "nest_short_key_overread_miss", "nest_none_match_next_to_match", "nest_non_canonical",
            "lift_plain", "lift_add_prefix", "lift_remove_prefix", "lift_value_not_map", "lift_duplicate_keys", "lift_empty_inner_map",
            "lift_inner_int_key_no_prefix", "lift_nested_two_levels",
            "metadata", "legacy_rows", "group_markers", "non_map_body", "garbage_reserved_byte", "garbage_cut_record",
            "empty_chunk_of_empty_maps", "bad_time_modified", "bad_time_unmodified"]
# the two cases the reference leaves undefined: recorded, never compared in bytes; only these may have died
UNDEFINED = ["undef_remove_prefix_short_key", "undef_lift_int_key_with_prefix"]


def test_the_recorded_set_is_complete():
    names = [c["name"] for c in CASES]
    assert not [n for n in REQUIRED + UNDEFINED if n not in names]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert bool(c.get("undefined")) == (c["name"] in UNDEFINED)
        if c.get("crashed"):
            assert c["name"] in UNDEFINED
        else:
            assert c.get("refused") or c.get("out") is not None, c["name"]
    refused = [c["name"] for c in CASES if c.get("refused")]
    assert sorted(refused) == ["both_prefixes", "operation_prefix_words_Nest", "same_property_twice_key", "same_property_twice_operation",
                               "same_property_twice_prefix", "unknown_property"]


def decodable(data):
    """what the processor hands back of a chunk the filter did not touch"""
    p = 0
    while p < len(data):
        try:
            end, skip, *_ = mm.decode_event(data, p)
        except mm.Bad:
            break
        assert not skip
        p = end
    return data[:p]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_plugin(case):
    props = [tuple(p) for p in case["props"]]
    data = base64.b64decode(case["in"])
    if case.get("refused"):
        with pytest.raises(ValueError):
            nm.Model(props)
        return
    m = nm.Model(props)
    ret, out = m.filter(data)
    if case.get("undefined"):
        # counted, not matched: the record goes out as it came
        assert (ret, out) == (m.MODIFIED, data) and m.counters()[2] == 1
        return
    assert m.counters()[1:] == (0, 0, 0)
    want = base64.b64decode(case["out"])
    assert (out if ret == m.MODIFIED else decodable(data)) == want

"""The CPU model of filter_type_converter (tests/typeconv_model.py) against the answers of the real plugin, recorded by
tools/gen_typeconv_golden.py into tests/golden/typeconv_ref_cases.json: refusal and output bytes, every entry.  The file holds bytes
only (the reference's processor does not hand the callback's return code on): where the model answers NOTOUCH the processor handed
its input through its group normalisation (modify_model.processor_output), the records its decoder takes."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import modify_model as mm
import typeconv_model as tm

CASES = json.load(open(os.path.join(HERE, "golden", "typeconv_ref_cases.json")))["cases"]
REQUIRED = [
    # tests/runtime/filter_type_converter.c
    "rt_str_to_int", "rt_str_to_float", "rt_str_to_hex", "rt_int_to_str", "rt_int_to_float", "rt_str_int_and_int_str", "rt_nest_key",
    # the front end
    "fe_names_without_case_and_repeat", "fe_two_tokens", "fe_two_tokens_next_to_a_good_rule", "fe_empty_value", "fe_four_tokens_skipped",
    "fe_four_tokens_only", "fe_unknown_type_next_to_a_good_rule", "fe_unknown_type_only", "fe_unknown_property", "fe_quoted_tokens",
    "fe_rule_order_is_configures", "fe_type_words_prefix", "fe_type_word_empty_is_int", "fe_unsupported_pairs_start",
    "fe_accessor_pre_dollar", "fe_accessor_tag", "fe_accessor_regex_id", "fe_accessor_dot", "fe_accessor_plain_name_with_dot",
    "fe_accessor_dollar_alone", "fe_accessor_refused_next_to_a_good_rule", "fe_accessor_refused_only",
    # lookups
    "lk_subkeys", "lk_subkeys_on_scalar_ignored", "lk_duplicate_top_level_key", "lk_duplicate_inner_key", "lk_bin_key_never_matches",
    "lk_to_key_equals_existing_key", "lk_two_rules_on_one_key", "lk_lookup_on_original_body", "lk_key_absent",
    # conversions
    "cv_str_to_int", "cv_str_to_uint", "cv_str_to_hex", "cv_str_to_float", "cv_str_to_bool", "cv_str_source_of_other_types",
    "cv_int_to_string", "cv_int_to_float", "cv_int_to_uint", "cv_uint_to_string", "cv_uint_to_float", "cv_uint_to_int",
    "cv_int_source_of_other_types", "cv_float_to_string", "cv_float_to_int", "cv_float_to_uint", "cv_float_source_of_other_types",
    # one call
    "call_notouch_no_conversion_succeeds", "call_one_success_marks_the_chunk", "call_non_canonical_entries", "call_wide_body_header",
    "metadata", "legacy_rows", "group_markers", "non_map_body", "garbage_reserved_byte", "garbage_cut_record",
    "cut_record_on_a_field_boundary", "bad_time", "bad_time_float", "empty_maps"]
# float -> int / uint of values the target cannot hold: C leaves them undefined
UNDEFINED = ["undef_float_to_int", "undef_float_to_uint"]
# config_rule unlinks a rule it never linked (type_converter.c:52, 95-100): the real plugin dies, create refuses
CRASHED = ["fe_unknown_type_next_to_a_good_rule", "fe_unknown_type_only", "fe_accessor_refused_next_to_a_good_rule", "fe_accessor_refused_only"]
REFUSED = ["fe_two_tokens", "fe_two_tokens_next_to_a_good_rule", "fe_empty_value", "fe_four_tokens_only", "fe_unknown_property"]


def test_the_recorded_set_is_complete():
    names = [c["name"] for c in CASES]
    assert not [n for n in REQUIRED + UNDEFINED if n not in names]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert bool(c.get("undefined")) == (c["name"] in UNDEFINED)
        assert bool(c.get("crashed")) == (c["name"] in CRASHED)
        assert c.get("refused") or c.get("crashed") or c.get("out") is not None, c["name"]
    assert sorted(c["name"] for c in CASES if c.get("refused")) == sorted(REFUSED)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_plugin(case):
    props = [tuple(p) for p in case["props"]]
    data = base64.b64decode(case["in"])
    if case.get("refused") or case.get("crashed"):
        with pytest.raises(ValueError):
            tm.Model(props)
        return
    m = tm.Model(props)
    ret, out = m.filter(data)
    if case.get("undefined"):
        # counted, not matched in bytes: every conversion of such a case is an undefined one
        assert ret == m.MODIFIED and m.counters()[2] == len(props) and m.counters()[:2] == (len(props), 0)
        return
    assert m.counters()[2:] == (0, 0)
    want = base64.b64decode(case["out"])
    assert (out if ret == m.MODIFIED else mm.processor_output(data)) == want


def test_what_the_recorded_bytes_settle():
    by = {c["name"]: c for c in CASES}

    def answer(name):
        c = by[name]
        m = tm.Model([tuple(p) for p in c["props"]])
        return m.filter(base64.b64decode(c["in"])), m
    # no conversion succeeds: NOTOUCH although a buffer was built; one success anywhere and every record goes out re-packed
    (ret, _), m = answer("call_notouch_no_conversion_succeeds")
    assert ret == m.NOTOUCH and m.counters() == (0, 2, 0, 0) and m.counts() == (3, 3)
    (ret, _), m = answer("call_one_success_marks_the_chunk")
    assert ret == m.MODIFIED and m.counters() == (1, 1, 0, 0)
    # a decoder error behind converted records: "encoder error", NOTOUCH
    for name in ("non_map_body", "garbage_reserved_byte", "garbage_cut_record"):
        (ret, _), m = answer(name)
        assert ret == m.NOTOUCH and m.counters()[0] >= 1, name
    (ret, _), m = answer("cut_record_on_a_field_boundary")
    assert ret == m.MODIFIED
    # the body header is map32, a refused time goes out as 0.0
    (ret, out), m = answer("bad_time")
    assert ret == m.MODIFIED and out.count(b"\x92\x92\xd7\x00" + bytes(8) + b"\x80\xdf\x00\x00\x00\x03") == 1
    # "0", "abc", "", "  -0" stay strings
    (ret, out), m = answer("cv_str_to_int")
    assert out.count(b"\xa2t0\xa10") == 1 and out.count(b"\xa2t1\xa3abc") == 1 and out.count(b"\xa2t2\xa0") == 1 and out.count(b"\xa2t3\xa4  -0") == 1

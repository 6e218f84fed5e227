"""The CPU model of filter_checklist (tests/checklist_model.py) against the recorded answers of the real plugin
(tests/golden/checklist_ref_cases.json, written by tools/gen_checklist_golden.py): cb_filter's return value and the output bytes of
every case, and the cases the recording must hold."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import checklist_model as cm

FIXTURE = os.path.join(HERE, "golden", "checklist_ref_cases.json")
CASES = json.load(open(FIXTURE))["cases"]
# the real plugin ran these; create refuses them: the loader reads buf[-1] at a NUL that begins a line
RAN_BUT_REFUSED = {"ld_nul_at_line_start"}
MUST_HOLD = [
    "rt_lookup_key", "rt_lookup_keys", "rt_records", "rt_ignore_case", "rt_mode_partial",
    "fe_no_record", "fe_duplicate_record_keys", "fe_record_replaces_lookup_key", "fe_record_value_kinds", "fe_record_one_token",
    "fe_mode_word_partial_case", "fe_mode_word_unknown_is_exact", "fe_no_file", "fe_missing_file", "fe_accessor_refused",
    "ld_empty_file", "ld_comments_only", "ld_crlf", "ld_last_line_without_newline",
    "ld_line_2045_in_the_middle", "ld_line_2046_in_the_middle", "ld_line_2047_in_the_middle",
    "ld_line_2045_last_with_newline", "ld_line_2046_last_with_newline", "ld_line_2047_last_with_newline",
    "ld_line_2045_last_without_newline", "ld_line_2046_last_without_newline", "ld_line_2047_last_without_newline",
    "ld_nul_in_the_middle_of_a_line", "ld_nul_at_line_start", "ld_entry_percent_exact", "ld_entry_percent_partial",
    "ld_ignore_case_high_bytes",
    "lk_value_types", "lk_duplicate_key_str_then_int", "lk_duplicate_key_int_then_str", "lk_subkey_path", "lk_path_ends_on_index",
    "lk_empty_str_value",
    "wr_keys_that_are_no_str", "wr_non_canonical_encodings", "wr_float32_and_ext", "wr_metadata", "wr_integer_and_float_time",
    "wr_time_the_encoder_refuses",
    "call_matches_only_at_the_end", "call_matches_only_at_the_start", "call_no_match", "call_group_markers_in_front_of_a_match",
    "call_group_markers_in_front_of_an_unmatched_record", "call_garbage_reserved_byte", "call_garbage_cut_record", "call_empty_chunk",
]


def model_of(case):
    files = {b"@LIST@": base64.b64decode(case["list"])} if case["list"] is not None else {}
    return cm.Model([tuple(p) for p in case["props"]], files)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_recording(case):
    if case.get("refused") or case.get("crashed") or case["name"] in RAN_BUT_REFUSED:
        with pytest.raises(ValueError):
            model_of(case)
        return
    ret, out = model_of(case).filter(base64.b64decode(case["in"]))
    assert ret == case["ret"]
    assert out == (base64.b64decode(case["out"]) if case["out"] is not None else None)


def test_the_recording_holds_the_cases_it_must():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert not [n for n in MUST_HOLD if n not in names]
    assert os.path.getsize(FIXTURE) < 128 * 1024
    # both answers, both modes, refusals and the one configuration at which the recording host died
    by = {c["name"]: c for c in CASES}
    assert {c.get("ret") for c in CASES} >= {1, 2}
    assert by["fe_accessor_refused"].get("crashed") and by["fe_record_one_token"].get("refused")
    assert sum(1 for c in CASES if ["mode", "partial"] in c["props"]) >= 5


def test_what_the_recording_showed():
    by = {c["name"]: c for c in CASES}
    # the value of a `record` is the LAST entry of the split, not everything behind the key
    out = base64.b64decode(by["fe_record_value_is_last_entry"]["out"])
    assert b"\xa1k\xa3val" in out and b"\xa1q\xa6c  d e" in out
    # a property that is not repeatable is refused when it is set twice
    assert by["fe_mode_set_twice"].get("refused")
    # a line with a NUL in it that is not the last line stops the load: "zzz" behind it is not on the list, "la" is not either
    m = model_of(by["ld_nul_in_the_middle_of_a_line"])
    assert (m.cfg.entries, m.cfg.status, m.cfg.stop_line) == ([b"abc"], cm.STOPPED, 1)
    m = model_of(by["ld_nul_in_the_last_line_without_newline"])
    assert (m.cfg.entries, m.cfg.status) == ([b"abc", b"la"], cm.OK)
    # a final line of exactly 2046 bytes without a newline stops the load, one of 2045 is an entry
    assert model_of(by["ld_line_2046_last_without_newline"]).cfg.status == cm.STOPPED
    assert len(model_of(by["ld_line_2045_last_without_newline"]).cfg.entries) == 2
    # a first record that matched and was rolled back goes out raw with the span in front of the next match
    c = by["wr_refused_first_record_then_a_match"]
    assert base64.b64decode(c["out"]).startswith(base64.b64decode(c["in"])[:20]) and c["ret"] == 1
    assert by["wr_refused_first_record_then_nothing"]["ret"] == 2

"""The CPU model of filter_multiline (tests/mlfilter_model.py) against the recorded answers of the real plugin
(tests/golden/mlfilter_ref_cases.json, tools/gen_mlfilter_golden.py): every case, every call, return value and bytes.  Configurations
the reference starts and this project refuses (buffered mode, partial_message, several parsers) are the documented deviations: the
model must refuse them, and a case the reference refuses must be refused too."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mlfilter_chunks as mc
import mlfilter_model as mlm
import modify_model as mm

CASES = json.load(open(os.path.join(HERE, "golden", "mlfilter_ref_cases.json")))["cases"]
# started by the reference, refused here
NOT_BUILT = {"fe_mode_partial_message": "partial_message", "fe_two_parsers": "more than one", "fe_two_parser_lines": "more than one"}


def model_of(case, **kw):
    limit = mlm.DEFAULT_LIMIT if case["limit"] is None else int(case["limit"])
    return mlm.Model([tuple(p) for p in case["props"]], {p["name"]: p for p in case["parsers"]}, limit, **kw)


def records(buf):
    out, p = [], 0
    while p < len(buf):
        o = mm.unpack(buf, p)
        out.append(buf[p:o.end])
        p = o.end
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_recording(case):
    if case.get("refused") or case["name"] in NOT_BUILT:
        with pytest.raises(mlm.Refused) as e:
            model_of(case)
        if case["name"] in NOT_BUILT:
            assert NOT_BUILT[case["name"]] in str(e.value) and not case.get("refused")
        return
    # a case the device hands back at run time: the model WITHOUT the hand-back reproduces the reference, the model with it answers -1
    m = model_of(case, hand_back_empty_start=not case.get("handed_back"))
    assert len(case["rets"]) == len(case["calls"])
    for i, (data, ret, out) in enumerate(zip(case["calls"], case["rets"], case["outs"])):
        got = m.filter(base64.b64decode(data))
        want = (ret, base64.b64decode(out) if out is not None else None)
        assert got[0] == want[0], (i, got[0], want[0])
        assert got == want, (i, records(got[1] or b""), records(want[1] or b""))
        assert m.counters()[2:] == (0, 0)


def test_a_start_with_an_empty_text_is_handed_back():
    case = [c for c in CASES if c.get("handed_back")][0]
    m = model_of(case)
    assert m.filter(base64.b64decode(case["calls"][0])) == (-1, None) and m.counters() == (0, 0, 1, 0) and m.state_of() == -1 and m.counts() == (0, 0)
    # the call that follows holds no such record: it is taken, from the state the stream had before
    assert m.filter(base64.b64decode(case["calls"][1])) == (case["rets"][1], base64.b64decode(case["outs"][1]))


def test_the_recording_holds_what_the_issue_lists():
    names = {c["name"] for c in CASES}
    need = ["rt_unbuffered", "builtin_java", "builtin_go", "builtin_python", "builtin_ruby", "nokey_record_without_the_key",
            "nokey_non_str_value_with_str_duplicate", "nokey_two_str_entries_in_the_first_record", "nokey_non_map_body", "canon_first_record",
            "state_continuation_opens_a_call", "state_not_processed_between_start_and_continuation", "call_empty_chunk",
            "call_undecodable_bytes_behind_the_records", "call_group_markers", "call_integer_and_float_time", "trunc_start", "trunc_continuation",
            "call_empty_content_as_continuation", "endswith", "endswith_negate", "equal", "equal_negate"]
    assert not [n for n in need if n not in names]
    assert os.path.getsize(os.path.join(HERE, "golden", "mlfilter_ref_cases.json")) < 128 * 1024


def test_the_reference_runtime_test_expectations():
    """flb_test_multiline_unbuffered: six pushes, six records, "panic" in the first"""
    case = [c for c in CASES if c["name"] == "rt_unbuffered"][0]
    outs = [r for o in case["outs"] for r in records(base64.b64decode(o))]
    assert len(case["calls"]) == len(mc.REF_UNBUFFERED) and len(outs) == mc.REF_UNBUFFERED_EXPECT["records"]
    assert mc.REF_UNBUFFERED_EXPECT["pattern"].encode() in outs[mc.REF_UNBUFFERED_EXPECT["pattern_index"]]


def test_group_markers_do_not_reach_the_output():
    case = [c for c in CASES if c["name"] == "call_group_markers"][0]
    for o in case["outs"]:
        for r in records(base64.b64decode(o or "")):
            assert r[4:8] not in (b"\xff\xff\xff\xff", b"\xff\xff\xff\xfe")


MUTANTS = {"lastkey": "the last instead of the first matching key", "reset": "the state reset by a not-processed record", "map32": "the map32 body header",
           "nosep": "the separator left out on a continuation", "calltime": "the call's time instead of the first record's"}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_of_the_model_misses_a_recorded_case(mutant):
    """the recording tells these apart: a model with the mutation fails at least one case (so the device test, which compares the
    device with the recording, does too)"""
    missed = []
    for case in CASES:
        if case.get("refused") or case["name"] in NOT_BUILT:
            continue
        m = model_of(case, mutate=mutant, hand_back_empty_start=not case.get("handed_back"))
        for data, ret, out in zip(case["calls"], case["rets"], case["outs"]):
            if m.filter(base64.b64decode(data), (12345, 678)) != (ret, base64.b64decode(out) if out is not None else None):
                missed.append(case["name"])
                break
    assert missed, MUTANTS[mutant]

"""filter_expect's CPU model (tests/expect_model.py) against the recording of the real plugin (tests/golden/expect_ref_cases.json,
written by tools/gen_expect_golden.py): per case the return value, the output bytes, the plugin's "exception on rule ..." lines in
record order, the number of "expect check failed" lines and the exit request.  No device."""
import base64
import json
import os

import pytest

import expect_model as em

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "expect_ref_cases.json")))["cases"]
BY_NAME = {c["name"]: c for c in CASES}

# the cases the issue names: the recording has to hold every one of them
MUST_HOLD = (
    ["rt_base_configuration"] + ["rt_%s_%s" % (r, m) for r in em.RULE_NAMES[:5] for m in ("matched", "not_matched")] +
    ["rule_%s_warn" % r for r in em.RULE_NAMES[:5]] + ["types_%s_%s" % (r, a) for r in em.RULE_NAMES[:5] for a in ("warn", "result_key")] +
    ["acc_plain_exists", "acc_dollar_exists", "acc_pre_dollar_exists", "acc_tag_exists", "acc_subkeys_exists", "acc_ends_on_index_exists",
     "acc_refused", "dup_is_null", "dup_eq", "eq_one_token", "eq_empty_value", "eq_rest_of_the_line", "eq_val", "eq_prefix_va",
     "eq_longer_value", "action_warn", "action_WARN", "action_Exit", "action_RESULT_KEY", "action_explode", "action_set_twice",
     "result_key_set_twice", "unknown_property", "result_key_empty", "result_key_in_body", "numbering_action_between_rules", "no_rules_warn",
     "wr_keys_that_are_no_str", "wr_non_canonical_encodings", "wr_float32_and_ext", "wr_metadata", "wr_integer_and_float_time",
     "wr_time_the_encoder_refuses_first", "wr_time_the_encoder_refuses_middle", "wr_time_the_encoder_refuses_last",
     "wr_float_time_minus_three", "groups_warn", "groups_result_key"] +
    ["call_%s_%s" % (c, a) for c in ("empty_chunk", "garbage_reserved_byte", "cut_record") for a in em.ACTIONS])


def test_recording_holds_the_named_cases():
    assert [n for n in MUST_HOLD if n not in BY_NAME] == []
    ran = [c for c in CASES if "ret" in c]
    assert {c["ret"] for c in ran} == {em.Model.MODIFIED, em.Model.NOTOUCH}
    assert any(c.get("refused") for c in CASES)
    actions = set()
    for c in ran:
        actions.add(em.parse([tuple(p) for p in c["props"]]).action)
    assert actions == {em.WARN, em.EXIT, em.RESULT_KEY}
    assert any(c["exit_status"] == 255 for c in ran) and any(c["exceptions"] for c in ran)
    assert os.path.getsize(os.path.join(HERE, "golden", "expect_ref_cases.json")) < 128 * 1024


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_recording(case):
    props = [tuple(p) for p in case["props"]]
    if case.get("refused") or case.get("crashed"):
        with pytest.raises(ValueError):
            em.parse(props)
        return
    data = base64.b64decode(case["in"])
    m = em.Model(props)
    ret, out = m.filter(data)
    assert ret == case["ret"]
    assert out == (base64.b64decode(case["out"]) if case["out"] is not None else None)
    assert m.exit_status == case["exit_status"]
    want = [base64.b64decode(x) + b"\n" for x in case["exceptions"]]
    assert m.texts(data) == want
    # `warn` logs one "expect check failed" per failing record; the other actions log none
    assert case["check_failed"] == (len(m.failures) if m.cfg.action == em.WARN else 0)

"""The CPU model of filter_record_modifier (tests/recmod_model.py) against the answers of the real plugin, recorded by
tools/gen_recmod_golden.py into tests/golden/recmod_ref_cases.json: output bytes and return code, every entry"""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import recmod_model as rm

CASES = json.load(open(os.path.join(HERE, "golden", "recmod_ref_cases.json")))["cases"]
REQUIRED = ["rt_json_long", "rt_remove_keys", "rt_records", "rt_allowlist_keys", "rt_whitelist_keys", "rt_multiple", "rt_exclusive_setting",
            "rt_uuid_key", "case_fold", "prefix", "star_remove", "star_allow", "bin_int_remove", "bin_int_allow", "empty_map_record",
            "loses_all_next_to_kept", "all_lose_all", "non_map_body", "legacy_rows", "metadata", "non_canonical", "record_one_token",
            "record_quoted", "garbage_reserved_byte", "garbage_cut_record", "notouch"]


def test_the_recorded_set_is_complete():
    names = [c["name"] for c in CASES]
    assert not [n for n in REQUIRED if n not in names]
    assert len(set(names)) == len(names)
    # every entry but the one the product refuses on purpose carries an answer of the real plugin
    for c in CASES:
        assert c.get("refused_here") or c.get("refused") or c["ret"] in (1, 2), c["name"]
    assert any(c.get("ret") == 1 for c in CASES) and any(c.get("ret") == 2 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_plugin(case):
    props = [tuple(p) for p in case["props"]]
    data = base64.b64decode(case["in"])
    if case.get("refused") or case.get("refused_here"):
        with pytest.raises(ValueError):
            rm.Model(props)
        return
    ret, out = rm.Model(props).filter(data)
    assert ret == case["ret"]
    assert out == (base64.b64decode(case["out"]) if case["out"] is not None else None)

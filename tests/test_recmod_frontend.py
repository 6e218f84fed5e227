"""filter_record_modifier's configuration on the host (csrc/recmod.cpp flbgpu_record_modifier_parse_check, no device needed) against
the CPU model's restatement of the config map and configure() (tests/recmod_model.py)"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import recmod_model as rm

CASES = json.load(open(os.path.join(HERE, "golden", "recmod_ref_cases.json")))["cases"]


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def product(g, props):
    try:
        return g.record_modifier_parse_check(props)
    except ValueError:
        return None


def model(props):
    try:
        return rm.describe(rm.parse(props))
    except ValueError:
        return None


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_programs(g, case):
    props = [tuple(p) for p in case["props"]]
    want = model(props)
    assert (want is None) == bool(case.get("refused") or case.get("refused_here"))
    assert product(g, props) == want


QUIRKS = [
    # names without case
    [("RECORD", "a b"), ("record", "c d"), ("ReMoVe_KeY", "x")],
    [("ALLOWLIST_KEY", "x"), ("whitelist_KEY", "y")],
    # Whitelist_key joins the allowlist, behind the Allowlist_key entries wherever it stands
    [("Whitelist_key", "w1"), ("Allowlist_key", "a1"), ("Whitelist_key", "w2"), ("Allowlist_key", "a2")],
    # prefixes
    [("Remove_key", "a*")],
    [("Remove_key", "*")],
    [("Allowlist_key", "*")],
    [("Remove_key", "a**")],
    [("Remove_key", "a*b")],
    [("Remove_key", "MiXed*"), ("Remove_key", "É")],
    # quoted Record values
    [("Record", 'k "v w"')],
    [("Record", '"a b" c')],
    [("Record", '"a b" "c d"')],
    [("Record", 'q "x \\" y"')],
    [("Record", '"a b"c d')],
    [("Record", 'k "unterminated v')],
    [("Record", "k 'v w'")],
    [("Record", '"" v')],
    [("Record", "   k    v   ")],
    [("Record", "k v ")],
    # one token, none, more than two
    [("Record", "lonely")],
    [("Record", "lonely ")],
    [("Record", "")],
    [("Record", "   ")],
    [("Record", '"')],
    [("Record", "a b c")],
    [("Record", "a b c d"), ("Record", "k v")],
    [("Record", 'a "b c" d')],
    # nothing at all
    [],
]


@pytest.mark.parametrize("props", QUIRKS, ids=[str(i) for i in range(len(QUIRKS))])
def test_quirks(g, props):
    assert product(g, props) == model(props)


def test_quirk_answers():
    assert model([("Whitelist_key", "w1"), ("Allowlist_key", "a1")]) == "allow;Ke,6131;Ke,7731"
    assert model([("Remove_key", "a*")]) == "remove;Kp,61"
    assert model([("Remove_key", "*")]) == "remove;Kp,"
    assert model([("Record", 'k "v w"')]) == "none;R6b,762077"
    assert model([("Record", "a b c")]) == "none"
    assert model([("Record", "lonely")]) is None
    assert model([]) == "none"


REFUSED = [
    [("Remove_key", "a"), ("Allowlist_key", "b")],
    [("Remove_key", "a"), ("Whitelist_key", "b")],
    [("Uuid_key", "id")],
    [("uuid_KEY", "id"), ("Record", "a b")],
    [("Remove_key", "")],
    [("Allowlist_key", "")],
    [("Whitelist_key", "")],
    [("Remove_key", "k%d" % i) for i in range(65)],
    [("Allowlist_key", "k%d" % i) for i in range(33)] + [("Whitelist_key", "w%d" % i) for i in range(32)],
    [("Record", "k%d v" % i) for i in range(65)],
    [("Remove_key", "x" * 40000)],
    [("No_such_property", "x")],
]


@pytest.mark.parametrize("props", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refusals(g, props):
    assert model(props) is None
    with pytest.raises(ValueError):
        g.record_modifier_parse_check(props)
    assert g.last_error().startswith("filter_record_modifier: ")


def test_caps_are_inclusive(g):
    for props in ([("Remove_key", "k%d" % i) for i in range(64)], [("Record", "k%d v" % i) for i in range(64)],
                  [("Record", "k%d v" % i) for i in range(64)] + [("Record", "a b c")] * 5):
        assert product(g, props) == model(props) is not None

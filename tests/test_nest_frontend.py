"""filter_nest's configuration on the host (csrc/nest.cpp flbgpu_nest_parse_check, no device needed) against the CPU model's
restatement of the config map and configure() (tests/nest_model.py)"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import nest_model as nm

CASES = json.load(open(os.path.join(HERE, "golden", "nest_ref_cases.json")))["cases"]


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def product(g, props):
    try:
        return g.nest_parse_check(props)
    except ValueError:
        return None


def model(props):
    try:
        return nm.describe(nm.parse(props))
    except ValueError:
        return None


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_programs(g, case):
    props = [tuple(p) for p in case["props"]]
    want = model(props)
    assert (want is None) == bool(case.get("refused"))
    assert product(g, props) == want


N = [("Operation", "nest")]
QUIRKS = [
    # names without case
    [("OPERATION", "nest"), ("wildCARD", "a"), ("NEST_under", "k"), ("ADD_PREFIX", "p")],
    [("operation", "lift"), ("NESTED_UNDER", "k"), ("remove_PREFIX", "p")],
    # the first four bytes of Operation decide, with their case
    [("Operation", "nested")],
    [("Operation", "lifting")],
    [("Operation", "nestXYZ")],
    # both names set the one key for either operation, the last one wins; an empty key is a key
    N + [("Nest_under", "a"), ("Nested_under", "b")],
    N + [("Nested_under", "b"), ("Nest_under", "a")],
    [("Operation", "lift"), ("Nest_under", "a")],
    N + [("Nest_under", "")],
    N,
    # an empty prefix is a prefix
    N + [("Add_prefix", "")],
    N + [("Remove_prefix", "")],
    # wildcards: a trailing star is cut off, a star elsewhere is a byte
    N + [("Wildcard", "a*")],
    N + [("Wildcard", "*")],
    N + [("Wildcard", "a**")],
    N + [("Wildcard", "a*b")],
    N + [("Wildcard", "x"), ("Wildcard", "x"), ("Wildcard", "É*")],
    [("Operation", "lift"), ("Wildcard", "ignored*")],
]


@pytest.mark.parametrize("props", QUIRKS, ids=[str(i) for i in range(len(QUIRKS))])
def test_quirks(g, props):
    assert product(g, props) == model(props) is not None


def test_quirk_answers():
    assert model([("Operation", "nested"), ("Wildcard", "a*"), ("Wildcard", "b"), ("Nest_under", "k")]) == "nest;K6b;Pn,;Wp,61;We,62"
    assert model([("Operation", "lifting"), ("Nest_under", "k"), ("Add_prefix", "p_")]) == "lift;K6b;Pa,705f"
    assert model([("Operation", "lift"), ("Remove_prefix", "p_")]) == "lift;K-;Pr,705f"
    assert model(N + [("Nest_under", "")]) == "nest;K;Pn,"
    assert model(N + [("Wildcard", "*")]) == "nest;K-;Pn,;Wp,"
    assert model(N + [("Nest_under", "a"), ("Nested_under", "b")]) == "nest;K62;Pn,"
    assert model([("Operation", "nest"), ("Operation", "lift")]) is None
    assert model([("Operation", "Nest")]) is None


REFUSED = [
    [("Operation", "Nest")],
    [("Operation", "NEST")],
    [("Operation", "nes")],
    [("Operation", "")],
    [("Operation", " nest")],
    # only Wildcard may repeat: the config map refuses another name that is set twice, whatever its case
    [("Operation", "nest"), ("Operation", "lift")],
    [("Operation", "nest"), ("OPERATION", "nest")],
    N + [("Nest_under", "a"), ("nest_under", "b")],
    N + [("Nested_under", "a"), ("Nested_under", "a")],
    N + [("Add_prefix", "a"), ("Add_prefix", "b")],
    N + [("Remove_prefix", "a"), ("Remove_prefix", "b")],
    # a missing Operation: the reference reads an uninitialised field
    [],
    [("Wildcard", "a"), ("Nest_under", "k")],
    # an empty Wildcard: the reference reads key[-1]
    N + [("Wildcard", "")],
    N + [("Add_prefix", "a"), ("Remove_prefix", "a")],
    N + [("Remove_prefix", "a"), ("Wildcard", "x"), ("Add_prefix", "b")],
    # configure() knows Prefix_with, the config map does not
    N + [("Prefix_with", "p")],
    N + [("No_such_property", "x")],
    N + [("Wildcard", "k%d" % i) for i in range(65)],
    N + [("Wildcard", "x" * 40000)],
    N + [("Nest_under", "x" * 20000), ("Add_prefix", "y" * 20000)],
]


@pytest.mark.parametrize("props", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refusals(g, props):
    assert model(props) is None
    with pytest.raises(ValueError):
        g.nest_parse_check(props)
    assert g.last_error().startswith("filter_nest: ")


def test_caps_are_inclusive(g):
    for props in (N + [("Wildcard", "k%d" % i) for i in range(64)],
                  N + [("Wildcard", "x" * 32768)],
                  N + [("Wildcard", "x" * 16384 + "*"), ("Nest_under", "k" * 8192), ("Add_prefix", "p" * 8192)]):
        assert product(g, props) == model(props) is not None
    for props in (N + [("Wildcard", "k%d" % i) for i in range(65)],
                  N + [("Wildcard", "x" * 32769)],
                  N + [("Wildcard", "x" * 16384 + "*"), ("Nest_under", "k" * 8192), ("Add_prefix", "p" * 8193)]):
        assert product(g, props) is None and model(props) is None

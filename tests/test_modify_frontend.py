"""filter_modify's configuration on the host (csrc/modify.cpp flbgpu_modify_parse_check, no device needed) against the CPU model's
restatement of setup() (tests/modify_model.py), and the model itself on the reference's runtime cases"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import modify_model as mm
import oracle_binding as ob
import synth

CASES = json.load(open(os.path.join(HERE, "golden", "modify_runtime_cases.json")))["cases"]


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def product(g, props):
    try:
        return g.modify_parse_check(props)
    except ValueError:
        return None


def model(props):
    try:
        return mm.describe(mm.parse(props))
    except ValueError:
        return None


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_runtime_case_programs(g, case):
    props = [tuple(p) for p in case["props"]]
    want = model(props)
    assert (want is None) == bool(case.get("refused"))      # invalid_wildcard (Remove_wildcard *s3) fails to start
    assert product(g, props) == want


QUIRKS = [
    # three tokens: a RENAME of the first to the last, whatever the property (modify.h:28-29)
    [("Set", "msg hello world")],
    [("Remove", "a b c")],
    [("Copy", "a b c")],
    # four tokens, zero tokens
    [("Set", "a b c d")],
    [("Set", "")],
    [("Set", "   ")],
    # quotes and escapes
    [("Set", '"a b" "c \\" d"')],
    [("Set", "'it''s' x")],
    [("Set", "'a\\'b' \"c\\\\d\"")],
    [("Set", '"a b"c d')],
    [("Set", '"unterminated x')],
    # leading blanks, the empty token of two trailing blanks, one trailing blank
    [("Add", "   k v")],
    [("Add", "k v  ")],
    [("Add", "k v ")],
    # property names are case-insensitive; unknown names and wrong token counts are refused
    [("sEt", "k v"), ("REMOVE", "x"), ("condition", "KEY_EXISTS k")],
    [("Frobnicate", "k v")],
    [("Remove", "k v")],
    [("Rename", "k")],
    [("Add_if_not_present", "k v")],
    # conditions: one token, every type, accessors
    [("Condition", "Key_exists")],
    [("Condition", "Key_exists $a['b'][0]"), ("Set", "x y")],
    [("Condition", "Key_exists $TAG"), ("Condition", "Key_exists $0"), ("Condition", "Key_exists x$y")],
    [("Condition", "Key_value_equals k")],
    [("Condition", "Key_value_matches k")],
    [("Condition", "A_key_matches ^a"), ("Condition", "No_key_matches ^b x")],
    [("Condition", "Matching_keys_have_matching_values ^a ^b")],
    [("Condition", "Matching_keys_do_not_have_matching_values ^a")],
    [("Condition", "No_such_condition k")],
    # Hard_copy onto itself; a value Onigmo refuses; look-ahead executed vs only compiled
    [("Hard_copy", "k k")],
    [("Hard_copy", "k K")],
    [("Set", "k [abc")],
    [("Set", "k (?=abc)x")],
    [("Remove_regex", "^(?!a)")],
    [("Condition", "Key_value_matches k (?<=a)b")],
    # a condition pattern Onigmo refuses: cb_init takes it and the first record dereferences the NULL regex -- refused here
    [("Condition", "Key_value_matches k [abc")],
    [("Condition", "A_key_matches (abc")],
    [("Remove_regex", "/^A/i")],
]


@pytest.mark.parametrize("props", QUIRKS, ids=[str(i) for i in range(len(QUIRKS))])
def test_quirks(g, props):
    assert product(g, props) == model(props)


def test_pinned_quirks(g):
    assert product(g, [("Set", "msg hello world")]) == "R0,%s,%s" % (b"msg".hex(), b"world".hex())
    assert product(g, [("Add", "k v  ")]) == "R0,%s," % b"k".hex()
    assert product(g, [("Set", "a b c d")]) is None
    assert product(g, [("Condition", "Key_exists")]) is None
    assert product(g, [("Hard_copy", "k k")]) is None
    assert product(g, [("Set", "k [abc")]) is None
    assert product(g, [("Set", "k (?=abc)x")]) is not None
    assert product(g, [("Remove_regex", "^(?!a)")]) is None


def test_caps(g):
    assert product(g, [("Add", "k%d v" % i) for i in range(64)]) is not None
    assert product(g, [("Add", "k%d v" % i) for i in range(65)]) is None
    assert product(g, [("Condition", "Key_exists k%d" % i) for i in range(32)]) is not None
    assert product(g, [("Condition", "Key_exists k%d" % i) for i in range(33)]) is None
    with pytest.raises(ValueError, match="more than 64 rules"):
        g.modify_parse_check([("Add", "k%d v" % i) for i in range(65)])
    with pytest.raises(ValueError, match="not a regular expression"):
        g.modify_parse_check([("Remove_regex", "^(?!a)")])


def runtime_input(case):
    return b"".join(synth.mp([[synth.ext_ts(0, 0), {}], json.loads(p)[1]]) for p in case["inputs"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_runtime_case(case):
    """the model's output, rendered as out_lib renders it, holds the substring the reference's test expects (or as many records)"""
    if case.get("refused"):
        with pytest.raises(ValueError):
            mm.Model([tuple(p) for p in case["props"]])
        return
    m = mm.Model([tuple(p) for p in case["props"]])
    data = runtime_input(case)
    r, out = m.filter(data)
    out = data if r != m.MODIFIED else out
    if "expect_records" in case:
        assert ob.count_records(out) == case["expect_records"]
    js = ob.msgpack_to_json_format(out, 1, 0, b"date")
    text = js.decode() if isinstance(js, bytes) else str(js)
    for e in case["expect"]:
        assert e in text, (case["name"], text)

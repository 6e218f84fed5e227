"""filter_expect's configuration on the host (csrc/expect.cpp flbgpu_expect_parse_check and flbgpu_expect_text_check, no device needed)
against the CPU model's restatement of the config map and context_create (tests/expect_model.py): every recorded configuration, the
refusals, the caps, and the messages of the failures -- against the model's strings and against the lines the real plugin logged."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import expect_model as em

CASES = json.load(open(os.path.join(HERE, "golden", "expect_ref_cases.json")))["cases"]


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def product(g, props):
    try:
        return g.expect_parse_check(props)
    except ValueError:
        return None


def model(props):
    try:
        return em.describe(em.parse(props))
    except ValueError:
        return None


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_configurations(g, case):
    props = [tuple(p) for p in case["props"]]
    want = model(props)
    # where the real plugin did not start, or died, create refuses
    assert (want is None) == bool(case.get("refused") or case.get("crashed"))
    assert product(g, props) == want
    if want is None:
        assert g.last_error().startswith("filter_expect: ")


@pytest.mark.parametrize("case", [c for c in CASES if c.get("exceptions")], ids=[c["name"] for c in CASES if c.get("exceptions")])
def test_failure_texts(g, case):
    props = [tuple(p) for p in case["props"]]
    data = base64.b64decode(case["in"])
    m = em.Model(props)
    m.filter(data)
    got = [g.expect_text_check(props, f.rule.no, f.kind, f.vt, data[f.val_off:f.val_off + f.val_len]) for f in m.failures]
    assert got == m.texts(data)
    assert got == [base64.b64decode(x) + b"\n" for x in case["exceptions"]]


def test_the_line_says_what_was_configured(g):
    props = [("Key_Exists", "$m['a'][2]"), ("ACTION", "Result_Key"), ("key_val_eq", " log  a b  c "), ("result_key", "r"), ("key_not_exists", "$TAG"),
             ("key_val_is_null", "plain"), ("key_val_is_not_null", "")]
    assert g.expect_parse_check(props) == ("action=result_key;result_key=72;#0:key_exists:K6d.61[2];#1:action:-;#2:key_val_eq:K6c6f67:E" + b"a b  c ".hex() +
                                           ";#3:key_not_exists:-;#4:key_val_is_null:K706c61696e;#5:key_val_is_not_null:-") == model(props)
    assert g.expect_parse_check([]) == "action=warn;result_key=6d617463686564" == model([])
    # one word is the accessor and the expected text at once
    assert g.expect_parse_check([("key_val_eq", "$k")]) == "action=warn;result_key=6d617463686564;#0:key_val_eq:K6b:E246b"


def test_the_wording_is_the_reference_s(g):
    p = [("action", "warn"), ("key_val_eq", "$k val"), ("key_val_is_not_null", "$n")]
    # key_val_eq's not-found text names another rule (plugins/filter_expect/expect.c:366-373); the rule number counts `action`
    assert g.expect_text_check(p, 1, em.NOT_FOUND, em.VT_NONE) == b"exception on rule #1 'key_val_is_null', key '$k val' not found. Record content:\n"
    assert g.expect_text_check(p, 1, em.DIFFERENT, em.VT_STRING, b"va\0lue") == (
        b"exception on rule #1 'key_val_eq', key value 'va' is different than expected: 'val'. Record content:\n")
    assert g.expect_text_check(p, 2, em.WRONG_TYPE, em.VT_NULL) == (
        b"exception on rule #2 'key_val_is_not_null', key '$n' contains a value type 'null'. Record content:\n")
    assert g.expect_text_check(p, 2, em.WRONG_TYPE, em.VT_BINARY).count(b"'UNKNOWN'") == 1
    for rule in (0, 3):                                       # the action's rule cannot fail; there is no rule #3
        with pytest.raises(ValueError):
            g.expect_text_check(p, rule, em.NOT_FOUND, em.VT_NONE)


REFUSED = [
    [("nope", "1")], [("action", "warn"), ("ACTION", "warn")], [("result_key", "a"), ("Result_Key", "a")], [("action", "warning")], [("action", "")],
    [("key_val_eq", "")], [("key_val_eq", "   ")], [("key_exists", "$a['x")], [("key_exists", "$a[x]")], [("key_val_eq", "$a['x val")],
    [("key_exists", "${HOME}")], [("key_val_eq", "$a ${HOME}")], [("key_exists", "k" * 128)],
    [("key_val_eq", "$a b ${")], [("result_key", "${R}"), ("action", "result_key")],
    [("key_exists", "$k%d" % i) for i in range(65)], [("key_exists", "$k%d" % i) for i in range(64)] + [("action", "exit")],
    [("key_val_eq", "k " + "v" * 32768)], [("result_key", "r" * 65535)], [("result_key", "r" * 65536)],
]
STARTS = [
    [("key_exists", "$k%d" % i) for i in range(64)], [("key_exists", "$k%d" % i) for i in range(63)] + [("action", "exit")],
    [("key_exists", "$k%d" % i) for i in range(64)] + [("result_key", "r")], [("key_exists", "k" * 127)], [("key_exists", "")], [("key_exists", "$")],
    [("key_exists", "a.b")], [("key_exists", "$a.b")], [("key_val_eq", "k " + "v" * 30000)], [("result_key", "")], [("result_key", "r" * 30000)],
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_refused(g, i):
    assert product(g, REFUSED[i]) is None and model(REFUSED[i]) is None
    assert g.last_error().startswith("filter_expect: ")


@pytest.mark.parametrize("i", range(len(STARTS)))
def test_starts(g, i):
    assert product(g, STARTS[i]) == model(STARTS[i]) is not None


def test_caps(g):
    """64 rules start and 65 do not; a result_key of 65536 bytes is refused for its length, one of 65535 bytes for the table it would
    need (the table's 32768 bytes are the nearer limit); the table itself at 32768 / 32769 bytes"""
    assert product(g, REFUSED[15]) is None and "64 rules" in g.last_error()
    assert product(g, REFUSED[19]) is None and "65535" in g.last_error()
    assert product(g, REFUSED[18]) is None and "32768" in g.last_error()

    def table_props(nbytes):
        # 16 bytes of words, the packed "matched" (8), one rule of 32 bytes, the 4-byte key "k", the expected text
        return [("key_val_eq", "k " + "v" * (nbytes - 16 - 8 - 32 - 4))]
    assert em.table_bytes(em.parse(table_props(32768))) == 32768
    assert product(g, table_props(32768)) == model(table_props(32768)) is not None
    assert product(g, table_props(32769)) is None and model(table_props(32769)) is None and "32768" in g.last_error()

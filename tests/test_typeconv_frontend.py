"""filter_type_converter's configuration on the host (csrc/typeconv.cpp flbgpu_type_converter_parse_check, no device needed) against
the CPU model's restatement of the config map, config_rule and configure() (tests/typeconv_model.py)"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import typeconv_model as tm

CASES = json.load(open(os.path.join(HERE, "golden", "typeconv_ref_cases.json")))["cases"]


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def product(g, props):
    try:
        return g.type_converter_parse_check(props)
    except ValueError:
        return None


def model(props):
    try:
        return tm.describe(tm.parse(props))
    except ValueError:
        return None


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_programs(g, case):
    props = [tuple(p) for p in case["props"]]
    want = model(props)
    # where the real plugin did not start, or died, create refuses
    assert (want is None) == bool(case.get("refused") or case.get("crashed"))
    assert product(g, props) == want


def test_rules_are_regrouped_in_configures_order(g):
    props = [("float_key", "f f2 string"), ("uint_key", "u u2 string"), ("str_key", "s1 a int"), ("int_key", "i i2 float"),
             ("str_key", "s2 b hex"), ("float_key", "g g2 int")]
    assert g.type_converter_parse_check(props) == ("str>int,K7331,T61;str>hex,K7332,T62;int>float,K69,T6932;uint>string,K75,T7532;"
                                                   "float>string,K66,T6632;float>int,K67,T6732")


WORDS = {"": "int", "i": "int", "in": "int", "int": "int", "INT": "int", "u": "uint", "ui": "uint", "uint": "uint", "Uint": "uint",
         "f": "float", "fl": "float", "float": "float", "h": "hex", "he": "hex", "hex": "hex", "s": "string", "st": "string",
         "str": "string", "strin": "string", "string": "string", "b": "bool", "bo": "bool", "bool": "bool", "BOOL": "bool"}
UNKNOWN = ["integer", "strings", "ints", "uint8", "floats", "x", "double", "boolean", "hexa", "0", "t"]


@pytest.mark.parametrize("word", sorted(WORDS))
def test_type_word_is_a_prefix_of_the_first_name_it_fits(g, word):
    props = [("str_key", 'k t "%s"' % word)]
    assert g.type_converter_parse_check(props) == "str>%s,K6b,T74" % WORDS[word] == model(props)


@pytest.mark.parametrize("word", UNKNOWN)
def test_unknown_type_word_is_refused(g, word):
    # the reference dies at these (typeconv_model.Skip)
    for props in ([("str_key", "k t " + word)], [("str_key", "k t " + word), ("int_key", "i j string")]):
        assert product(g, props) is None and model(props) is None


QUIRKS = [
    # names without case, each may repeat
    [("STR_KEY", "a b int"), ("Str_key", "a c float"), ("INT_KEY", "a d string"), ("UINT_key", "a e string"), ("FLOAT_KEY", "a f string")],
    # a fourth entry is the rest of the line: the rule is skipped, the others stay
    [("str_key", "a b int and more"), ("int_key", "c d string")],
    [("str_key", "a b int  x"), ("str_key", "c d int")],
    # quoted tokens, a quoted empty type word
    [("str_key", '"a b" "c d" int')],
    [("str_key", 'a b ""')],
    [("str_key", '  a   b   int  ')],
    # pairs no conversion exists for are rules all the same
    [("str_key", "a b string"), ("int_key", "a b int"), ("int_key", "a b hex"), ("int_key", "a b bool"), ("uint_key", "a b uint"),
     ("uint_key", "a b hex"), ("float_key", "a b float"), ("float_key", "a b hex"), ("float_key", "a b bool")],
    # accessors
    [("str_key", "$a b int")],
    [("str_key", "$a['b']['c'] t int"), ("str_key", "$a['l'][3] t int"), ("str_key", "$a[0][1] t int")],
    [("str_key", "$a['it''s'] t int")],
    [("str_key", "$a['x.y'] t int")],
    [("str_key", "pre$key t int")],
    [("str_key", "pre$key['a t int")],                                  # the part behind is refused all the same
    [("str_key", "$TAG t int")],
    [("str_key", "$TAG[2] t int")],
    [("str_key", "$TAGS t int")],
    [("str_key", "$0 t int")],
    [("str_key", "$9x t int")],
    [("str_key", "$ t int")],
    [("str_key", "$a.b t int")],
    [("str_key", "$a.b['c t int")],                                     # the accessor ends at the '.': what follows is text
    [("str_key", "a.b t int")],
    [("str_key", "a$ t int")],
    [("str_key", "x t int")],
    [("str_key", "$a$b t int")],
    [("str_key", "$a,b t int")],
    # refused: an accessor the grammar refuses, limits
    [("str_key", "$a['x t int")],
    [("str_key", "$a[x] t int")],
    [("str_key", "$a['x']y t int")],
    [("str_key", "$a[1 t int")],
    [("str_key", "$-a t int")],
    [("str_key", "$" + "k" * 127 + " t int")],
    [("str_key", "$" + "k" * 128 + " t int")],
    [("str_key", "k" * 127 + " t int")],
    [("str_key", "k" * 128 + " t int")],
    [("str_key", "$a" + "['s']" * 8 + " t int")],
    [("str_key", "$a" + "['s']" * 9 + " t int")],
    [("str_key", "$a['" + "s" * 256 + "'] t int")],
    [("str_key", "$a['" + "s" * 257 + "'] t int")],
    # refused: nothing left, too few entries, unknown names
    [],
    [("str_key", "a b int extra")],
    [("str_key", "a b")],
    [("str_key", "a")],
    [("str_key", "")],
    [("str_key", "a b int"), ("int_key", "a b")],
    [("bool_key", "a b string")],
    [("str_key", "a b int"), ("Match", "*")],
    # limits of the table
    [("str_key", "k%d t%d int" % (i, i)) for i in range(64)],
    [("str_key", "k%d t%d int" % (i, i)) for i in range(65)],
    [("str_key", "k%d t%d int extra" % (i, i)) for i in range(100)] + [("str_key", "a b int")],      # skipped rules do not count
]


@pytest.mark.parametrize("i", range(len(QUIRKS)))
def test_quirks(g, i):
    assert product(g, QUIRKS[i]) == model(QUIRKS[i])


def test_what_the_quirks_decide():
    refused = [i for i, p in enumerate(QUIRKS) if model(p) is None]
    # a part the grammar refuses (also behind another part), the limits' first value over, nothing left, too few entries, unknown
    # names, the 65th rule
    assert refused == [12, 24, 26, 27, 28, 29, 30, 32, 34, 36, 38, 39, 40, 41, 42, 43, 44, 45, 46, 48]
    assert model([("str_key", "pre$key t int")]) == "str>int,K707265,T74"
    assert model([("str_key", "$TAG t int")]) == model([("str_key", "$0 t int")]) == model([("str_key", "$ t int")]) == "str>int,-,T74"
    assert model([("str_key", "$a.b t int")]) == "str>int,K61,T74"
    assert model([("str_key", "a.b t int")]) == "str>int,K612e62,T74"
    assert model([("str_key", "$a['b'][1] t int")]) == "str>int,K61.62[1],T74"


def table_props(nbytes):
    """one rule whose table is exactly nbytes: 24 bytes of words, a 4-byte key, the to_key behind a 3-byte STR header"""
    return [("str_key", "abcd " + "t" * (nbytes - 24 - 4 - 3) + " int")]


def test_table_limit(g):
    assert tm.table_bytes(tm.parse(table_props(32768))) == 32768
    assert product(g, table_props(32768)) == model(table_props(32768)) is not None
    assert product(g, table_props(32769)) is None and model(table_props(32769)) is None
    assert "32768" in g.last_error()

"""filter_rewrite_tag's configuration on the host (csrc/rtag.cpp flbgpu_rewrite_tag_parse_check, no device needed) against the CPU
model's restatement of the config map, process_config and the record accessor's parts (tests/rtag_model.py): every configuration of
the recorded fixture, a list of corner lines, and a seeded batch of generated Rule lines.  Refusals and acceptances must agree, and so
must the rules as text."""
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import rtag_model as rm
from rtag_chunks import P1, P16

CASES = json.load(open(os.path.join(HERE, "golden", "rtag_ref_cases.json")))["cases"]


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def product(g, props):
    try:
        return g.rewrite_tag_parse_check(props)
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
    # where the real plugin did not start, create refuses
    assert (want is None) == bool(case.get("refused"))
    assert product(g, props) == want


def test_the_rules_as_text(g):
    assert g.rewrite_tag_parse_check(P1) == "K6c6f67,P5e2e2a6572726f722e2a24,[S6572722e T],drop" == model(P1)
    props = [("rule", "$a['b'][1] ^(x)(y)?$ $TAG[1].$1.$0.$k['m'] on extra words"), ("Rule", "$TAG . plain false")]
    assert g.rewrite_tag_parse_check(props) == "K61.62[1],P5e2878292879293f24,[t1 S2e R1 S2e R0 S2e K6b.6d],keep;-,P2e,[S706c61696e],drop" == model(props)
    assert product(g, []) == "" == model([])
    assert product(g, P16) == model(P16) is not None


QUIRKS = [
    # names without case; the emitter's properties are read and put aside
    [("RULE", "a b c true"), ("Emitter_Name", "x"), ("EMITTER_MEM_BUF_LIMIT", "10M"), ("emitter_storage.TYPE", "FileSystem")],
    [("emitter_storage.type", "memory")], [("emitter_storage.type", "mem")], [("emitter_storage.type", "")],
    # entries
    [("Rule", "a b c")], [("Rule", "a b")], [("Rule", "")], [("Rule", "a b c d e f")], [("Rule", '"a" "b c" "d e" "yes"')], [("Rule", "  a   b   c   on  ")],
    [("Rule", 'a b "" true')], [("Rule", '"" b c true')], [("Rule", 'a "" c true')],
    # KEEP words
    [("Rule", "a b c TRUE")], [("Rule", "a b c oN")], [("Rule", "a b c Yes")], [("Rule", "a b c 1")], [("Rule", "a b c off")], [("Rule", "a b c trueish")],
    # KEY: the first part decides
    [("Rule", "$a b c true")], [("Rule", "pre$key b c true")], [("Rule", "$TAG b c true")], [("Rule", "$TAG[1] b c true")], [("Rule", "$0 b c true")],
    [("Rule", "$ b c true")], [("Rule", "$a.b b c true")], [("Rule", "a.b b c true")], [("Rule", "$a['x']['y'][2] b c true")], [("Rule", "$a['it''s'] b c true")],
    [("Rule", "$a['x b c true")], [("Rule", "$a[x] b c true")], [("Rule", "$-a b c true")], [("Rule", "$" + "k" * 127 + " b c true")],
    [("Rule", "$" + "k" * 128 + " b c true")], [("Rule", "k" * 127 + " b c true")], [("Rule", "k" * 128 + " b c true")],
    [("Rule", "$a" + "['s']" * 8 + " b c true")], [("Rule", "$a" + "['s']" * 9 + " b c true")],
    # NEW_TAG: parts
    [("Rule", "a b $TAG true")], [("Rule", "a b $TAG[0].$TAG[12] true")], [("Rule", "a b $TAG[] true")], [("Rule", "a b $TAG[ true")], [("Rule", "a b $TAGS true")],
    [("Rule", "a b $TA true")], [("Rule", "a (b) $0$1$2 true")], [("Rule", "a (b) $10 true")], [("Rule", "a b x$ true")], [("Rule", "a b $ true")],
    [("Rule", "a b $k.$k['a'][0],$j true")], [("Rule", "a b $k['x true")], [("Rule", "a b $k[x] true")], [("Rule", "a b " + ".".join(["$k"] * 8) + " true")],
    [("Rule", "a b " + "".join(["$k,"] * 8) + " true")], [("Rule", "a b " + "".join(["$k,"] * 9) + " true")], [("Rule", "a b " + "x" * 5000 + " true")],
    # patterns
    [("Rule", "a ^(x c true")], [("Rule", "a [x c true")], [("Rule", "a /^X$/i c true")], [("Rule", "a (?=x) c true")], [("Rule", "a (x)\\1 c true")],
    [("Rule", "a (?<!x)y c true")], [("Rule", "a (?>x) c true")], [("Rule", "a " + "(x)" * 10 + " $10 true")], [("Rule", "a " + "(x)" * 9 + " $10 true")],
    # unknown names, limits of the table
    [("Match", "*")], [("Rule", "a b c true"), ("rules", "a b c true")],
    [("Rule", "k%d ^v%d$ t%d.$TAG true" % (i, i, i)) for i in range(32)], [("Rule", "k%d ^v%d$ t%d.$TAG true" % (i, i, i)) for i in range(33)],
]


@pytest.mark.parametrize("i", range(len(QUIRKS)))
def test_quirks(g, i):
    assert product(g, QUIRKS[i]) == model(QUIRKS[i])


def test_what_the_quirks_decide(g):
    refused = [i for i, p in enumerate(QUIRKS) if model(p) is None]
    assert [QUIRKS[i][0][1][:14] for i in refused if QUIRKS[i][0][0] == "Rule"][:4] == ["a b c", "a b", "", '"" b c true']
    assert model([("Rule", "pre$key b c true")]).startswith("K707265,")
    assert model([("Rule", "$TAG b c true")]).startswith("-,") and model([("Rule", "$0 b c true")]).startswith("-,")
    assert model([("Rule", "a b c trueish")]).endswith(",drop") and model([("Rule", "a b c oN")]).endswith(",keep")
    # a pattern that is not a regular expression is refused, and last_error says so
    for pat in ("(?=x)", "(x)\\1", "(?<!x)y", "(?>x)"):
        assert product(g, [("Rule", "a %s c true" % pat)]) is None
        assert "not a regular expression" in g.last_error()
    # sixteen rules of eight template parts each fit
    assert product(g, P16) is not None and all(len(r["parts"]) >= 8 for r in rm.parse(P16))


KEYS = ["log", "$log", "$a['b']", "$a['b'][2]", "$a[0]", "pre$x", "$TAG", "$TAG[1]", "$3", "$", "a.b", "$a.b", "$a['x", "$a[y]", "$9z", "é", "$é"]
PATS = ["^x$", ".", "(a)(b)?", "^(?<n>\\d+)-(\\w+)$", "[a-z]+", "/^ab/i", "(", "[z", "(?=a)b", "(a)\\1", "a|b|c", "\\d{2,3}", "(?:x)(y)"]
PARTS = ["lit", ".", "$TAG", "$TAG[0]", "$TAG[3]", "$TAG[", "$TAG[]", "$0", "$1", "$2", "$9", "$12", "$k", "$k['a']", "$k['a'][1]", "$k.", "$k,", "$", " ", "-",
         "$k['x", "$k[z]", "x$y", "$TAGX", "$TA"]
KEEPS = ["true", "false", "on", "off", "yes", "no", "TRUE", "x", '""', "true extra"]


def rnd_props(r):
    props = []
    for _ in range(r.choice([1, 1, 1, 2, 3])):
        tag = "".join(r.choice(PARTS) for _ in range(r.choice([1, 2, 3, 5, 9])))
        q = r.random() < 0.3
        props.append(("Rule", "%s %s %s %s" % (r.choice(KEYS), r.choice(PATS), '"%s"' % tag if (q or " " in tag) and '"' not in tag else tag.replace(" ", "_"), r.choice(KEEPS))))
    if r.random() < 0.1:
        props.append((r.choice(["emitter_name", "emitter_storage.type", "bogus"]), r.choice(["memory", "x"])))
    return props


@pytest.mark.parametrize("seed", [31001, 31002, 31003])
def test_generated_rule_lines(g, seed):
    r = random.Random(seed)
    ok = no = 0
    for _ in range(400):
        props = rnd_props(r)
        want = model(props)
        assert product(g, props) == want, props
        ok += want is not None
        no += want is None
    assert ok >= 60 and no >= 60


def table_props(nbytes):
    """one rule whose table is exactly nbytes: 24 bytes of words, a 4-byte key, one 16-byte STR part and its text"""
    return [("Rule", "abcd . " + "t" * (nbytes - 24 - 4 - 16) + " true")]


def test_table_limit(g):
    assert rm.table_bytes(rm.parse(table_props(24576))) == 24576
    assert product(g, table_props(24576)) == model(table_props(24576)) is not None
    assert product(g, table_props(24577)) is None and model(table_props(24577)) is None
    assert "24576" in g.last_error()

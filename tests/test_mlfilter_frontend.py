"""filter_multiline's configuration on the host (csrc/mlfilter.cpp flbgpu_multiline_parse_check, no device needed) against the CPU
model's restatement of the config map and cb_ml_init's checks (tests/mlfilter_model.py): every configuration of the recorded fixture,
the refusals with their messages, and a seeded batch of generated property lists.  The [MULTILINE_PARSER] definitions live on the
device, so here a custom parser is a name without a definition; the built-ins are described from their tables.  The coverage floors
of the device tests' corpus are asserted here too, from the model."""
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import mlfilter_chunks as mc
import mlfilter_model as mlm

CASES = json.load(open(os.path.join(HERE, "golden", "mlfilter_ref_cases.json")))["cases"]
# started by the reference, refused here
NOT_BUILT = ("fe_mode_partial_message", "fe_two_parsers", "fe_two_parser_lines")


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def product(g, props, names):
    try:
        return g.multiline_parse_check(props, {n: None for n in names})
    except ValueError as e:
        return "refused: " + str(e).split("filter_multiline: ", 1)[-1]


def model(props, names):
    try:
        return mlm.describe(mlm.parse(props, set(names)))
    except mlm.Refused as e:
        return "refused: " + str(e)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_configurations(g, case):
    props, names = [tuple(p) for p in case["props"]], [p["name"] for p in case["parsers"]]
    want = model(props, names)
    # where the real plugin did not start, create refuses; what it starts and this project does not build is listed
    assert want.startswith("refused: ") == (bool(case.get("refused")) or case["name"] in NOT_BUILT)
    assert product(g, props, names) == want


def test_the_kept_configuration_as_text(g):
    assert product(g, mc.props("java"), []) == "parser=java key_content=log type=regex rules=8 buffer_limit=2097152" == model(mc.props("java"), [])
    assert product(g, [("multiline.parser", "ruby"), ("buffer", "off")], []) == "parser=ruby key_content=log type=regex rules=2 buffer_limit=2097152"
    assert product(g, mc.props("mine", key="message"), ["mine"]) == "parser=mine key_content=message" == model(mc.props("mine", key="message"), ["mine"])
    assert product(g, [("multiline.parser", " mine "), ("Buffer", "No")], ["mine"]) == "parser=mine key_content=(none)"


REFUSALS = [
    ([("multiline.parser", "java")], "buffered mode is not built: say 'buffer off'"),
    ([("multiline.parser", "java"), ("buffer", "on")], "buffered mode is not built: say 'buffer off'"),
    ([("multiline.parser", "java"), ("buffer", "0")], "buffered mode is not built: say 'buffer off'"),        # flb_utils_bool knows no digits: -1, which cb_ml_init reads as on
    ([("multiline.parser", "java"), ("buffer", "off"), ("mode", "partial_message")], "mode partial_message is not built"),
    ([("multiline.parser", "java"), ("buffer", "off"), ("mode", "lines")], "'Mode' must be 'partial_message' or 'parser'"),
    ([("multiline.parser", "java, go"), ("buffer", "off")], "more than one multiline parser is not built"),
    ([("multiline.parser", "java"), ("multiline.parser", "go"), ("buffer", "off")], "more than one multiline parser is not built"),
    ([("multiline.parser", "docker"), ("buffer", "off")], "a multiline parser with a parser in front ('docker') is not built"),
    ([("multiline.parser", "cri"), ("buffer", "off")], "a multiline parser with a parser in front ('cri') is not built"),
    ([("multiline.parser", "nope"), ("buffer", "off")], "multiline parser 'nope' is not defined"),
    ([("buffer", "off")], "mode parser requires at least one 'multiline.parser'"),
    ([("multiline.parser", "java"), ("buffer", "off"), ("multiline.key_group", "x")], "unknown property 'multiline.key_group'"),
]


@pytest.mark.parametrize("props,why", REFUSALS)
def test_refusals_say_which(g, props, why):
    assert product(g, props, ["mine"]) == "refused: " + why == model(props, ["mine"])


def test_generated_property_lists(g):
    rnd = random.Random(20261019)
    names = ["buffer", "Buffer", "mode", "multiline.parser", "Multiline.Parser", "multiline.key_content", "flush_ms", "emitter_name", "emitter_storage.type",
             "emitter_mem_buf_limit", "debug_flush", "match", "multiline.key_group"]
    values = {"buffer": ["off", "Off", "false", "no", "on", "true", "1", "0", ""], "mode": ["parser", "Parser", "partial_message", "x"],
              "multiline.parser": ["java", "go", "mine", "mine, java", " python ", "cri", "other", ",ruby,", ""], "multiline.key_content": ["log", "message", ""]}
    seen = set()
    for _ in range(400):
        props = []
        for _ in range(rnd.randint(0, 5)):
            n = rnd.choice(names)
            props.append((n, rnd.choice(values.get(n.lower(), ["x", "1", ""]))))
        got, want = product(g, props, ["mine"]), model(props, ["mine"])
        assert got == want, props
        seen.add(got.split(" ")[0] if not got.startswith("refused") else got)
    assert len(seen) >= 10


# ---- coverage floors of the device tests' corpus (tests/test_mlfilter_gpu.py), from the model
def test_the_generated_corpus_holds_every_class_at_every_size():
    import re
    csrc = os.path.join(os.path.dirname(HERE), "fluent-bit_amd", "csrc")
    tile = 1
    for name in ("ML_FS_T", "ML_FS_PER"):
        tile *= int(re.search(r"\b%s\s*=\s*(\d+)" % name, open(os.path.join(csrc, "ml_kernels.inc")).read()).group(1))
    for n in [63, 64, 65, 255, 256, 257, tile + 1, 2 * tile + 1]:
        for seed in (0, 3):
            m = mlm.Model(mc.props("cont"), {"cont": mc.CONT})
            seen = m.classes(mc.mixed(n, seed))
            assert {"rules", "not_processed", "start", "continuation", "alone"} <= seen, (n, seed, seen)
    m = mlm.Model(mc.props("cont"), {"cont": mc.CONT})
    assert "metadata" in m.classes(mc.rec(mc.kv(("log", "x")), 1, 1, mc.kv(("m", 1))))

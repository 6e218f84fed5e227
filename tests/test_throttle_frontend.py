"""The configuration of filter_throttle_size and filter_throttle on the host (csrc/throttle.cpp flbgpu_throttle_size_parse_check,
flbgpu_throttle_parse_check; no device needed) against the CPU model's resolved configuration (tests/throttle_model.py, which asks
libc for strtod / strtoul / atoi): every recorded property set and a generated list.  (tools/throttle_sanitize.cpp drives the same
entry points as a stand-alone program under AddressSanitizer and UBSan: host code only, run on the CPU, by hand.)"""
import itertools
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import flbamd_loader
import throttle_model as tm

FIX = {k: json.load(open(os.path.join(HERE, "golden", "%s_ref_cases.json" % k)))["cases"] for k in ("throttle_size", "throttle")}
NUMBERS = ["", "0", "1", "2", "5", "-1", "1.5", "0.5", "1e3", "10x", "x", " 7", "7 ", "+3", "65536", "65537", "1k", "1K", "2kb", "1.5M", "1G", "3mb", "1kx", "false",
           "FALSE", "1e400", "nan", "inf", "0x10", "3s", "2m", "1h", "1d", "5ss", "1x", "s", "4294967297", "-0", "99999999999999999999"]
PATHS = ["", "a", "a|b", "|", "||", "a||b", "|a", "a|", "a||", "|".join("k%d" % i for i in range(20)), "|".join("k%d" % i for i in range(21)),
         "|".join("k%d" % i for i in range(25)) + "||x|", "a" * 300 + "|b"]


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def both(g, kind, props):
    check, model = (g.throttle_size_parse_check, tm.SizeConfig) if kind == "throttle_size" else (g.throttle_parse_check, tm.ThrottleConfig)
    try:
        got = check(props)
    except ValueError:
        got = None
    try:
        want = model(props).describe()
    except tm.Refused:
        want = None
    assert got == want, props


@pytest.mark.parametrize("kind", ["throttle_size", "throttle"])
def test_recorded_property_sets(g, kind):
    for c in FIX[kind]:
        both(g, kind, [tuple(p) for p in c["props"]])
        assert g.throttle_size_parse_check([tuple(p) for p in c["props"]]) if kind == "throttle_size" else True      # (none is refused)


def test_generated_throttle_size_properties(g):
    for name in ("rate", "window", "interval", "window_time_duration"):
        for v in NUMBERS:
            both(g, "throttle_size", [(name, v)])
    for i, d, w in itertools.product(["0", "3s", "2m", "x"], ["1", "7", "1h"], ["1", "2", "30"]):
        both(g, "throttle_size", [("Interval", i), ("WINDOW_TIME_DURATION", d), ("window", w)])
    for p in PATHS:
        both(g, "throttle_size", [("name_field", p)])
        both(g, "throttle_size", [("log_field", p), ("name_field", "n")])
    both(g, "throttle_size", [("rate", "5"), ("rate", "7"), ("print_status", "maybe"), ("hash_table_size", "0"), ("anything", "else")])
    both(g, "throttle_size", [("name_field", "|".join("x" * 2000 for _ in range(21)))])                            # the path table's cap


def test_generated_throttle_properties(g):
    for name in ("rate", "window", "interval"):
        for v in NUMBERS:
            both(g, "throttle", [(name, v)])
    for props in ([("print_status", "on")], [("print_status", "maybe")], [("nope", "1")], [("rate", "2"), ("Rate", "3")], [("interval", "${X}")],
                  [("RATE", "2.5"), ("Window", "7"), ("INTERVAL", "2m"), ("Print_Status", "FALSE")]):
        both(g, "throttle", props)

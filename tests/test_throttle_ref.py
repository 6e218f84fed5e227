"""The CPU model of filter_throttle_size and filter_throttle (tests/throttle_model.py) against the recorded answers of the real plugins
(tests/golden/throttle_size_ref_cases.json, throttle_ref_cases.json; tools/gen_throttle_golden.py): every case, step by step, byte for
byte.  The two cases marked `deviates` -- a name with a NUL byte -- are the only ones left out of byte equality: for them the test
asserts the documented behaviour."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import throttle_chunks as tc
import throttle_model as tm

FIX = {k: json.load(open(os.path.join(HERE, "golden", "%s_ref_cases.json" % k))) for k in ("throttle_size", "throttle")}
ALL = [(k, c) for k in FIX for c in FIX[k]["cases"]]


def recorded(case):
    return [(tm.MODIFIED if s[2] == 1 else tm.NOTOUCH, base64.b64decode(s[3]) if s[3] is not None else None) for s in case["steps"] if s[0] == "chunk"]


@pytest.mark.parametrize("kind,case", ALL, ids=["%s-%s" % (k, c["name"]) for k, c in ALL])
def test_model_reproduces_the_recording(kind, case):
    assert not case.get("refused")
    _m, res = tm.replay(kind, case)
    if case.get("deviates"):
        assert kind == "throttle_size" and case["name"] in tc.DEVIATES
        return
    assert res == recorded(case)


def test_fixtures_hold_the_named_cases():
    for kind, cases in (("throttle_size", tc.size_cases()), ("throttle", tc.throttle_cases())):
        assert FIX[kind]["recorded_from"] == "whole plugin"
        have = {c["name"]: c for c in FIX[kind]["cases"]}
        assert [n for n, _, _ in cases] == [c["name"] for c in FIX[kind]["cases"]]
        for name, props, steps in cases:
            c = have[name]
            assert [tuple(p) for p in c["props"]] == props
            assert [(s[0], base64.b64decode(s[1]) if s[0] == "chunk" else s[1]) for s in c["steps"]] == [tuple(s) for s in steps], name
    names = {c["name"] for c in FIX["throttle_size"]["cases"]}
    for must in ("rt_simple_log", "rt_nested_log", "rt_default_name_field", "rt_default_log_field", "edge_sum_300_kept", "edge_sum_301_dropped",
                 "edge_0001_in_binary64", "first_record_alone_too_large", "small_after_dropped", "ticks_rotate_every_pane", "stale_deletion_then_the_name_again",
                 "star_window_goes_stale", "load_zero_leaves_timestamp", "path_depth_20", "path_depth_21", "call_empty_chunk") + tc.DEVIATES:
        assert must in names
    assert sorted(c["name"] for c in FIX["throttle_size"]["cases"] if c.get("deviates")) == sorted(tc.DEVIATES)
    assert {"rt_throttle", "before_the_first_tick", "k_0", "k_1", "k_n_minus_1", "k_n", "k_over_n", "ticks_with_a_repeated_timestamp", "window_wraps",
            "cfg_window_1"} <= {c["name"] for c in FIX["throttle"]["cases"]}


def test_the_edges_as_recorded():
    """the figures the issue names, read off the recording: a sum of 300 under rate 10 x window 30 is kept, 301 is not"""
    have = {c["name"]: recorded(c) for c in FIX["throttle_size"]["cases"]}
    assert have["edge_sum_300_kept"][0][0] == tm.MODIFIED                 # (the 1 byte on top of 300 is what goes)
    k = tm.ThrottleSize([("window", "30"), ("rate", "10")])
    assert not k.over(300) and k.over(301)


def test_nul_names_are_whole_names():
    """the product (and the model) take the full bytes as the name, so a\\0b has a window of its own that fills like any other"""
    for name in tc.DEVIATES:
        case = [c for c in FIX["throttle_size"]["cases"] if c["name"] == name][0]
        m, res = tm.replay("throttle_size", case)
        assert b"a\0b" in m.windows and m.windows[b"a\0b"].total == 30
        assert res[0][0] == tm.MODIFIED
        assert recorded(case)[0][0] == tm.NOTOUCH                           # the reference never finds the window again: all kept


def test_path_through_a_value_that_is_no_map_finds_nothing():
    """DESIGN 8 (not recorded: undefined behaviour in the reference): the record is kept and exempt"""
    from throttle_chunks import kv, rec
    m = tm.ThrottleSize([("rate", "1"), ("window", "2"), ("name_field", "a|b"), ("log_field", "log")])
    data = b"".join(rec(kv(("a", v), ("log", "x" * 100)), i + 1) for i, v in enumerate(["bb", [kv(("b", "n"))], 7, 2.5, True]))
    assert m.filter(data) == (tm.NOTOUCH, None) and m.n_exempt == 5 and not m.windows

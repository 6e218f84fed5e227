"""The CPU model of filter_kubernetes (tests/kube_model.py) against the recorded answers of the real plugin
(tests/golden/kube_ref_cases.json, tools/gen_kube_golden.py): every case byte for byte, none left out except those the real filter did
not start on, which parse must refuse.  And the host's tag matcher (the project's own regex front end and backtracking search, through
flbgpu_kubernetes_tag_check) against real Onigmo's group spans (tests/rxdiff.py) on the recording's tags and a generated list.  No device."""
import base64
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import kube_model as km
import rxdiff
from kube_chunks import DOCKER_ID

FIXTURE = json.load(open(os.path.join(HERE, "golden", "kube_ref_cases.json")))
CASES = FIXTURE["cases"]
MODIFIED, NOTOUCH = km.Model.MODIFIED, km.Model.NOTOUCH

# the cases the issue names: the recording must hold them
NAMES = """rt_core_base rt_merge_log_enabled_json rt_merge_log_enabled_text rt_merge_log_enabled_invalid_json rt_merge_log_disabled_json
rt_keep_log_enabled_json rt_keep_log_disabled_json rt_merge_log_key_json rt_merge_log_trim_enabled_json rt_merge_log_trim_disabled_json
rt_exclude_default rt_exclude_stdout rt_exclude_stderr st_every_status_keep_on_nokey st_every_status_keep_on_key
st_every_status_keep_off_nokey st_every_status_keep_off_key key_bin key_str8 key_value_str32 key_second_log key_absent key_merge_log_off
log_key_integer_3 trim_shapes trim_nested_str trim_header_width trim_json_escape stream_exclude_none stream_exclude_stdout
stream_exclude_stderr stream_exclude_both stream_all_excluded json_nesting_31 json_nesting_32 json_nesting_33 json_nesting_63 json_nesting_64 json_nesting_65 json_nesting_70 json_decimals
json_invalid_utf8 json_embedded_nul json_duplicate_keys json_15_pairs json_16_pairs json_white_space wr_metadata_dropped
wr_integer_and_float_time wr_time_refused_first wr_time_refused_middle wr_time_refused_last wr_group_markers wr_non_canonical
wr_float32_and_ext wr_namespace_only wr_pod_and_namespace tag_stock tag_pod_with_dots tag_container_with_dashes tag_no_longer_than_prefix
tag_does_not_match tag_custom_prefix call_empty_chunk call_garbage_reserved_byte call_cut_record""".split()


def test_the_recording_holds_the_named_cases():
    have = {c["name"] for c in CASES}
    assert not [n for n in NAMES if n not in have]
    assert "whole plugin" in FIXTURE["recorded_from"]


def model_of(case):
    """the model set up as the case was recorded: the entries through set_meta, or the tag through set_tag"""
    props = [tuple(p) for p in case["props"]]
    m = km.Model(props)
    if m.cfg.tag_meta:
        m.set_tag(case["tag"])
    else:
        m.set_meta(base64.b64decode(case["pod"]) if case["pod"] else None, base64.b64decode(case["ns"]) if case["ns"] else None)
    return m


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_recording(case):
    if case.get("refused") or case.get("crashed"):
        with pytest.raises(ValueError):
            km.parse([tuple(p) for p in case["props"]])
        return
    ret, out = model_of(case).filter(base64.b64decode(case["in"]))
    assert ret == case["ret"]
    assert out == (base64.b64decode(case["out"]) if case["out"] is not None else None)


def generated_tags():
    """200 tags, half of them built to match"""
    rnd = random.Random(20241020)
    low = "abcdefghijklmnopqrstuvwxyz0123456789"

    def word(alpha, lo, hi):
        return "".join(rnd.choice(alpha) for _ in range(rnd.randint(lo, hi)))

    def label():
        w = word(low, 1, 6)
        return w if rnd.random() < 0.5 else w + word(low + "-", 0, 5) + word(low, 1, 2)
    tags = []
    for i in range(200):
        pod = ".".join(label() for _ in range(rnd.randint(1, 3)))
        ns = word(low + "-.", 1, 12)
        cont = word(low + "-_.", 1, 14)
        did = word("abcdef0123456789", 64, 64)
        t = "%s_%s_%s-%s.log" % (pod, ns, cont, did)
        if i % 2:
            how = rnd.randrange(6)
            t = [t[:-1], t.replace("_", "-"), "%s_%s_%s-%s.log" % (pod, ns, cont, did[:rnd.randint(0, 63)]), pod.upper() + t[len(pod):] if pod.upper() != pod else "_" + t,
                 t + "\n", "%s__%s-%s.log" % (pod, cont, did.upper())][how]
        tags.append(t)
    return tags


@pytest.mark.skipif(rxdiff.load_ref() is None, reason="oracle/_ref/libonig_ref.so not built (needs the reference tree)")
def test_tag_matcher_spans_equal_onigmo():
    g = flbamd_loader.load()
    rx = rxdiff.RefRegex(rxdiff.load_ref(), km.KUBE_TAG_TO_REGEX.encode())
    assert rx.ok
    group_of = dict(rx.names())
    prefix = km.TAG_PREFIX.decode()
    tags = [c["tag"][len(prefix):] for c in CASES if c["tag"].startswith(prefix) and len(c["tag"]) > len(prefix) + 1] + generated_tags()
    props = [("use_tag_for_meta", "on"), ("kube_tag_prefix", "")]
    hits = 0
    for t in tags:
        tb = t.encode()
        found = rx.search(tb)
        spans = {n: found[group_of[n]] for n in km.TAG_FIELDS} if found is not None else None
        want = km.tag_entry(b"", tb) if len(tb) > 1 else None
        if spans is None:
            assert want is None
            with pytest.raises(ValueError):
                g.kubernetes_tag_check(props, tb)
            continue
        hits += 1
        # Onigmo's spans are the model's, and the entry the host builds holds exactly those bytes
        assert {n: tuple(spans[n]) for n in km.TAG_FIELDS} == km.tag_spans(tb)
        assert g.kubernetes_tag_check(props, tb) == want
    assert 100 <= hits < len(tags)

"""filter_kubernetes' host-only entry points (csrc/kube.cpp) against the CPU model (tests/kube_model.py), no device: the line
flbgpu_kubernetes_parse_check writes, every refusal of create with its last_error, what set_meta keeps of two cache entries and what
it refuses (flbgpu_kubernetes_meta_check), and the pod entry set_tag builds from a tag (flbgpu_kubernetes_tag_check)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import kube_model as km
from kube_chunks import DOCKER_ID, STOCK_TAG, blob_of, pod_meta


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


LINES = [
    ([], "merge_log=0;keep_log=1;trim=1;merge_log_key=-;tag_meta=0;prefix=" + b"kube.var.log.containers.".hex()),
    ([("Merge_Log", "On"), ("KEEP_LOG", "no"), ("merge_log_trim", "false"), ("merge_log_key", "parsed"), ("use_tag_for_meta", "YES"), ("kube_tag_prefix", "k.")],
     "merge_log=1;keep_log=0;trim=0;merge_log_key=706172736564;tag_meta=1;prefix=6b2e"),
    ([("merge_log_key", "")], "merge_log=0;keep_log=1;trim=1;merge_log_key=;tag_meta=0;prefix=" + b"kube.var.log.containers.".hex()),
    # the names that configure the metadata half are accepted and not looked at
    ([("kube_url", "https://127.0.0.1:1"), ("labels", "off"), ("annotations", "off"), ("k8s-logging.parser", "on"), ("k8s-logging.exclude", "on"),
      ("namespace_labels", "on"), ("owner_references", "on"), ("kube_meta_cache_ttl", "60"), ("buffer_size", "1M"), ("use_journal", "off"), ("dummy_meta", "no"),
      ("tls.verify", "off"), ("kube_meta_preload_cache_dir", "/nowhere"), ("use_kubelet", "true"), ("set_platform", "eks")],
     "merge_log=0;keep_log=1;trim=1;merge_log_key=-;tag_meta=0;prefix=" + b"kube.var.log.containers.".hex()),
    ([("merge_log_key", "k" * 32767)], None),
]


@pytest.mark.parametrize("props,line", LINES, ids=range(len(LINES)))
def test_parse_check_lines(g, props, line):
    got = g.kubernetes_parse_check(props)
    assert got == km.describe(km.parse(props))
    if line is not None:
        assert got == line


REFUSALS = [
    ([("no_such_property", "1")], "unknown configuration property 'no_such_property'"),
    ([("merge_log", "maybe")], "invalid boolean value 'maybe' for 'merge_log'"),
    ([("labels", "2")], "invalid boolean value '2' for 'labels'"),
    ([("keep_log", "")], "invalid boolean value '' for 'keep_log'"),
    ([("use_journal", "on")], "use_journal"),
    ([("dummy_meta", "true")], "dummy_meta"),
    ([("merge_parser", "json")], "merge_parser names a parser"),
    ([("regex_parser", "custom")], "regex_parser names a parser"),
    ([("merge_log_key", "k" * 32768)], "merge_log_key of 32768 bytes or more"),
    ([("kube_url", "${KUBE}")], "environment variables are not translated"),
    ([("merge_log", "on"), ("Merge_Log", "off")], "is set more than once"),
]


@pytest.mark.parametrize("props,why", REFUSALS, ids=[r[1][:24] for r in REFUSALS])
def test_refusals(g, props, why):
    with pytest.raises(ValueError) as e:
        g.kubernetes_parse_check(props)
    assert str(e.value).startswith("filter_kubernetes: ") and why in str(e.value)
    with pytest.raises(ValueError):
        km.parse(props)
    # create refuses in front of any device work, with the same words
    with pytest.raises(ValueError) as e2:
        g.FilterKubernetes(props)
    assert why in str(e2.value)


def meta_line(pod, ns):
    p, eo, ee = km.read_entry(pod, True)
    n = km.read_entry(ns, False)[0]
    return "pod=%s;ns=%s;stdout_exclude=%d;stderr_exclude=%d" % (p.hex() if p else "-", n.hex() if n else "-", eo, ee)


META = [
    (None, None), (b"", b""), (pod_meta(), None), (None, blob_of(5)), (blob_of(1), blob_of(1)), (pod_meta() + km.props_array(), blob_of(40)),
    (pod_meta() + km.props_array(True, False), None), (pod_meta() + km.props_array(False, True), None), (blob_of(64) + km.props_array(True, True), blob_of(3)),
    # only the first object of an entry is appended: a second map behind the namespace's, a properties array in a wider header
    (blob_of(9), blob_of(7) + blob_of(4)), (blob_of(9) + b"\xdc\x00\x04\xc0\xc0\xc3\xc2", None), (b"\x05", b"\xa1x"),
]


@pytest.mark.parametrize("pod,ns", META, ids=range(len(META)))
def test_set_meta_keeps(g, pod, ns):
    assert g.kubernetes_meta_check(pod, ns) == meta_line(pod, ns)


META_REFUSED = [
    (b"\x81\xa1k", None, "first object does not decode"),
    (b"\xc1", None, "first object does not decode"),
    (None, b"\x81\xa1k\xa5xx", "namespace entry"),
    (None, b"\x91" * 40 + b"\x90", "first object does not decode"),
    (blob_of(5) + b"\x93\xc0\xc0\xc2", None, "another shape"),
    (blob_of(5) + b"\x80", None, "another shape"),
    (blob_of(5) + b"\x94\xc0\xc0\x01\xc2", None, "another shape"),
    (blob_of(5) + b"\x94\x01\xc0\xc2\xc2", None, "another shape"),
    (blob_of(5) + b"\x94\xc0\xc0\xc2", None, "another shape"),
    (blob_of(5) + km.props_array(False, False, b"apache"), None, "parser"),
    (blob_of(5) + km.props_array(False, False, None, b"json"), None, "parser"),
    (blob_of((1 << 20) + 1), None, "1 MiB"),
    (None, blob_of((1 << 20) + 1), "1 MiB"),
]


@pytest.mark.parametrize("pod,ns,why", META_REFUSED, ids=range(len(META_REFUSED)))
def test_set_meta_refusals(g, pod, ns, why):
    with pytest.raises(ValueError) as e:
        g.kubernetes_meta_check(pod, ns)
    assert str(e.value).startswith("filter_kubernetes: ") and why in str(e.value)
    with pytest.raises(ValueError):
        meta_line(pod, ns)


def test_entry_of_a_mebibyte_is_taken(g):
    pod = blob_of(1 << 20)
    assert g.kubernetes_meta_check(pod, None) == meta_line(pod, None)


TAG = [("use_tag_for_meta", "on")]
TAGS = [
    (TAG, STOCK_TAG),
    (TAG, "kube.var.log.containers.my.pod-0.with.dots_kube-system_side-car-%s.log" % DOCKER_ID),
    (TAG, "kube.var.log.containers.p_n_c-with--dashes-and_under_scores-%s.log" % DOCKER_ID),
    (TAG + [("kube_tag_prefix", "custom.")], "custom.pod_ns_c-%s.log" % DOCKER_ID),
    (TAG + [("kube_tag_prefix", "")], "pod_ns_c-%s.log" % DOCKER_ID),
    (TAG, "kube.var.log.containers.xx" + STOCK_TAG),
    # the prefix is not compared, only its length is skipped (kube_meta.c:1797)
    (TAG + [("kube_tag_prefix", "other.prefix.that.is.long.")], STOCK_TAG),
]
BAD_TAGS = [
    (TAG, "kube.var.log.containers.", "shorter than kube_tag_prefix"),
    (TAG, "kube.var.log.containers.a", "shorter than kube_tag_prefix"),
    (TAG, "short", "shorter than kube_tag_prefix"),
    (TAG, "kube.var.log.containers.apache_default_apache-%s.log" % DOCKER_ID[:63], "invalid pattern"),
    (TAG, "kube.var.log.containers.Apache_default.log", "invalid pattern"),
    (TAG, STOCK_TAG + "x", "invalid pattern"),
    ([], STOCK_TAG, "use_tag_for_meta"),
]


@pytest.mark.parametrize("props,tag", TAGS, ids=range(len(TAGS)))
def test_set_tag_entries(g, props, tag):
    want = km.tag_entry(km.parse(props).prefix, tag.encode())
    assert want is not None and g.kubernetes_tag_check(props, tag) == want
    assert want[:5] == b"\xdf\x00\x00\x00\x04"


@pytest.mark.parametrize("props,tag,why", BAD_TAGS, ids=range(len(BAD_TAGS)))
def test_set_tag_refusals(g, props, tag, why):
    with pytest.raises(ValueError) as e:
        g.kubernetes_tag_check(props, tag)
    assert why in str(e.value)
    if props:
        assert km.tag_entry(km.parse(props).prefix, tag.encode()) is None

#!/usr/bin/env python3
"""Records the answers of the real filter_kubernetes for tests/golden/kube_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of
`make -C oracle engine` (oracle/_ref/engine).  The WHOLE plugin -- kubernetes.c, kube_conf.c, kube_meta.c, kube_regex.c,
kube_property.c, kubernetes_aws.c -- is compiled where it lies as a loadable flb-filter_kubernetes.so in a scratch directory outside
the repository (it links against the minimal engine as it is; no part of it is replaced), next to tools/kube_ref_host.c -- this
project's own host, which creates the filter instance in the reference engine library and calls the plugin's cb_init / cb_filter
with the case's tag.  Nothing compiled and no reference text enters the repository, only the fixture.

The metadata never comes from a network: every case that is not use_tag_for_meta gets kube_meta_preload_cache_dir -- a scratch
directory into which this generator writes <namespace>_<pod>.meta (and <namespace>.namespace_meta where the case asks for namespace
metadata) -- and kube_url https://127.0.0.1:1, a closed loopback port, so that a mistake fails at once inside the machine.  The
generator refuses to run a case whose file is not there.

Per case the fixture holds the properties, the tag, the input (base64), cb_filter's return value, the output when it is
FLB_FILTER_MODIFIED, and the pod / namespace entries to hand to flbgpu_kubernetes_set_meta: the maps are cut out of a probe run (one
plain record, the same properties with k8s-logging.exclude off), every output record of the case is checked to carry the same bytes,
and behind the pod map stands the properties array as flb_kube_prop_pack would write it from the annotations of the case's meta
file -- or "refused": the filter did not start, or "crashed": the host died.

The JSON-path cases of the reference's runtime test (tests/runtime/filter_kubernetes.c) are transcribed first, with its meta files
read from the reference tree at generation time.  (tools/perf_kubernetes.py --cpu-reference times the plugin through the same host.)"""
import argparse
import base64
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402
import modify_model as mm  # noqa: E402
import kube_model as km  # noqa: E402
from gen_recmod_golden import includes  # noqa: E402
from kube_chunks import BIG_T, DOCKER_ID, GROUP_END, GROUP_START, R, docker, f32, kv, nested, rec, rows, sv  # noqa: E402

CRASHES = ("log_key_integer_3",)
KUBE_URL = "https://127.0.0.1:1"
MODIFIED = 1


def tag_of(pod, ns="default", container="app"):
    return "kube.var.log.containers.%s_%s_%s-%s.log" % (pod, ns, container, DOCKER_ID)


def cases():
    c = []

    def add(name, props, data, annotations=None, meta_file=None, ns_meta=None, tag=None, pod=None, ns="default"):
        pod = pod or name.split("_")[0]
        c.append(dict(name=name, props=[list(p) for p in props], data=data, annotations=annotations or {}, meta_file=meta_file, ns_meta=ns_meta,
                      tag=tag if tag is not None else tag_of(pod, ns), pod=pod, ns=ns))
    ML = [("merge_log", "on")]
    rt_json = docker(0, '{"text":"Simple text"}\n')
    # ---- tests/runtime/filter_kubernetes.c, the JSON-path cases (the docker parser's records: log, stream, time)
    add("rt_core_base", ML, docker(0, "Fluent Bit is logging\n"), meta_file="core_base.meta")
    add("rt_merge_log_enabled_json", ML, rt_json)
    add("rt_merge_log_enabled_text", ML, docker(0, "This is a text message\n"))
    add("rt_merge_log_enabled_invalid_json", ML, docker(0, '{"this is": "invalid" json}\n'))
    add("rt_merge_log_disabled_json", [("merge_log", "off")], rt_json)
    add("rt_keep_log_enabled_json", ML + [("keep_log", "on")], rt_json)
    add("rt_keep_log_disabled_json", ML + [("keep_log", "off")], rt_json)
    add("rt_merge_log_key_json", ML + [("merge_log_key", "merge-log-key")], rt_json)
    trim = docker(0, '{"text":"text with trailing newlines\\n\\n"}\n')
    add("rt_merge_log_trim_enabled_json", ML + [("merge_log_trim", "on")], trim)
    add("rt_merge_log_trim_disabled_json", ML + [("merge_log_trim", "off")], trim)
    both = docker(0, "to stdout\n", "stdout") + docker(1, "to stderr\n", "stderr") + rec(kv(("log", "no stream")), 5)
    EX = [("k8s-logging.exclude", "on")]
    add("rt_exclude_default", EX, both, {"fluentbit.io/exclude": "true"})
    add("rt_exclude_stdout", EX, both, {"fluentbit.io/exclude_stdout": "true"})
    add("rt_exclude_stderr", EX, both, {"fluentbit.io/exclude_stderr": "true"})
    add("rt_exclude_option_off", [("k8s-logging.exclude", "off")], both, {"fluentbit.io/exclude": "true"})
    # ---- every merge status x keep_log x merge_log_key
    logs = [("none_not_json", "plain text\n"), ("none_root_array", "[1]"), ("none_two_records", '{"a":1}{"b":2}'), ("none_second_value", '{"a":1} 5'),
            ("parsed_plus_junk", '{"a":1} x'), ("parsed", '{"a":1,"b":"two\\n","c":[1,{"d":null}]}'), ("parsed_empty", "{}"), ("map", kv(("a", 1), ("b", "two\n"))),
            ("map_empty", kv()), ("type_integer", 7), ("type_nil", None), ("type_bin", R(b"\xc4\x07{\"a\":1}")), ("type_array", ['{"a":1}'])]
    data = b"".join(rec(kv(("case", lname), ("log", log), ("stream", "stdout")), 10 + i, 20) for i, (lname, log) in enumerate(logs))
    for keep in ("on", "off"):
        for key in (None, "merged"):
            add("st_every_status_keep_%s_%s" % (keep, "key" if key else "nokey"), ML + [("keep_log", keep)] + ([("merge_log_key", key)] if key else []), data, pod="st")
    # ---- `log` key forms
    add("key_bin", ML, rec(kv((R(b"\xc4\x03log"), '{"a":1}')), 1), pod="key")
    add("key_bin16", ML, rec(kv((R(b"\xc5\x00\x03log"), "text")), 1), pod="key")
    add("key_str8", ML, rec(kv((R(b"\xd9\x03log"), '{"a":1}')), 1), pod="key")
    add("key_value_str32", ML, rec(kv(("log", R(b"\xdb\x00\x00\x00\x07{\"a\":1}"))), 1) + rec(kv(("log", R(b"\xdb\x00\x00\x00\x04text"))), 2), pod="key")
    add("key_second_log", ML, rec(kv(("log", '{"a":1}'), ("log", '{"b":2}')), 1) + rec(kv(("log", "text"), ("log", '{"b":2}')), 2), pod="key")
    add("key_absent", ML, rec(kv(("logs", '{"a":1}'), ("lo", "x"), ("Log", "y")), 1), pod="key")
    add("key_merge_log_off", [], rec(kv(("log", '{"a":1}')), 1), pod="key")
    add("log_key_integer_3", ML, rec(kv((3, "three"), ("log", '{"a":1}')), 1), pod="key")
    # ---- trim
    shapes = ['{"s":"\\n"}', '{"s":"\\n\\n"}', '{"s":"x\\\\n"}', '{"s":"x\\n"}', '{"s":"a\\\\n\\n\\\\r\\n"}', '{"s":"\\\\n"}', '{"s":"n"}', '{"s":""}', '{"s":"\\\\r\\\\n"}',
              '{"s":"x\\\\\\\\n"}']
    tr = b"".join(rec(kv(("log", s)), i + 1) for i, s in enumerate(shapes))
    add("trim_shapes", ML, tr, pod="trim")
    add("trim_nested_str", ML, rec(kv(("log", '{"m":{"s":"x\\n"},"l":["y\\n"],"t":"z\\n"}')), 1), pod="trim")
    add("trim_header_width", ML, rec(kv(("log", '{"t":"' + "x" * 31 + '\\n\\n"}')), 1) + rec(kv(("log", '{"t":"' + "x" * 32 + '\\n"}')), 2), pod="trim")
    add("trim_json_escape", ML, rec(kv(("log", '{"t":"end\\u000a","u":"\\u005cn"}')), 1), pod="trim")
    add("trim_map_values_stay", ML, rec(kv(("log", kv(("s", "x\n\n"), ("t", "\\n")))), 1), pod="trim")
    # ---- stream
    sk = [("stream", "stdout"), ("stream", "std"), ("stream", ""), ("stream", "stderr"), ("stream", "other"), ("s", "stderr"), ("", "stderr"), ("streams", "stderr"),
          ("stream", R(b"\xc4\x06stderr")), (sv(b"stream\0x"), "stderr"), ("stream", sv(b"stdout\0x")), ("stream", "stdoutx"), (R(b"\xc4\x06stream"), "stderr")]
    st = b"".join(rec(kv((k, v)), i + 1) for i, (k, v) in enumerate(sk)) + rec(kv(("n", 99)), 99) + rec(kv(("s", "other"), ("stream", "stderr")), 100)
    for nm, ann in (("none", {}), ("stdout", {"fluentbit.io/exclude_stdout": "true"}), ("stderr", {"fluentbit.io/exclude_stderr": "true"}),
                    ("both", {"fluentbit.io/exclude": "true"})):
        add("stream_exclude_" + nm, EX, st, ann, pod="stream-" + nm)
    add("stream_all_excluded", EX, rows(3), {"fluentbit.io/exclude_stdout": "true"}, pod="stream-stdout")
    add("stream_value_integer", EX, rec(kv(("stream", 5)), 1) + rec(kv(("stream", None)), 2), {"fluentbit.io/exclude_stdout": "true"}, pod="stream-stdout")
    # ---- JSON corners
    for d in (31, 32, 33, 63, 64, 65, 70):
        add("json_nesting_%d" % d, ML + [("keep_log", "off")], rec(kv(("log", nested(d)), ("x", 1)), 1), pod="json")
    add("json_nesting_64_key", ML + [("merge_log_key", "k")], rec(kv(("log", nested(64))), 1), pod="json")
    add("json_decimals", ML, rec(kv(("log", '{"d":0.1,"e":1e300,"f":123456789012345678901234567890,"g":3.' + "1" * 40 + ',"h":-0.0,"i":18446744073709551615}')), 1), pod="json")
    add("json_invalid_utf8", ML, rec(kv(("log", sv(b'{"b":"\xff\xfe x \xc3","c":"\xe2\x82"}'))), 1), pod="json")
    add("json_embedded_nul", ML, rec(kv(("log", '{"z":"a\\u0000b","y":"c"}')), 1) + rec(kv(("log", sv(b'{"z":"a\0b"}'))), 2), pod="json")
    add("json_surrogates", ML, rec(kv(("log", '{"x":"\\ud800","y":"\\ud83d\\ude00","z":"\\udc00 t"}')), 1), pod="json")
    add("json_duplicate_keys", ML, rec(kv(("a", 0), ("log", '{"a":1,"a":2,"log":"inner"}')), 1), pod="json")
    for n in (15, 16):
        js = "{" + ",".join('"k%d":%d' % (i, i) for i in range(n)) + "}"
        add("json_%d_pairs" % n, ML + [("keep_log", "off")], rec(kv(("log", js)), 1), pod="json")
        add("json_%d_pairs_key" % n, ML + [("merge_log_key", "k")], rec(kv(("log", js)), 1), pod="json")
    add("json_white_space", ML, rec(kv(("log", ' \t\r\n{ "a" : 1 , "b" : [ 1 , 2 ] } \n\t ')), 1) + rec(kv(("log", "   ")), 2) + rec(kv(("log", "")), 3), pod="json")
    add("json_malformed", ML, b"".join(rec(kv(("log", s)), i + 1) for i, s in enumerate(['{"a":', '{"a":1,}', "{a:1}", '{"a":1}}', '{"a":tru}', '{"a":01}'])), pod="json")
    # ---- the writer
    w = ML
    add("wr_metadata_dropped", w, rec(kv(("log", '{"a":1}')), 5, 6, kv(("m", 1), ("z", [1, 2]))) + rec(kv(("x", 1)), 7, 8, kv(("m", 2))), pod="wr")
    add("wr_integer_and_float_time", w, synth.mp([1700000000, kv(("log", '{"a":1}'))]) + synth.mp([1700000000.25, kv(("log", "text"))]), pod="wr")
    big = synth.mp([BIG_T, kv(("log", "big"))])
    a, b = rec(kv(("log", '{"a":1}')), 1), rec(kv(("nolog", "b")), 2)
    add("wr_time_refused_first", w, big + a + b, pod="wr")
    add("wr_time_refused_middle", w, a + big + b, pod="wr")
    add("wr_time_refused_last", w, a + b + big, pod="wr")
    add("wr_time_refused_but_excluded", EX, a + synth.mp([BIG_T, kv(("stream", "stdout"))]) + b, {"fluentbit.io/exclude_stdout": "true"}, pod="stream-stdout")
    add("wr_group_markers", w, a + GROUP_START + b + GROUP_END + a, pod="wr")
    add("wr_group_markers_only", w, GROUP_START + GROUP_END, pod="wr")
    add("wr_non_canonical", w, rec(R(b"\xde\x00\x04" + b"\xd9\x03log" + b"\xd9\x07{\"a\":1}" + b"\xa1i" + b"\xd3" + struct.pack(">q", 1) + b"\xda\x00\x01j" +
                                     b"\xd2\xff\xff\xff\xff" + b"\xa1u" + b"\xcf" + struct.pack(">Q", 5)), 1), pod="wr")
    add("wr_float32_and_ext", w, rec(kv(("log", "hit"), ("f", f32(1.5)), ("e", R(b"\xc7\x03\x05abc")), ("x", R(b"\xd6\x01abcd")), ("d", 2.5)), 1), pod="wr")
    add("wr_keys_that_are_no_str", w, rec(kv((R(b"\xc4\x01b"), 1), (7, "seven"), (None, 1), ("log", '{"a":1}')), 1), pod="wr")
    add("wr_empty_body", w, rec(kv(), 1), pod="wr")
    add("wr_namespace_only", w + [("namespace_labels", "on"), ("namespace_metadata_only", "on")], a + b, ns_meta="core.namespace_meta", pod="wr", ns="core")
    add("wr_pod_and_namespace", w + [("namespace_labels", "on"), ("namespace_annotations", "on")], a + b, ns_meta="core.namespace_meta", meta_file="core_base.meta",
        pod="wr-both", ns="core")
    add("wr_labels_and_annotations_off", w + [("labels", "off"), ("annotations", "off")], a, meta_file="core_base.meta", pod="wr-plain")
    # ---- tag mode (no files at all)
    T = [("use_tag_for_meta", "on")] + ML
    add("tag_stock", T, a + b, tag=tag_of("apache-logs", "default", "apache"))
    add("tag_pod_with_dots", T, a, tag=tag_of("my.pod-0.with.dots", "kube-system", "c"))
    add("tag_container_with_dashes", T, a, tag=tag_of("p", "n", "side-car--x_y"))
    add("tag_no_longer_than_prefix", T, a, tag="kube.var.log.containers.")
    add("tag_does_not_match", T, a, tag="kube.var.log.containers.Apache_default.log")
    add("tag_custom_prefix", T + [("kube_tag_prefix", "custom.")], a, tag="custom.pod_ns_c-%s.log" % DOCKER_ID)
    # ---- one call
    add("call_empty_chunk", w, b"", pod="wr")
    add("call_garbage_reserved_byte", w, a + b + b"\xc1\xff", pod="wr")
    add("call_cut_record", w, a + b + rec(kv(("log", "long value of a cut record")), 3)[:-4], pod="wr")
    add("call_non_map_body", w, a + synth.mp([[synth.ext_ts(3), {}], "text"]) + b, pod="wr")
    add("call_rows", w, b"".join(rec(kv(("log", "text" if i in (0, 63, 65) else '{"i":%d}' % i), *([("stream", "stderr")] if i in (5, 64) else [])), 100 + i)
                               for i in range(66)), pod="wr")
    # ---- refusals of this library that the reference starts with or without
    add("prop_unknown", [("nope", "1")], a, pod="wr")
    add("prop_bool_that_is_none", [("merge_log", "maybe")], a, pod="wr")
    return c


def build_reference(reference, engine, tmp):
    """compiles the plugin and tools/kube_ref_host.c into tmp: (host, plugin)"""
    so, host = os.path.join(tmp, "flb-filter_kubernetes.so"), os.path.join(tmp, "kube_ref_host")
    src = os.path.join(reference, "plugins", "filter_kubernetes")
    inc = includes(reference, engine)
    files = [os.path.join(src, f) for f in ("kubernetes.c", "kube_conf.c", "kube_meta.c", "kube_regex.c", "kube_property.c", "kubernetes_aws.c")]
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-w", "-D__FLB_FILENAME__=__FILE__"] + inc + ["-I" + os.path.join(reference, "lib"), "-I" + src, "-o", so] + files,
                   check=True)
    subprocess.run(["gcc", "-O2", "-Wall"] + inc + ["-o", host, os.path.join(ROOT, "tools", "kube_ref_host.c"),
                    "-L" + os.path.join(engine, "lib"), "-lfluent-bit", "-Wl,-rpath," + os.path.join(engine, "lib"), "-lpthread", "-ldl", "-lm"], check=True)
    return host, so


def is_true(v):
    return v.lower() in ("true", "on", "yes")


def excludes(c):
    """what flb_kube_prop_set_from_annotations keeps under k8s-logging.exclude on"""
    on = any(k.lower() == "k8s-logging.exclude" and is_true(v) for k, v in c["props"])
    ann = c["annotations"]
    both = on and is_true(ann.get("fluentbit.io/exclude", "false"))
    return (both or (on and is_true(ann.get("fluentbit.io/exclude_stdout", "false"))),
            both or (on and is_true(ann.get("fluentbit.io/exclude_stderr", "false"))))


def cut_maps(out):
    """the values of the last `kubernetes` / `kubernetes_namespace` pairs of every record: [(pod bytes|None, ns bytes|None)]"""
    res, p = [], 0
    while p < len(out):
        end, skip, sec, nsec, meta, body = mm.decode_event(out, p)
        pod = ns = None
        for k, v in body.v[-2:]:
            if k.t == "str" and k.v == b"kubernetes":
                pod = out[v.start:v.end]
            elif k.t == "str" and k.v == b"kubernetes_namespace":
                ns = out[v.start:v.end]
        res.append((pod, ns))
        p = end
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kube_ref_cases.json"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_kubernetes")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(os.path.join(engine, "lib", "libfluent-bit.so")):
        sys.exit("build the reference engine first: make -C oracle engine")
    ref_meta = os.path.join(a.reference, "tests", "runtime", "data", "kubernetes", "meta")
    out = []
    with tempfile.TemporaryDirectory(prefix="kube_golden_") as tmp:
        host, so = build_reference(a.reference, engine, tmp)
        fin, fout, cache = (os.path.join(tmp, n) for n in ("in.mp", "out.mp", "meta"))
        os.mkdir(cache)

        def run(c, props, data):
            with open(fin, "wb") as f:
                f.write(data)
            if os.path.exists(fout):
                os.unlink(fout)
            cmd = [host, so, fin, fout, c["tag"]] + ["%s=%s" % (k, v) for k, v in props]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if r.returncode < 0 or r.returncode >= 128:
                return "crashed", r
            if r.returncode != 0 or not lines:
                sys.exit("%s: kube_ref_host failed (%d): %s" % (c["name"], r.returncode, r.stderr.decode(errors="replace")[-600:]))
            res = json.loads(lines[-1])
            if not res["init"]:
                return "refused", r
            return (res["ret"], open(fout, "rb").read() if res["ret"] == MODIFIED else None), r
        for c in cases():
            e = dict(name=c["name"], props=c["props"], tag=c["tag"], **{"in": base64.b64encode(c["data"]).decode()})
            tag_mode = any(k.lower() == "use_tag_for_meta" and is_true(v) for k, v in c["props"])
            props = [tuple(p) for p in c["props"]]
            if not tag_mode:
                # the preloaded files: without them the plugin would ask the API server
                for f in os.listdir(cache):
                    os.unlink(os.path.join(cache, f))
                pod_file = os.path.join(cache, "%s_%s.meta" % (c["ns"], c["pod"]))
                with open(pod_file, "w") as f:
                    if c["meta_file"]:
                        f.write(open(os.path.join(ref_meta, c["meta_file"])).read())
                    else:
                        json.dump({"metadata": {"annotations": c["annotations"]}}, f)         # (as the reference's own exclude files are)
                if c["ns_meta"]:
                    with open(os.path.join(cache, "%s.namespace_meta" % c["ns"]), "w") as f:
                        f.write(open(os.path.join(ref_meta, c["ns_meta"])).read())
                want_ns = any(k.lower() in ("namespace_labels", "namespace_annotations") and is_true(v) for k, v in props)
                if not os.path.exists(pod_file) or (want_ns and not os.path.exists(os.path.join(cache, "%s.namespace_meta" % c["ns"]))):
                    sys.exit("%s: no preloaded file for the tag's pod -- the case is not run" % c["name"])
                props += [("kube_url", KUBE_URL), ("kube_meta_preload_cache_dir", cache)]
            res, r = run(c, props, c["data"])
            if res == "crashed":
                if c["name"] not in CRASHES:
                    sys.exit("%s: kube_ref_host died (%d): %s" % (c["name"], r.returncode, r.stderr.decode(errors="replace")[-600:]))
                e["crashed"] = True
            elif res == "refused":
                e["refused"] = True
            else:
                e["ret"], e["out"] = res[0], base64.b64encode(res[1]).decode() if res[1] is not None else None
                e["pod"] = e["ns"] = None
                if not tag_mode:
                    # the entries: cut out of a probe run that excludes nothing
                    probe = [(k, v) for k, v in props if k.lower() != "k8s-logging.exclude"]
                    pres, _ = run(c, probe, rec(kv(("probe", 1)), 1))
                    if pres in ("crashed", "refused") or pres[0] != MODIFIED:
                        sys.exit("%s: the probe run failed" % c["name"])
                    pod, ns = cut_maps(pres[1])[0]
                    if res[1]:
                        try:
                            same = set(cut_maps(res[1])) == {(pod, ns)}
                        except mm.Bad:
                            # an output nested past what the walker (and the decoder) takes: its end is looked at
                            same = res[1].endswith((b"\xaakubernetes" + pod if pod else b"") + (b"\xb4kubernetes_namespace" + ns if ns else b""))
                        if not same:
                            sys.exit("%s: the output records do not carry the probe's maps" % c["name"])
                    eo, ee = excludes(c)
                    e["pod"] = base64.b64encode(pod + km.props_array(eo, ee)).decode() if pod is not None else None
                    e["ns"] = base64.b64encode(ns).decode() if ns is not None else None
            out.append(e)
    with open(a.out, "w") as f:
        f.write('{"recorded_from": "the whole plugin (kubernetes.c, kube_conf.c, kube_meta.c, kube_regex.c, kube_property.c, kubernetes_aws.c) '
                'linked against the minimal engine; metadata from kube_meta_preload_cache_dir or the tag",\n "cases": [\n' +
                ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d cases (%d refused, %d crashed), %d bytes -> %s" % (len(out), sum(1 for e in out if e.get("refused")),
                                                                sum(1 for e in out if e.get("crashed")), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()

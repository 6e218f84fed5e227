#!/usr/bin/env python3
"""Records the answers of the real filter_expect for tests/golden/expect_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of
`make -C oracle engine` (oracle/_ref/engine).  The plugin's own source is compiled where it lies as a loadable flb-filter_expect.so in
a scratch directory outside the repository, next to tools/expect_ref_host.c -- this project's own host, which creates the filter
instance in the reference engine library and calls the plugin's cb_init / cb_filter.  Nothing compiled and no reference text enters
the repository, only the fixture: per case the properties, the input (base64), cb_filter's return value, the output when it is
FLB_FILTER_MODIFIED, config->exit_status_code after the call, the plugin's "exception on rule ..." lines (each up to and including
"Record content:") and the number of "expect check failed" lines as the host's stderr showed them -- or "refused": the filter did not
start, or "crashed": the host died.

The runtime test of the reference (tests/runtime/filter_expect.c) is transcribed first: its base configuration and its ten rules on
the records it pushes.  (tools/perf_expect.py --cpu-reference times the plugin through the same host.)"""
import argparse
import base64
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402
from gen_recmod_golden import includes  # noqa: E402
from expect_chunks import BIG_T, GROUP_END, GROUP_START, R, RULES, f32, kv, map_n, rec, rows, sv, type_records  # noqa: E402

# the cases at which the recording host may die (create refuses them)
CRASHES = ("eq_empty_value", "acc_refused")
LINE = re.compile(rb"exception on rule .*?Record content:", re.S)


def cases():
    c = []

    def add(name, props, data):
        c.append(dict(name=name, props=[list(p) for p in props], data=data))
    # ---- tests/runtime/filter_expect.c (legacy integer times, as the test's JSON input gives them)
    base = [("action", "result_key"), ("result_key", "result")]
    val, nul = synth.mp([0, kv(("key", "val"))]), synth.mp([0, kv(("key", None))])
    add("rt_base_configuration", base, val)
    add("rt_key_exists_matched", base + [("key_exists", "key")], val)
    add("rt_key_exists_not_matched", base + [("key_exists", "not_key")], val)
    add("rt_key_not_exists_matched", base + [("key_not_exists", "not_key")], val)
    add("rt_key_not_exists_not_matched", base + [("key_not_exists", "key")], val)
    add("rt_key_val_is_null_matched", base + [("key_val_is_null", "key")], nul)
    add("rt_key_val_is_null_not_matched", base + [("key_val_is_null", "key")], val)
    add("rt_key_val_is_not_null_matched", base + [("key_val_is_not_null", "key")], val)
    add("rt_key_val_is_not_null_not_matched", base + [("key_val_is_not_null", "key")], nul)
    add("rt_key_val_eq_matched", base + [("key_val_eq", "key val")], val)
    add("rt_key_val_eq_not_matched", base + [("key_val_eq", "not_key val")], val)
    # ---- every rule kind passing and failing, every value type under every rule
    mixed = rec(kv(("k", "val")), 1) + rec(kv(("k", None)), 2) + rec(kv(("x", 1)), 3) + rec(kv(("k", "other")), 4)
    types = type_records()
    for r in RULES:
        v = "$k val" if r == "key_val_eq" else "$k"
        add("rule_%s_warn" % r, [(r, v)], mixed)
        add("types_%s_warn" % r, [(r, v)], types)
        add("types_%s_result_key" % r, [(r, v), ("action", "result_key")], types)
    # ---- accessors
    deep = kv(("m", kv(("a", kv(("b", "hit"))), ("l", ["x", "hit", kv(("z", "other"))]))), ("log", "text"), ("s", "9"))
    acc = rec(deep, 1) + rec(kv(("m", kv(("a", 1), ("l", ["one"])))), 2) + rec(kv(("x", 1)), 3)
    for name, a in (("plain", "log"), ("dollar", "$log"), ("pre_dollar", "log$x"), ("tag", "$TAG"), ("subkeys", "$m['a']['b']"),
                    ("ends_on_index", "$m['l'][1]"), ("index_then_key", "$m['l'][2]['z']"), ("subkeys_on_a_str", "$s['a']")):
        add("acc_%s_exists" % name, [("key_exists", a)], acc)
    add("acc_tag_not_exists", [("key_not_exists", "$TAG")], acc)
    add("acc_refused", [("key_exists", "$log['x")], acc)
    add("acc_empty", [("key_exists", "")], acc)
    add("acc_empty_not_exists", [("key_not_exists", "")], acc)
    add("acc_only_a_dollar", [("key_exists", "$")], acc)
    add("acc_eq_refused",[("key_val_eq", "$log['x val")], acc)
    # ---- duplicate keys: the last one wins
    dup = rec(kv(("k", "val"), ("k", None)), 1) + rec(kv(("k", None), ("k", "val")), 2)
    add("dup_is_null", [("key_val_is_null", "$k")], dup)
    add("dup_eq", [("key_val_eq", "$k val")], dup)
    # ---- key_val_eq
    eq = (rec(kv(("k", "k")), 1) + rec(kv(("k", "a b  c")), 2) + rec(kv(("k", "c")), 3) + rec(kv(("k", sv(b"va\0l"))), 4) + rec(kv(("k", "")), 5) +
          rec(kv(("k", "va")), 6) + rec(kv(("k", "val")), 7) + rec(kv(("k", "value")), 8) + rec(kv(("k", sv(b"val\0"))), 9))
    add("eq_one_token", [("key_val_eq", "k")], eq)
    add("eq_one_token_dollar", [("key_val_eq", "$k")], eq)
    add("eq_empty_value", [("key_val_eq", "")], eq)
    add("eq_spaces_only", [("key_val_eq", "   ")], eq)
    add("eq_rest_of_the_line", [("key_val_eq", "$k a b  c")], eq)
    add("eq_trailing_and_leading_spaces", [("key_val_eq", "  $k   val  ")], eq)
    add("eq_val", [("key_val_eq", "$k val")], eq)
    add("eq_prefix_va", [("key_val_eq", "$k va")], eq)
    add("eq_longer_value", [("key_val_eq", "$k value")], eq)
    add("eq_result_key", [("key_val_eq", "$k val"), ("action", "result_key")], eq)
    # ---- the action, the result key, the properties
    two = rec(kv(("a", 1), ("matched", "old")), 1) + rec(kv(("b", 2)), 2) + rec(kv(("a", 3)), 3)
    for a in ("warn", "WARN", "Exit", "RESULT_KEY", "explode", ""):
        add("action_%s" % (a or "empty"), [("key_exists", "$a"), ("action", a)], two)
    add("action_set_twice", [("action", "warn"), ("key_exists", "$a"), ("action", "exit")], two)
    add("result_key_set_twice", [("action", "result_key"), ("result_key", "x"), ("result_key", "y")], two)
    add("unknown_property", [("key_exists", "$a"), ("nope", "1")], two)
    add("names_without_case", [("KEY_EXISTS", "$a"), ("Action", "result_key"), ("RESULT_KEY", "r")], two)
    add("result_key_empty", [("action", "result_key"), ("result_key", ""), ("key_exists", "$a")], two)
    add("result_key_in_body", [("action", "result_key"), ("key_exists", "$a")], two)
    add("result_key_default_without_rules", [("action", "result_key")], two)
    add("result_key_without_the_action", [("result_key", "r"), ("key_exists", "$a")], two)
    add("result_key_long", [("action", "result_key"), ("result_key", "r" * 300), ("key_exists", "$a")], two)
    add("numbering_action_between_rules", [("key_exists", "$a"), ("action", "warn"), ("key_not_exists", "$zz"), ("key_exists", "$a")], two)
    add("numbering_action_first", [("action", "warn"), ("key_exists", "$a")], two)
    add("numbering_result_key_between_rules", [("key_not_exists", "$zz"), ("result_key", "r"), ("key_exists", "$a")], two)
    add("no_rules_warn", [], two)
    add("no_rules_exit", [("action", "exit")], two)
    add("first_failing_rule_ends_the_record", [("key_exists", "$a"), ("key_exists", "$c"), ("key_not_exists", "$matched")], two)
    add("exit_stops_at_the_first_failure", [("key_exists", "$a"), ("action", "exit")], two + rec(kv(("b", 1)), 4))
    add("exit_without_a_failure", [("key_exists", "$a"), ("action", "exit")], rec(kv(("a", 1)), 1))
    # ---- the writer
    w = [("action", "result_key"), ("key_exists", "$log")]
    add("wr_keys_that_are_no_str", w, rec(kv((R(b"\xc4\x01b"), 1), ("log", "hit"), (7, "seven"), (None, 1), ("m", kv((1, 2), ("a", [1, {}])))), 1))
    add("wr_non_canonical_encodings", w, rec(R(b"\xde\x00\x04" + b"\xd9\x03log" + b"\xd9\x03hit" + b"\xa1i" + b"\xd3" + struct.pack(">q", 1) +
                                               b"\xda\x00\x01j" + b"\xd2\xff\xff\xff\xff" + b"\xa1u" + b"\xcf" + struct.pack(">Q", 5)), 1))
    add("wr_float32_and_ext", w, rec(kv(("log", "hit"), ("f", f32(1.5)), ("e", R(b"\xc7\x03\x05abc")), ("x", R(b"\xd6\x01abcd")), ("d", 2.5)), 1))
    add("wr_metadata", w, rec(kv(("log", "hit")), 5, 6, kv(("m", 1), ("z", [1, 2]))) +
        synth.mp([[synth.ext_ts(7, 8), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("nolog", "hit"))]))
    add("wr_empty_body", w, rec(kv(), 1))
    for n in (14, 15, 16):
        add("wr_body_of_%d_entries" % n, w, rec(map_n(n, ("log", "x")), 1))
    add("wr_integer_and_float_time", w, synth.mp([1700000000, kv(("log", "hit"))]) + synth.mp([1700000000.25, kv(("log", "hit"))]) +
        synth.mp([1700000001, kv(("nolog", "no"))]))
    big = synth.mp([BIG_T, kv(("log", "big"))])
    a, b = rec(kv(("log", "a")), 1), rec(kv(("nolog", "b")), 2)
    add("wr_time_the_encoder_refuses_first", w, big + a + b)
    add("wr_time_the_encoder_refuses_middle", w, a + big + b)
    add("wr_time_the_encoder_refuses_last", w, a + b + big)
    add("wr_time_the_encoder_refuses_alone", w, big)
    add("wr_time_the_encoder_refuses_warn", [("key_exists", "$nolog")], a + big + b)
    add("wr_float_time_minus_three", w, a + synth.mp([-3.0, kv(("log", "odd"))]) + b)
    add("wr_float_time_minus_three_warn", [("key_exists", "$nolog")], a + synth.mp([-3.0, kv(("log", "odd"))]) + b)
    add("wr_float_time_minus_one_and_a_half", w, a + synth.mp([-1.5, kv(("log", "odd"))]) + b)
    add("wr_float_time_minus_one", w, a + synth.mp([-1.0, kv(("log", "odd"))]) + b)
    # ---- group markers
    g = a + GROUP_START + b + GROUP_END + a
    for act in ("warn", "exit", "result_key"):
        add("groups_%s" % act, [("key_exists", "$log"), ("action", act)], g)
    add("groups_only_result_key", w, GROUP_START + GROUP_END)
    add("groups_at_both_ends_result_key", w, GROUP_START + b + a + GROUP_END)
    # ---- one call
    for act in ("warn", "exit", "result_key"):
        p = [("key_exists", "$log"), ("action", act)]
        add("call_empty_chunk_%s" % act, p, b"")
        add("call_garbage_reserved_byte_%s" % act, p, a + b + b"\xc1\xff")
        add("call_garbage_only_%s" % act, p, b"\xc1")
        add("call_cut_record_%s" % act, p, a + b + rec(kv(("log", "long value of a cut record")), 3)[:-4])
        add("call_cut_on_a_field_boundary_%s" % act, p, a + b + rec(kv(("log", "v"), ("x", "y")), 3)[:-2])
        add("call_non_map_body_%s" % act, p, a + synth.mp([[synth.ext_ts(3), {}], "text"]) + b)
    add("call_rows", [("key_exists", "$a"), ("key_val_is_not_null", "$a")], rows(70, (0, 5, 63, 64, 69)))
    return c


def build_reference(reference, engine, tmp):
    """compiles the plugin and tools/expect_ref_host.c into tmp: (host, plugin)"""
    so, host = os.path.join(tmp, "flb-filter_expect.so"), os.path.join(tmp, "expect_ref_host")
    src = os.path.join(reference, "plugins", "filter_expect")
    inc = includes(reference, engine)
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-maybe-uninitialized", "-D__FLB_FILENAME__=__FILE__"] + inc +
                   ["-I" + os.path.join(reference, "lib"), "-I" + src, "-o", so, os.path.join(src, "expect.c")], check=True)
    subprocess.run(["gcc", "-O2", "-Wall"] + inc + ["-o", host, os.path.join(ROOT, "tools", "expect_ref_host.c"),
                    "-L" + os.path.join(engine, "lib"), "-lfluent-bit", "-Wl,-rpath," + os.path.join(engine, "lib"), "-lpthread", "-ldl", "-lm"], check=True)
    return host, so


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "expect_ref_cases.json"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_expect")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(os.path.join(engine, "lib", "libfluent-bit.so")):
        sys.exit("build the reference engine first: make -C oracle engine")
    out = []
    with tempfile.TemporaryDirectory(prefix="expect_golden_") as tmp:
        host, so = build_reference(a.reference, engine, tmp)
        fin, fout = (os.path.join(tmp, n) for n in ("in.mp", "out.mp"))
        for c in cases():
            e = dict(name=c["name"], props=c["props"], **{"in": base64.b64encode(c["data"]).decode()})
            with open(fin, "wb") as f:
                f.write(c["data"])
            if os.path.exists(fout):
                os.unlink(fout)
            cmd = [host, so, fin, fout] + ["%s=%s" % (k, v) for k, v in c["props"]]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if r.returncode < 0 or r.returncode >= 128:
                if c["name"] not in CRASHES:
                    sys.exit("%s: expect_ref_host died (%d): %s" % (c["name"], r.returncode, r.stderr.decode(errors="replace")[-600:]))
                e["crashed"] = True
            elif r.returncode != 0 or not lines:
                sys.exit("%s: expect_ref_host failed (%d): %s" % (c["name"], r.returncode, r.stderr.decode(errors="replace")[-600:]))
            else:
                res = json.loads(lines[-1])
                if not res["init"]:
                    e["refused"] = True
                else:
                    e["ret"] = res["ret"]
                    e["out"] = base64.b64encode(open(fout, "rb").read()).decode() if res["ret"] == 1 else None
                    e["exit_status"] = res["exit_status"]
                    # the message from "exception on rule" on; the text in front of it is the logger's (time, level, instance name)
                    e["exceptions"] = [base64.b64encode(m).decode() for m in LINE.findall(r.stderr)]
                    e["check_failed"] = r.stderr.count(b"expect check failed")
            out.append(e)
    with open(a.out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d cases (%d refused, %d crashed), %d bytes -> %s" % (len(out), sum(1 for e in out if e.get("refused")),
                                                                sum(1 for e in out if e.get("crashed")), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()

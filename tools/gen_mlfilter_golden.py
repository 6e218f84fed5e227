#!/usr/bin/env python3
"""Records the answers of the real filter_multiline (mode parser, buffer off) for tests/golden/mlfilter_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of
`make -C oracle engine` (oracle/_ref/engine).  The plugin's own source is compiled where it lies, as a loadable
flb-filter_multiline.so in a scratch directory outside the repository, next to tools/mlfilter_ref_host.c -- this project's own host,
which defines the custom multiline parsers through the reference's flb_ml_parser_create / flb_ml_rule_create, creates the filter
instance in the reference engine library and calls the plugin's cb_init and, once per chunk of the case, cb_filter.  Nothing compiled
and no reference text enters the repository, only the fixture: per case the properties, the parser definitions, the buffer limit, the
chunks (base64), cb_filter's return values and the outputs where they are FLB_FILTER_MODIFIED -- or "refused": the filter did not start.

The records of the reference's runtime test flb_test_multiline_unbuffered (tests/runtime/filter_multiline.c) are one case, read as data
(tests/mlfilter_chunks.py REF_UNBUFFERED): the test pushes them one by one and expects six records, the first of which holds "panic"."""
import argparse
import base64
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402
from gen_recmod_golden import includes  # noqa: E402
import mlfilter_chunks as mc  # noqa: E402
from mlfilter_chunks import GROUP_END, GROUP_START, R, kv, logrec, rec  # noqa: E402


def cases():
    c = []

    def add(name, props, calls, parsers=(), limit=None, handed_back=False):
        c.append(dict(name=name, props=[list(p) for p in props], parsers=[mc.PARSERS[p] for p in parsers], limit=limit, calls=list(calls), handed_back=handed_back))

    def lines(texts, t0=0):
        return b"".join(logrec(t, t0 + i) for i, t in enumerate(texts))
    P = mc.props
    # ---- the reference's runtime test: one record per call
    add("rt_unbuffered", [("multiline.key_content", "log"), ("multiline.parser", "go"), ("buffer", "off"), ("debug_flush", "off")],
        [logrec(t, i) for i, t in enumerate(mc.REF_UNBUFFERED)])
    # ---- the built-ins, a trace per call and a trace cut across calls
    for name, trace in (("java", mc.JAVA_TRACE), ("go", mc.GO_TRACE), ("python", mc.PYTHON_TRACE), ("ruby", mc.RUBY_TRACE)):
        add("builtin_%s" % name, P(name), [lines(trace), lines(trace[:3], 100), lines(trace[3:], 200)])
    # ---- front end
    one = lines(["2024-03-01 start", "  cont"])
    add("fe_buffer_default_is_on", [("multiline.parser", "cont")], [one], ["cont"])
    for w in ("off", "OFF", "false", "no", "0", "on", "true", "yes", "1", "maybe", ""):
        add("fe_buffer_%s" % (w or "empty"), [("multiline.parser", "cont"), ("buffer", w)], [one], ["cont"])
    add("fe_no_key_content", [("multiline.parser", "cont"), ("buffer", "off")], [one], ["cont"])
    add("fe_names_without_case", [("Multiline.Parser", "cont"), ("BUFFER", "Off"), ("Multiline.Key_Content", "log"), ("Flush_Ms", "500"),
                                  ("Emitter_Name", "e"), ("emitter_storage.type", "memory"), ("emitter_mem_buf_limit", "1M"), ("debug_flush", "false")], [one], ["cont"])
    add("fe_mode_parser", P("cont", extra=[("mode", "PARSER")]), [one], ["cont"])
    add("fe_mode_partial_message", [("multiline.parser", "cont"), ("multiline.key_content", "log"), ("mode", "Partial_Message")], [], ["cont"])      # (no call: its first call wants the engine's scheduler)
    add("fe_mode_unknown", P("cont", extra=[("mode", "other")]), [one], ["cont"])
    add("fe_no_parser", [("buffer", "off"), ("multiline.key_content", "log")], [one])
    add("fe_unknown_parser", P("nope"), [one], ["cont"])
    add("fe_unknown_property", P("cont", extra=[("multiline.key_group", "x")]), [one], ["cont"])
    add("fe_two_parsers", P("cont, block"), [one], ["cont", "block"])
    add("fe_two_parser_lines", [("multiline.parser", "cont"), ("multiline.parser", "block")] + mc.OFF, [one], ["cont", "block"])
    add("fe_other_key", P("cont", key="message"), [rec(kv(("message", "2024-03-01 a"), ("log", "x")), 1) + rec(kv(("message", "  b")), 2) + rec(kv(("log", "  c")), 3)], ["cont"])
    # ---- records that are not processed
    add("nokey_record_without_the_key", P("cont"), [lines(["2024-03-01 a", "  b"]) + rec(kv(("msg", "  c")), 5) + lines(["  d"], 6)], ["cont"])
    add("nokey_non_str_value_with_str_duplicate", P("cont"),
        [rec(kv(("log", 5), ("x", 1), ("log", "2024-03-01 a")), 1) + rec(kv(("log", None), ("log", "  b")), 2) + rec(kv(("log", R(b"\xc4\x01z"))), 3)], ["cont"])
    add("nokey_two_str_entries_in_the_first_record", P("cont"),
        [rec(kv(("log", "2024-03-01 a"), ("m", 1), ("log", "second")), 1) + logrec("  b", 2)], ["cont"])
    add("nokey_second_entry_as_long_as_the_buffer", P("cont", key="message"),
        [rec(kv(("message", "2024-03-01"), ("2024-03-01", "x"), ("mes", "y"), ("message", "z")), 1),
         rec(kv(("message", "2024-03-01 "), ("m", 1), ("message\x00abc", "q")), 1)], ["cont"])
    add("nokey_bin_key", P("cont"), [rec(kv((R(b"\xc4\x03log"), "2024-03-01 a"), ("log", "2024-03-01 b")), 1)], ["cont"])
    add("nokey_no_rule_takes_it", P("cont"), [lines(["plain", "  cont without start", "2024-03-01 a", "plain again", "  b"])], ["cont"])
    add("nokey_non_map_body", P("cont"), [logrec("2024-03-01 a", 1) + synth.mp([[synth.ext_ts(3), {}], "text"]) + logrec("  b", 2)], ["cont"])
    add("nokey_empty_map", P("cont"), [logrec("2024-03-01 a", 1) + rec({}, 2) + rec(R(b"\xde\x00\x00"), 3)], ["cont"])
    # ---- other entries that are not canonical
    odd = kv(("i", R(b"\xd3" + (5).to_bytes(8, "big"))), ("log", "2024-03-01 a"), ("s", R(b"\xdb\x00\x00\x00\x02hi")), ("u", R(b"\xcf" + (7).to_bytes(8, "big"))),
             ("m", R(b"\xdf\x00\x00\x00\x01\xa1k\xdc\x00\x01\xd0\x05")), ("neg", R(b"\xd3" + (2 ** 64 - 3).to_bytes(8, "big"))), ("f", 1.5), ("e", R(b"\xc7\x01\x05x")))
    add("canon_first_record", P("cont"), [rec(odd, 1) + logrec("  b", 2)], ["cont"])
    add("canon_record_alone", P("cont"), [rec(kv(("i", R(b"\xd3" + (5).to_bytes(8, "big"))), ("s", R(b"\xdb\x00\x00\x00\x02hi"))), 1) +
                                          rec(kv(("log", "plain"), ("i", R(b"\xd1\x00\x05")), (R(b"\xda\x00\x01k"), "v")), 2)], ["cont"])
    add("canon_key_header", P("cont"), [rec(kv((R(b"\xd9\x03log"), "2024-03-01 a"), ("x", 1)), 1) + rec(kv((R(b"\xda\x00\x03log"), "  b")), 2)], ["cont"])
    # ---- state across calls
    add("state_continuation_opens_a_call", P("cont"), [lines(["2024-03-01 a", "  b"]), rec(kv(("x", 1), ("log", "  c")), 9, 9) + logrec("  d", 10), lines(["  e"], 20), lines(["plain"], 30), lines(["  f"], 40)], ["cont"])
    add("state_not_processed_between_start_and_continuation", P("cont"), [lines(["2024-03-01 a"]) + rec(kv(("msg", "x")), 5) + lines(["  b", "  c"], 6)], ["cont"])
    add("state_not_processed_across_calls", P("cont"), [lines(["2024-03-01 a"]), rec(kv(("msg", "x")), 5), lines(["  b"], 6)], ["cont"])
    add("state_flush_after_rule", P("block"), [lines(["BEGIN 1", " x", "END 1", "BEGIN 2", "END 2", " y", "BEGIN 3", " z"]), lines(["END 3", "other", "BEGIN 4", "END 4"], 50),
                                                lines(["BEGIN 5", "END 5"], 60) + rec(kv(("msg", "x")), 70), lines(["BEGIN 6"], 80), lines(["END 6"], 90), lines([" w"], 95)], ["block"])
    add("state_flush_after_rule_other_maps", P("block"),
        [rec(kv(("a", 1), ("log", "BEGIN 1")), 1, 1) + rec(kv(("b", 2), ("log", "END 1"), ("c", 3)), 2, 2) + rec(kv(("log", "BEGIN 2"), ("d", 4)), 3, 3) +
         rec(kv(("e", 5), ("log", " x")), 4, 4)], ["block"])
    # ---- calls
    add("call_empty_chunk", P("cont"), [b"", lines(["2024-03-01 a"]), b""], ["cont"])
    add("call_undecodable_bytes_behind_the_records", P("cont"), [lines(["2024-03-01 a", "  b"]) + b"\xc1\xff", lines(["  c"], 5) + logrec("  d", 6)[:-2], b"\xc1"], ["cont"])
    add("call_group_markers", P("cont"), [GROUP_START + lines(["2024-03-01 a"]) + GROUP_END + lines(["  b"], 3) + GROUP_START + GROUP_END, GROUP_START + GROUP_END], ["cont"])
    add("call_integer_and_float_time", P("cont"), [synth.mp([1700000000, kv(("log", "2024-03-01 a"))]) + synth.mp([1700000001, kv(("log", "  b"))]) +
                                                   synth.mp([1700000002.25, kv(("log", "2024-03-02 c"))]) + synth.mp([1700000003, kv(("msg", "x"))])], ["cont"])
    add("call_empty_content_as_continuation", P("emptycont"), [lines(["S1", "", "+x", "", "", "S2", ""]), lines(["", "+y"], 20)], ["emptycont"])
    add("call_empty_content_nobody_takes", P("cont"), [lines(["2024-03-01 a", "", "  b"])], ["cont"])
    add("call_mixed", P("cont"), [mc.mixed(40), mc.mixed(23, 4)], ["cont"])
    # ---- the buffer limit
    # (a group without a registered time takes the wall clock: every truncating start below follows a record that registered one)
    add("trunc_start", P("cont"), [lines(["plain", "2024-03-01 " + "a" * 40, "  b", "2024-03-02 c", "  d"])], ["cont"], limit="32")
    add("trunc_continuation", P("cont"), [lines(["2024-03-01 a", "  " + "b" * 10, "  " + "c" * 30, "  d", "2024-03-02 e", "  f"])], ["cont"], limit="32")
    add("trunc_continuation_exact_fit", P("cont"), [lines(["2024-03-01 " + "a" * 9, "  " + "b" * 9, "  c"])], ["cont"], limit="32")
    add("trunc_two_in_one_call", P("cont"), [lines(["2024-03-01 a", "  " + "b" * 40, "2024-03-02 e", "  " + "f" * 40, "  g"]) + rec(kv(("msg", 1)), 9) + lines(["2024-03-03 " + "h" * 30], 10),
                                             lines(["  i", "2024-03-04 j"], 20)], ["cont"], limit="32")
    add("trunc_start_then_empty_continuation", P("emptycont"), [lines(["other", "S" + "a" * 40]) + rec(kv(("e", 1), ("log", ""), ("f", 2)), 7, 7) + lines(["+b", "S2", "S" + "c" * 40, "+d"], 10)], ["emptycont"], limit="16")
    add("trunc_alone_is_not_cut", P("cont"), [lines(["plain " + "p" * 60, "2024-03-01 a"])], ["cont"], limit="32")
    # ---- endswith / equal
    ew = ["select 1", "from t;", "one;", "", "tail"]
    add("endswith", P("ew"), [lines(ew), lines([";", "x"], 10), rec(kv(("msg", 1)), 20) + lines(["y;"], 21)], ["ew"])
    add("endswith_negate", P("ewn"), [lines(["a \\", "b \\", "c", "d", "", "e \\"]), lines(["f"], 10)], ["ewn"])
    add("equal", P("eq"), [lines(["a", "b", "END", "END", "c"]), lines(["END"], 10) + rec(kv(("log", 5)), 11) + lines(["", "END"], 12)], ["eq"])
    add("equal_negate", P("eqn"), [lines(["...", "...", "go", "stop", "..."]), lines(["x"], 10)], ["eqn"])
    add("equal_empty_group", P("eq"), [rec(kv(("a", 1), ("log", "")), 1) + rec(kv(("log", "")), 2) + lines(["END"], 3)], ["eq"])
    # ---- what the device hands back at run time (-1): recorded so that the deviation rests on the reference's answer
    add("handed_back_empty_start", P("emptystart"),
        [rec(kv(("a", 1), ("log", "")), 1, 1) + rec(kv(("b", 2), ("log", "S2")), 2, 2) + rec(kv(("log", "+x")), 3, 3) + rec(kv(("c", 3), ("log", "")), 4, 4) +
         rec(kv(("d", 4), ("log", "")), 5, 5) + lines(["plain"], 6), lines(["S3", "+y"], 10)], ["emptystart"], handed_back=True)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mlfilter_ref_cases.json"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_multiline")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(os.path.join(engine, "lib", "libfluent-bit.so")):
        sys.exit("build the reference engine first: make -C oracle engine")
    out = []
    with tempfile.TemporaryDirectory(prefix="mlfilter_golden_") as tmp:
        so, host = os.path.join(tmp, "flb-filter_multiline.so"), os.path.join(tmp, "mlfilter_ref_host")
        src = os.path.join(a.reference, "plugins", "filter_multiline")
        inc = includes(a.reference, engine)
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__FLB_FILENAME__=__FILE__"] + inc +
                       ["-I" + os.path.join(a.reference, "lib"), "-I" + src, "-o", so, os.path.join(src, "ml.c"), os.path.join(src, "ml_concat.c")], check=True)
        subprocess.run(["gcc", "-O2", "-Wall", "-rdynamic"] + inc + ["-o", host, os.path.join(ROOT, "tools", "mlfilter_ref_host.c"),
                        "-L" + os.path.join(engine, "lib"), "-lfluent-bit", "-Wl,-rpath," + os.path.join(engine, "lib"), "-lpthread", "-ldl", "-lm"], check=True)
        for c in cases():
            e = dict(name=c["name"], props=c["props"], parsers=c["parsers"], limit=c["limit"], calls=[base64.b64encode(d).decode() for d in c["calls"]])
            if c["handed_back"]:
                e["handed_back"] = True
            for i, d in enumerate(c["calls"]):
                with open(os.path.join(tmp, "in_%d.mp" % i), "wb") as f:
                    f.write(d)
            cmd = [host, so, tmp, str(len(c["calls"])), c["limit"] or "-"]
            for p in c["parsers"]:
                cmd.append("P:%s:%s:%d:%s" % (p["name"], p["type"], p["negate"], p["match"].encode().hex()))
                cmd += ["R:%s:%s:%s:%s" % (p["name"], fr, to or "", rx.encode().hex()) for fr, rx, to in p["rules"]]
            cmd += ["%s=%s" % (k, v) for k, v in c["props"]]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                sys.exit("%s: mlfilter_ref_host failed (%d): %s" % (c["name"], r.returncode, r.stderr.decode()[-600:]))
            res = json.loads(lines[-1])
            if not res["init"]:
                e["refused"] = True
            else:
                e["rets"] = res["rets"]
                e["outs"] = [base64.b64encode(open(os.path.join(tmp, "out_%d.mp" % i), "rb").read()).decode() if ret == 1 else None
                             for i, ret in enumerate(res["rets"])]
            out.append(e)
    with open(a.out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d cases (%d refused), %d bytes -> %s" % (len(out), sum(1 for e in out if e.get("refused")), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()

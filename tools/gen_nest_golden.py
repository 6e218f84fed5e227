#!/usr/bin/env python3
"""Records the answers of the real filter_nest for tests/golden/nest_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of `make -C oracle`
(oracle/_ref/engine).  The plugin's own source is compiled where it lies, as a loadable flb-filter_nest.so in a scratch directory
outside the repository (the engine of oracle/build_engine.sh is a minimal build without it), with the include paths
tools/gen_recmod_golden.py uses.  Every case is one chunk through
`engine_host processor -e <.so> <in> <out> --unit nest k=v ...`; the file holds the properties, the input chunk and the output chunk
(base64) and "refused": the filter did not start.  The processor does not hand the callback's answer on, and MODIFIED with the
input's own bytes is this filter's usual answer, so the file records bytes only: what the processor hands back is the filter's
output -- or, where the filter answered NOTOUCH, the input -- through its group normalisation (src/flb_processor.c:1811-1852: the
records the decoder takes).  A case at which engine_host dies is written as "crashed": true without bytes; only the cases the
reference leaves undefined (UNDEFINED below) may end that way.

The runtime test of the reference (tests/runtime/filter_nest.c) is transcribed first: its four configurations, each with the records
it pushes (the two "multiple events" tests push two records through one instance)."""
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
from gen_recmod_golden import includes  # noqa: E402

R = synth.Raw
UNDEFINED = ("undef_remove_prefix_short_key", "undef_lift_int_key_with_prefix")


def rec(body, sec=0, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def kv(*items):
    return synth.KV(list(items))


def binkey(b):
    return R(b"\xc4" + bytes([len(b)]) + b)


NEST = [("Operation", "nest"), ("Nest_under", "n")]
LIFT = [("Operation", "lift"), ("Nested_under", "m")]
KEYS = kv(("k", 1), (binkey(b"kb"), 2), (7, 3), (None, 4), (True, 5), ("z", 6))
BAD_TIME = R(b"\xcf" + struct.pack(">Q", 2 ** 33))                      # a legacy integer time the EventTime cannot hold


def cases():
    c = []

    def add(name, props, data):
        c.append(dict(name=name, props=[list(p) for p in props], data=data))
    # ---- tests/runtime/filter_nest.c
    two = synth.mp([1448403340, kv(("to_nest", "This is the data to nest"), ("extra", "Some more data"))])
    rt_nest = [("Operation", "nest"), ("Wildcard", "to_nest"), ("Nest_under", "nested_key")]
    add("rt_single", rt_nest, two)
    add("rt_multi_nest", rt_nest, two + synth.mp([1448403341, kv(("not_nest", "dummy data"), ("extra", "dummy more data"))]))
    add("rt_multi_lift", [("Operation", "lift"), ("Nested_under", "nested")],
        synth.mp([1448403340, kv(("nested", kv(("child", "nested data"))), ("not_nestd", "not nested data"))]) +
        synth.mp([1448403341, kv(("not_nest", "dummy data"), ("extra", "dummy more data"))]))
    add("rt_add_prefix", [("Operation", "lift"), ("Nest_under", "nested_key"), ("Add_prefix", "_nested_key.")],
        synth.mp([1448403340, kv(("nested_key", kv(("key", "value"))))]))
    # ---- frontend
    one = rec(kv(("a", 1), ("b", 2), ("m", kv(("x", 1)))), 5, 6)
    add("operation_prefix_words", [("Operation", "nested"), ("Wildcard", "a"), ("Nest_under", "n")], one)
    add("operation_prefix_words_lifting", [("Operation", "lifting"), ("Nested_under", "m")], one)
    add("operation_prefix_words_Nest", [("Operation", "Nest"), ("Wildcard", "a"), ("Nest_under", "n")], one)
    add("unknown_property", NEST + [("Wildcard", "a"), ("Prefix_with", "p_")], one)
    add("both_prefixes", NEST + [("Wildcard", "a"), ("Add_prefix", "p_"), ("Remove_prefix", "q_")], one)
    add("last_key_wins", [("Operation", "nest"), ("Nest_under", "first"), ("Wildcard", "a"), ("Nested_under", "second")], one)
    add("last_key_wins_other_order", [("Operation", "nest"), ("Nested_under", "second"), ("Wildcard", "a"), ("Nest_under", "first")], one)
    add("same_property_twice_key", [("Operation", "nest"), ("Nest_under", "first"), ("Wildcard", "a"), ("Nest_under", "third")], one)
    add("same_property_twice_operation", [("Operation", "nest"), ("Operation", "lift"), ("Nested_under", "m")], one)
    add("same_property_twice_prefix", NEST + [("Wildcard", "a"), ("Add_prefix", "x"), ("Add_prefix", "y")], one)
    add("empty_key_and_prefix", [("Operation", "nest"), ("Wildcard", "a"), ("Nest_under", ""), ("Add_prefix", "")], one)
    add("nest_under_on_lift", [("Operation", "lift"), ("Nest_under", "m")], one)
    add("no_wildcards", NEST, one + rec(kv(("n", 1)), 7))
    add("nest_without_key", [("Operation", "nest"), ("Wildcard", "a")], rec(kv(("b", 1)), 1) + one + rec(kv(("c", 1)), 9))
    add("lift_without_key", [("Operation", "lift")],
        rec(kv(("", kv(("x", 1), ("y", 2))), ("m", kv(("z", 3)))), 1) + rec(kv(("", 5), ("q", 1)), 2))
    # ---- nest
    add("nest_exact_and_prefix", NEST + [("Wildcard", "host"), ("Wildcard", "k8s_*")],
        rec(kv(("host", "h"), ("k8s_pod", "p"), ("hostname", "no"), ("k8s_", 1), ("k8s", 2), ("log", "text")), 1, 2))
    add("nest_star", NEST + [("Wildcard", "*")], rec(KEYS, 1))
    add("nest_bin_key_with_prefix", NEST + [("Wildcard", "k*"), ("Add_prefix", "p.")], rec(KEYS, 1))
    add("nest_bin_key_no_prefix", NEST + [("Wildcard", "k*")], rec(KEYS, 1))
    add("nest_remove_prefix_partial", NEST + [("Wildcard", "*"), ("Remove_prefix", "app_")],
        rec(kv(("app_name", "x"), ("app_", "y"), ("apple", "z"), ("name", "w"), (binkey(b"app_b"), 1), (5, 6)), 1))
    add("nest_short_key_overread_hit", NEST + [("Wildcard", "ab*")], rec(kv(("a", 98), ("z", 1)), 1))
    add("nest_short_key_overread_miss", NEST + [("Wildcard", "ab*")], rec(kv(("a", 99), ("z", 1)), 1) + rec(kv(("a", "b")), 2))
    add("nest_none_match_next_to_match", NEST + [("Wildcard", "x")],
        rec(kv(("a", 1)), 1) + rec(kv(("x", 1), ("a", 2)), 2) + rec(kv(("b", 1)), 3) + rec(kv(("x", 3)), 4))
    noncanon = R(b"\xde\x00\x03" + b"\xda\x00\x03abc" + b"\xd1\x00\x07" + b"\xd9\x01x" + b"\xde\x00\x01\xd9\x01q\xd0\x05" + b"\xa1y\xd2\x00\x00\x00\x01")
    noncanon2 = R(b"\xde\x00\x02" + b"\xda\x00\x03abc" + b"\xd1\x00\x07" + b"\xa1y\xde\x00\x01\xd9\x01q\xd0\x05")
    add("nest_non_canonical", NEST + [("Wildcard", "x")], rec(noncanon, 1) + rec(noncanon2, 2))
    # ---- lift
    inner = kv(("pod", "p"), ("k8s_ns", "d"), (binkey(b"k8s_b"), 1), ("labels", kv(("app", "a"))))
    add("lift_plain", LIFT, rec(kv(("a", 1), ("m", inner), ("z", 2)), 1))
    add("lift_add_prefix", LIFT + [("Add_prefix", "k8s_")], rec(kv(("a", 1), ("m", inner), ("z", 2)), 1))
    add("lift_remove_prefix", LIFT + [("Remove_prefix", "k8s_")], rec(kv(("a", 1), ("m", inner), ("z", 2)), 1))
    add("lift_value_not_map", LIFT, rec(kv(("m", "text"), ("a", 1)), 1) + rec(kv(("m", [1, 2]), ("m", kv(("x", 1)))), 2))
    add("lift_duplicate_keys", LIFT, rec(kv(("m", kv(("x", 1))), ("a", 1), (binkey(b"m"), kv(("y", 2), ("x", 3))), ("m", kv(("x", 4)))), 1))
    add("lift_empty_inner_map", LIFT, rec(kv(("a", 1), ("m", {})), 1) + rec(kv(("m", {})), 2))
    add("lift_inner_int_key_no_prefix", LIFT, rec(kv(("m", kv((5, "five"), (None, 1), ("s", 2))), ("a", 1)), 1))
    add("lift_nested_two_levels", LIFT, rec(kv(("m", kv(("m", kv(("deep", 1))), ("x", 2))), ("a", 1)), 1))
    # ---- shared corners
    add("metadata", NEST + [("Wildcard", "x")],
        rec(kv(("x", 1), ("y", 2)), 5, 6, kv(("m", 1), ("z", [1, 2]))) +
        synth.mp([[synth.ext_ts(7, 8), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("x", 1), ("y", 2))]) +
        synth.mp([[synth.ext_ts(9, 1), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("y", 2))]))
    add("legacy_rows", LIFT,
        synth.mp([1700000000, kv(("m", kv(("k", 1))))]) + synth.mp([1700000000.25, kv(("m", kv(("k", 2))))]) +
        synth.mp([1700000001, kv(("k", 3))]) + synth.mp([R(b"\xd7\x00" + struct.pack(">II", 5, 6)), kv(("m", kv(("k", 4))))]))
    add("group_markers", NEST + [("Wildcard", "k")],
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), kv(("g", 1))], kv(("r", 1))]) + rec(kv(("k", 1)), 4) +
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xfe\x00\x00\x00\x00"), {}], {}]) + rec(kv(("k", 2)), 5))
    add("non_map_body", NEST + [("Wildcard", "x")],
        rec(kv(("x", 1), ("y", 2)), 1) + rec(kv(("y", 2)), 2) + synth.mp([[synth.ext_ts(3), {}], "text"]) + rec(kv(("x", 1)), 4))
    add("garbage_reserved_byte", NEST + [("Wildcard", "x")], rec(kv(("x", 1), ("y", 2))) + b"\xc1\xff")
    add("garbage_cut_record", LIFT, rec(kv(("m", kv(("y", 2))))) + rec(kv(("m", kv(("y", "long value")))))[:-4])
    add("empty_chunk_of_empty_maps", NEST + [("Wildcard", "*")], rec({}, 1) + rec({}, 2) + rec(R(b"\xde\x00\x00"), 3))
    add("bad_time_modified", NEST + [("Wildcard", "x")],
        rec(kv(("x", 1)), 1) + synth.mp([BAD_TIME, kv(("x", 2), ("y", 3))]) + rec(kv(("x", 3)), 3))
    add("bad_time_unmodified", NEST + [("Wildcard", "x")],
        rec(kv(("x", 1)), 1) + synth.mp([BAD_TIME, kv(("y", 3))]) + rec(kv(("x", 3)), 3))
    add("bad_time_lift", LIFT, synth.mp([BAD_TIME, kv(("m", kv(("x", 2))))]) + rec(kv(("m", kv(("x", 3)))), 3))
    # ---- what the reference leaves undefined: recorded to see whether it dies, never compared
    add("undef_remove_prefix_short_key", NEST + [("Wildcard", "*"), ("Remove_prefix", "ab")], rec(kv(("a", 98)), 1))
    add("undef_lift_int_key_with_prefix", LIFT + [("Add_prefix", "p_")], rec(kv(("m", kv((5, "five")))), 1))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "nest_ref_cases.json"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    host = os.path.join(engine, "engine_host")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_nest")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(host):
        sys.exit("build the reference engine first: make -C oracle")
    out = []
    with tempfile.TemporaryDirectory(prefix="nest_golden_") as tmp:
        so = os.path.join(tmp, "flb-filter_nest.so")
        src = os.path.join(a.reference, "plugins", "filter_nest")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__FLB_FILENAME__=__FILE__"] + includes(a.reference, engine) +
                       ["-I" + os.path.join(a.reference, "lib"), "-I" + src, "-o", so, os.path.join(src, "nest.c")], check=True)
        for c in cases():
            e = dict(name=c["name"], props=c["props"], **{"in": base64.b64encode(c["data"]).decode()})
            fin, fout = os.path.join(tmp, "in.mp"), os.path.join(tmp, "out.mp")
            with open(fin, "wb") as f:
                f.write(c["data"])
            if os.path.exists(fout):
                os.unlink(fout)
            cmd = [host, "processor", "-e", so, fin, fout, "--unit", "nest"] + ["%s=%s" % (k, v) for k, v in c["props"]]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if r.returncode < 0 or r.returncode >= 128:
                if c["name"] not in UNDEFINED:
                    sys.exit("%s: engine_host died (%d): %s" % (c["name"], r.returncode, r.stderr.decode()[-400:]))
                e["crashed"] = True
            elif not lines:
                # a property the config map refuses is reported before the processor starts
                if r.returncode == 3 or b"refused" in r.stderr:
                    e["refused"] = True
                else:
                    sys.exit("%s: engine_host said nothing (exit %d): %s" % (c["name"], r.returncode, r.stderr.decode()[-400:]))
            elif not json.loads(lines[-1]).get("init", True):
                e["refused"] = True
            else:
                e["out"] = base64.b64encode(open(fout, "rb").read()).decode()
            if c["name"] in UNDEFINED:
                e["undefined"] = True
            out.append(e)
    with open(a.out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d cases, %d bytes -> %s" % (len(out), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()

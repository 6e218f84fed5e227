#!/usr/bin/env python3
"""Records the answers of the real filter_type_converter for tests/golden/typeconv_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of
`make -C oracle engine` (oracle/_ref/engine).  The plugin's own source is compiled where it lies, as a loadable
flb-filter_type_converter.so in a scratch directory outside the repository (the engine of oracle/build_engine.sh is a minimal build
without it; src/flb_typecast.c is compiled in only when that engine's library does not export it), with the include paths
tools/gen_recmod_golden.py uses.  Every case is one chunk through
`engine_host processor -e <.so> <in> <out> --unit type_converter k=v ...`; the file holds the properties, the input chunk and the
output chunk (base64), "refused": the filter did not start, "crashed": engine_host died (only the cases of CRASHES may), and "undefined": a float -> int / uint conversion C leaves undefined is
in it.  The processor does not hand the callback's answer on, so the file records bytes only: what the processor hands back is the
filter's output -- or, where the filter answered NOTOUCH, the input -- through its group normalisation (src/flb_processor.c:1811-1852:
the records the decoder takes).

The runtime test of the reference (tests/runtime/filter_type_converter.c) is transcribed first: its seven configurations on the two
records it pushes."""
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
UNDEFINED = ("undef_float_to_int", "undef_float_to_uint")
# config_rule frees a rule it refuses with delete_conv_entry, which unlinks an entry that was never linked (type_converter.c:52,
# 95-100): the reference dies at an unknown type word and at a from_key the accessor refuses.  Recorded as "crashed"; create refuses.
CRASHES = ("fe_unknown_type_next_to_a_good_rule", "fe_unknown_type_only", "fe_accessor_refused_next_to_a_good_rule", "fe_accessor_refused_only")
BAD_TIME = R(b"\xcf" + struct.pack(">Q", 2 ** 33))                      # a legacy integer time the EventTime cannot hold


def rec(body, sec=0, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def kv(*items):
    return synth.KV(list(items))


def f32(v):
    return R(b"\xca" + struct.pack(">f", v))


def f64bits(b):
    return R(b"\xcb" + struct.pack(">Q", b))


def strs(*vals):
    """a body with the values under s0, s1, ..."""
    return kv(*[(b"s%d" % i, v) for i, v in enumerate(vals)])


def rules(prop, n, to, prefix="s"):
    return [(prop, "%s%d t%d %s" % (prefix, i, i, to)) for i in range(n)]


def cases():
    c = []

    def add(name, props, data):
        c.append(dict(name=name, props=[list(p) for p in props], data=data))
    # ---- tests/runtime/filter_type_converter.c
    flat = synth.mp([12345678, kv(("numstr", "123.456"), ("int", 123), ("float", 123.456), ("hexstr", "0xff"))])
    nest = synth.mp([12345678, kv(("nest", kv(("numstr", "123.456"), ("float", 123.456))))])
    add("rt_str_to_int", [("str_key", "numstr new int")], flat)
    add("rt_str_to_float", [("str_key", "numstr new float")], flat)
    add("rt_str_to_hex", [("str_key", "hexstr new hex")], flat)
    add("rt_int_to_str", [("int_key", "int new str")], flat)
    add("rt_int_to_float", [("int_key", "int new float")], flat)
    add("rt_str_int_and_int_str", [("str_key", "numstr new1 int"), ("int_key", "int new2 str")], flat)
    add("rt_nest_key", [("str_key", "$nest['numstr'] new int")], nest)
    # ---- front end
    one = rec(kv(("a", "12"), ("b", 7), ("c", 2.5), ("d", "0x1f")), 5, 6)
    add("fe_names_without_case_and_repeat", [("STR_KEY", "a a1 int"), ("Str_Key", "a a2 float"), ("INT_key", "b b1 string")], one)
    add("fe_two_tokens", [("str_key", "a a1")], one)
    add("fe_two_tokens_next_to_a_good_rule", [("str_key", "a a1 int"), ("int_key", "b b1")], one)
    add("fe_empty_value", [("str_key", "")], one)
    add("fe_four_tokens_skipped", [("str_key", "a a1 int extra"), ("int_key", "b b1 string")], one)
    add("fe_four_tokens_only", [("str_key", "a a1 int extra")], one)
    add("fe_unknown_type_next_to_a_good_rule", [("str_key", "a a1 integer"), ("str_key", "a a2 strings"), ("int_key", "b b1 string")], one)
    add("fe_unknown_type_only", [("str_key", "a a1 integer")], one)
    add("fe_unknown_property", [("str_key", "a a1 int"), ("bool_key", "a a2 string")], one)
    add("fe_quoted_tokens", [("str_key", '"a" "a 1" int')], one)
    add("fe_rule_order_is_configures", [("float_key", "c o4 string"), ("uint_key", "b o3 string"), ("int_key", "b o2 string"),
                                        ("str_key", "a o1 int"), ("str_key", "d o0 hex")], one)
    add("fe_type_words_prefix", [("str_key", "a t0 i"), ("str_key", "a t1 u"), ("str_key", "a t2 f"), ("str_key", "d t3 h"),
                                 ("int_key", "b t4 s"), ("int_key", "b t5 str"), ("str_key", "a t6 b"), ("str_key", "a t7 IN"),
                                 ("str_key", "a t8 UiNt"), ("int_key", "b t9 STRING"), ("str_key", "a t10 in"), ("str_key", "a t11 fl")], one)
    add("fe_type_word_empty_is_int", [("str_key", 'a t0 ""')], one)
    add("fe_unsupported_pairs_start", [("str_key", "a t0 string"), ("int_key", "b t1 int"), ("int_key", "b t2 hex"), ("int_key", "b t3 bool"),
                                       ("uint_key", "b t4 uint"), ("float_key", "c t5 float"), ("float_key", "c t6 bool"),
                                       ("float_key", "c t7 hex"), ("uint_key", "b t8 hex")], one)
    acc = rec(kv(("pre", "11"), ("key", "22"), ("TAG", "33"), ("0", "44"), ("a", "55"), ("a.b", "66"), ("$a", "77"), ("b", "88")), 1)
    add("fe_accessor_pre_dollar", [("str_key", "pre$key t int")], acc)
    add("fe_accessor_tag", [("str_key", "$TAG t int"), ("str_key", "b tb int")], acc)
    add("fe_accessor_regex_id", [("str_key", "$0 t int"), ("str_key", "b tb int")], acc)
    add("fe_accessor_dot", [("str_key", "$a.b t int")], acc)
    add("fe_accessor_plain_name_with_dot", [("str_key", "a.b t int")], acc)
    add("fe_accessor_dollar_alone", [("str_key", "$ t int"), ("str_key", "b tb int")], acc)
    add("fe_accessor_refused_next_to_a_good_rule", [("str_key", "$a['x t int"), ("str_key", "$a[x] t2 int"), ("str_key", "b tb int")], acc)
    add("fe_accessor_refused_only", [("str_key", "$a['x t int")], acc)
    # ---- lookups
    deep = kv(("m", kv(("a", kv(("b", "7"))), ("l", ["1", "2", kv(("z", "3"))]), ("a", kv(("b", "8"))))), ("s", "9"), ("n", 5))
    add("lk_subkeys", [("str_key", "$m['a']['b'] t0 int"), ("str_key", "$m['l'][1] t1 int"), ("str_key", "$m['l'][2]['z'] t2 int"),
                       ("str_key", "$m['nope'] t3 int"), ("str_key", "$m['l'][9] t4 int"), ("str_key", "$m t5 int")], rec(deep, 1))
    add("lk_subkeys_on_scalar_ignored", [("str_key", "$s['a']['b'] t0 int"), ("int_key", "$n['q'] t1 string")], rec(deep, 1))
    add("lk_duplicate_top_level_key", [("str_key", "a t int")], rec(kv(("a", "1"), ("b", 2), ("a", "3"), ("c", 4)), 1))
    add("lk_duplicate_inner_key", [("str_key", "$m['a'] t int")], rec(kv(("m", kv(("a", "1"), ("a", "2")))), 1))
    add("lk_bin_key_never_matches", [("str_key", "a t int")], rec(kv((R(b"\xc4\x01a"), "1"), ("b", "2")), 1) + rec(kv(("a", "5")), 2))
    add("lk_to_key_equals_existing_key", [("str_key", "a a int"), ("str_key", "a b float")], rec(kv(("a", "12"), ("b", "x")), 1))
    add("lk_two_rules_on_one_key", [("str_key", "a t0 int"), ("str_key", "a t1 float"), ("str_key", "a t2 bool")], rec(kv(("a", "12")), 1))
    add("lk_lookup_on_original_body", [("str_key", "a n int"), ("int_key", "n n2 string")], rec(kv(("a", "12")), 1))
    add("lk_key_absent", [("str_key", "zz t int"), ("str_key", "a t1 int")], rec(kv(("a", "12")), 1) + rec(kv(("b", "12")), 2))
    # ---- str -> int / uint / hex
    ints = ["0", "abc", "", "  -0", "12", "-12", "+12", " \t\n\v\f\r7", "12abc", "1\x002", "9223372036854775807", "9223372036854775808",
            "-9223372036854775808", "-9223372036854775809", "18446744073709551615", "18446744073709551616", "-1",
            "123456789012345678901234567890", "0x1f", "- 5", "+-5", "1.9e3"]
    add("cv_str_to_int", rules("str_key", len(ints), "int"), rec(strs(*ints), 1))
    add("cv_str_to_uint", rules("str_key", len(ints), "uint"), rec(strs(*ints), 1))
    hexs = ["0", "0x", "0xg", "0x1F", "0X1f", "ff", "-ff", "  +0xA", "0xffffffffffffffff", "0x10000000000000000", "g", "12", "0x0", "x1", "0b1"]
    add("cv_str_to_hex", rules("str_key", len(hexs), "hex"), rec(strs(*hexs), 1))
    flts = ["abc", "", "1.5", "-0", "1e400", "-1e400", "nan", "-nan", "nan(0x12)", "nan(abc)", "NAN(123", "inf", "-Infinity", "0x1.8p1",
            "  12.5xyz", "1\x002", ".", "1e", "4.9e-324", "2.2250738585072011e-308", "123.456"]
    add("cv_str_to_float", rules("str_key", len(flts), "float"), rec(strs(*flts), 1))
    bools = ["true", "false", "TRUE", "False", "TRUEish", "falsey", "tru", "fals", "yes", "", "1", " true", "t\x00rue"]
    add("cv_str_to_bool", rules("str_key", len(bools), "bool"), rec(strs(*bools), 1))
    add("cv_str_source_of_other_types", rules("str_key", 8, "int"), rec(strs(5, -5, 1.5, True, None, R(b"\xc4\x012"), ["1"], {"a": "1"}), 1))
    # ---- int / uint sources
    nums = [0, 1, -1, 127, 128, -32, -33, 2 ** 31, -2 ** 31 - 1, 2 ** 53 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, -2 ** 63,
            R(b"\xd3" + struct.pack(">q", 5)), R(b"\xd0\xfb"), 9007199254740993, 2 ** 63 + 1025]
    for prop in ("int_key", "uint_key"):
        for to in ("string", "float", "uint" if prop == "int_key" else "int"):
            add("cv_%s_to_%s" % (prop[:-4], to), rules(prop, len(nums), to), rec(strs(*nums), 1))
    add("cv_int_source_of_other_types", rules("int_key", 6, "string") + rules("uint_key", 6, "string", "s"),
        rec(strs("5", 1.5, f32(2.0), True, None, [1]), 1))
    # ---- float source
    fl = [0.0, -0.0, 1.0, -1.5, 123.456, 1e22, 2.0 ** 63 - 1024, -(2.0 ** 63), 1e15, 1e16, 123456789012345680.0, 0.1, 1e-7, 5e-324, f32(1.5),
          f32(0.1), f32(-3.0), float("inf"), float("-inf"), f64bits(0x7ff8000000000000), f64bits(0xfff8000000000000),
          f64bits(0x7ff8000000000123), 2.0 ** 63, -(2.0 ** 63) - 2048, 2.0 ** 64]
    add("cv_float_to_string", rules("float_key", len(fl), "string"), rec(strs(*fl), 1))
    defined = [0.0, -0.0, 1.0, -1.5, 123.456, 1e15, 2.0 ** 63 - 1024, -(2.0 ** 63) + 1024, 0.9, -0.9, f32(1.5), f32(-3.0), 5e-324]
    add("cv_float_to_int", rules("float_key", len(defined), "int"), rec(strs(*defined), 1))
    udef = [0.0, 1.0, 123.456, 2.0 ** 63 - 1024, 2.0 ** 63, 2.0 ** 63 + 2048, 2.0 ** 64 - 2048, 0.9, -0.9, -0.0, f32(1.5)]
    add("cv_float_to_uint", rules("float_key", len(udef), "uint"), rec(strs(*udef), 1))
    add("cv_float_source_of_other_types", rules("float_key", 5, "string"), rec(strs(5, -5, "1.5", True, None), 1))
    bad = [f64bits(0x7ff8000000000000), f64bits(0xfff8000000000001), float("inf"), float("-inf"), 2.0 ** 63, -(2.0 ** 63), -(2.0 ** 63) - 2048,
           1e300, -1.0, -1.5, 2.0 ** 64, -1e300, 1.8446744073709552e19 * 2]
    bad_int = [v for v in bad if v not in (-1.0, -1.5)]                 # (every value of a case is undefined for its target)
    add("undef_float_to_int", rules("float_key", len(bad_int), "int"), rec(strs(*bad_int), 1))
    bad_uint = [v for v in bad if v != 2.0 ** 63]
    add("undef_float_to_uint", rules("float_key", len(bad_uint), "uint"), rec(strs(*bad_uint), 1))
    # ---- one call
    conv = [("str_key", "x xi int")]
    add("call_notouch_no_conversion_succeeds", conv, rec(kv(("x", "abc"), ("y", 2)), 1) + rec(kv(("y", 2)), 2) + rec(kv(("x", 5)), 3))
    add("call_one_success_marks_the_chunk", conv, rec(kv(("x", "abc")), 1) + rec(kv(("y", 2)), 2) + rec(kv(("x", "5")), 3))
    noncanon = R(b"\xde\x00\x03" + b"\xda\x00\x01x" + b"\xd9\x017" + b"\xd9\x01q" + b"\xde\x00\x01\xd9\x01q\xd0\x05" + b"\xa1y\xd2\x00\x00\x00\x01")
    add("call_non_canonical_entries", conv, rec(noncanon, 1) + rec(kv(("x", R(b"\xdb\x00\x00\x00\x0242"))), 2))
    add("call_wide_body_header", conv, rec(R(b"\xde\x00\x11" + b"".join(synth.mp("k%d" % i) + synth.mp(i) for i in range(16)) + synth.mp("x") + synth.mp("3")), 1))
    add("metadata", conv,
        rec(kv(("x", "1"), ("y", 2)), 5, 6, kv(("m", 1), ("z", [1, 2]))) +
        synth.mp([[synth.ext_ts(7, 8), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("x", "1"), ("y", 2))]) +
        synth.mp([[synth.ext_ts(9, 1), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("y", 2))]))
    add("legacy_rows", conv,
        synth.mp([1700000000, kv(("x", "1"))]) + synth.mp([1700000000.25, kv(("x", "2"))]) +
        synth.mp([1700000001, kv(("k", 3))]) + synth.mp([R(b"\xd7\x00" + struct.pack(">II", 5, 6)), kv(("x", "4"))]))
    add("group_markers", conv,
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), kv(("g", 1))], kv(("r", 1))]) + rec(kv(("x", "1")), 4) +
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xfe\x00\x00\x00\x00"), {}], {}]) + rec(kv(("x", "2")), 5))
    add("non_map_body", conv,
        rec(kv(("x", "1"), ("y", 2)), 1) + rec(kv(("y", 2)), 2) + synth.mp([[synth.ext_ts(3), {}], "text"]) + rec(kv(("x", "1")), 4))
    add("garbage_reserved_byte", conv, rec(kv(("x", "1"), ("y", 2))) + b"\xc1\xff")
    add("garbage_cut_record", conv, rec(kv(("x", "1"))) + rec(kv(("x", "long value of a cut record")))[:-4])
    add("cut_record_on_a_field_boundary", conv, rec(kv(("x", "1"))) + rec(kv(("x", "2"), ("y", "abcd")))[:-5])
    add("bad_time", conv, rec(kv(("x", "1")), 1) + synth.mp([BAD_TIME, kv(("x", "2"), ("y", 3))]) + rec(kv(("x", "3")), 3))
    add("bad_time_float", conv, synth.mp([-5.5, kv(("x", "2"))]) + synth.mp([2.0 ** 40, kv(("x", "3"))]) + rec(kv(("x", "3")), 3))
    add("empty_maps", conv, rec({}, 1) + rec(kv(("x", "7")), 2) + rec(R(b"\xde\x00\x00"), 3))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "typeconv_ref_cases.json"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    host = os.path.join(engine, "engine_host")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_type_converter")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(host):
        sys.exit("build the reference engine first: make -C oracle engine")
    out = []
    with tempfile.TemporaryDirectory(prefix="typeconv_golden_") as tmp:
        so = os.path.join(tmp, "flb-filter_type_converter.so")
        src = os.path.join(a.reference, "plugins", "filter_type_converter")
        files = [os.path.join(src, "type_converter.c")]
        syms = subprocess.run(["nm", "-D", os.path.join(engine, "lib", "libfluent-bit.so")], stdout=subprocess.PIPE, check=True).stdout
        if b" T flb_typecast_pack" not in syms:
            files.append(os.path.join(a.reference, "src", "flb_typecast.c"))
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__FLB_FILENAME__=__FILE__"] + includes(a.reference, engine) +
                       ["-I" + os.path.join(a.reference, "lib"), "-I" + src, "-o", so] + files, check=True)
        for c in cases():
            e = dict(name=c["name"], props=c["props"], **{"in": base64.b64encode(c["data"]).decode()})
            fin, fout = os.path.join(tmp, "in.mp"), os.path.join(tmp, "out.mp")
            with open(fin, "wb") as f:
                f.write(c["data"])
            if os.path.exists(fout):
                os.unlink(fout)
            cmd = [host, "processor", "-e", so, fin, fout, "--unit", "type_converter"] + ["%s=%s" % (k, v) for k, v in c["props"]]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if r.returncode < 0 or r.returncode >= 128:
                if c["name"] not in CRASHES:
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

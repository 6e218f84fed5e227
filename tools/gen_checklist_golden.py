#!/usr/bin/env python3
"""Records the answers of the real filter_checklist for tests/golden/checklist_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF), the reference engine of
`make -C oracle engine` (oracle/_ref/engine) and the machine's libsqlite3.  The plugin's own source and src/flb_sqldb.c are compiled
where they lie, against the tree's sqlite3.h, as a loadable flb-filter_checklist.so in a scratch directory outside the repository,
next to tools/checklist_ref_host.c -- this project's own host, which creates the filter instance in the reference engine library
and calls the plugin's cb_init / cb_filter (its header says how it lives with an engine built without FLB_SQLDB).  Nothing compiled
and no reference text enters the repository, only the fixture: per case the properties ("@LIST@" stands for the list file's path,
"@MISSING@" for a path that does not exist), the list file's bytes (base64, or null), the input (base64), cb_filter's return value
and the output when it is FLB_FILTER_MODIFIED -- or "refused": the filter did not start, or "crashed": the host died.

The runtime test of the reference (tests/runtime/filter_checklist.c) is transcribed first: its five configurations on the records
it pushes."""
import argparse
import base64
import glob
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
from checklist_chunks import GROUP_END, GROUP_START, LIST, MISSING, R, f32, kv, rec, sv  # noqa: E402

# the cases at which the recording host may die (create refuses them)
CRASHES = ("fe_accessor_refused", "ld_nul_at_line_start")


def cases():
    c = []

    def add(name, props, lst, data):
        c.append(dict(name=name, props=[list(p) for p in props], list=lst, data=data))
    base = [("file", LIST), ("lookup_key", "secret"), ("record", "secret ----")]
    # ---- tests/runtime/filter_checklist.c (legacy integer times, as the test's JSON input gives them)
    mal, conf = synth.mp([0, kv(("secret", "malicious word"))]), synth.mp([0, kv(("secret", "confidential"))])
    add("rt_lookup_key", base, b"malicious word\n", mal)
    add("rt_lookup_keys", base, b"malicious word\nconfidential\n", mal + conf)
    add("rt_records", base + [("record", "checklist true")], b"malicious word\n", mal)
    add("rt_ignore_case", base + [("ignore_case", "true")], b"MaliCioUs Word\n", mal)
    add("rt_mode_partial", base + [("mode", "partial")], b"malicious\n", mal)
    # ---- front end
    lst = b"hit\nother\n"
    one = rec(kv(("log", "hit"), ("b", "q")), 5, 6) + rec(kv(("log", "miss"), ("b", "q")), 7, 8)
    f = [("file", LIST)]
    add("fe_no_record", f, lst, one)
    add("fe_names_without_case", [("FILE", LIST), ("Lookup_Key", "log"), ("MODE", "EXACT"), ("Ignore_Case", "Off"), ("RECORD", "k v"),
                                  ("print_query_time", "false")], lst, one)
    add("fe_duplicate_record_keys", f + [("record", "k one"), ("record", "k two"), ("record", "b three")], lst, one)
    add("fe_record_replaces_lookup_key", f + [("record", "log gone")], lst, one)
    add("fe_record_value_kinds", f + [("record", "t true"), ("record", "f FALSE"), ("record", "n Null"), ("record", "s truex")], lst, one)
    add("fe_record_value_is_last_entry", f + [("record", "k my val"), ("record", 'q "a b" c  d e')], lst, one)
    add("fe_record_one_token", f + [("record", "k")], lst, one)
    add("fe_record_empty", f + [("record", "")], lst, one)
    add("fe_unknown_property", f + [("nope", "1")], lst, one)
    add("fe_bad_bool", f + [("ignore_case", "maybe")], lst, one)
    add("fe_mode_word_partial_case", f + [("mode", "Partial"), ("record", "k v")], b"hi\n", one)
    add("fe_mode_word_unknown_is_exact", f + [("mode", "fuzzy"), ("record", "k v")], b"hi\nhit\n", one)
    add("fe_mode_set_twice", f + [("mode", "partial"), ("mode", "exact"), ("record", "k v")], b"hi\n", one)
    add("fe_no_file", [("record", "k v")], None, one)
    add("fe_missing_file", [("file", MISSING), ("record", "k v")], None, one)
    add("fe_default_lookup_key", f + [("record", "k v")], lst, one)
    add("fe_accessor_dollar", f + [("lookup_key", "$log"), ("record", "k v")], lst, one)
    add("fe_accessor_pre_dollar", f + [("lookup_key", "log$x"), ("record", "k v")], lst, one)
    add("fe_accessor_tag_never_finds", f + [("lookup_key", "$TAG"), ("record", "k v")], lst, one)
    add("fe_accessor_refused", f + [("lookup_key", "$log['x"), ("record", "k v")], lst, one)
    # ---- the list loader
    val = rec(kv(("log", "abc")), 1) + rec(kv(("log", "zzz")), 2) + rec(kv(("log", "last")), 3)
    r = [("file", LIST), ("record", "k v")]
    add("ld_empty_file", r, b"", val)
    add("ld_comments_only", r, b"# abc\n#zzz\n\n\n", val)
    add("ld_crlf", r, b"abc\r\nlast\r\n", val)
    add("ld_cr_inside_stays", r, b"ab\rc\nabc\r\r\n", rec(kv(("log", "ab\rc")), 1) + rec(kv(("log", "abc\r")), 2) + rec(kv(("log", "abc")), 3))
    add("ld_last_line_without_newline", r, b"abc\nlast", val)
    add("ld_empty_lines_between", r, b"\n\nabc\n\n\r\nlast\n", val)
    for n in (2045, 2046, 2047):
        long_ = b"L" * n
        v2 = rec(kv(("log", sv(long_))), 1) + rec(kv(("log", "abc")), 3) + rec(kv(("log", "last")), 4) + rec(kv(("log", "L")), 5)
        add("ld_line_%d_in_the_middle" % n, r, b"abc\n" + long_ + b"\nlast\n", v2)
        add("ld_line_%d_last_with_newline" % n, r, b"abc\n" + long_ + b"\n", v2)
        add("ld_line_%d_last_without_newline" % n, r, b"abc\n" + long_, v2)
    add("ld_nul_in_the_middle_of_a_line", r, b"abc\nla\0st\nzzz\n", val + rec(kv(("log", "la")), 4))
    add("ld_nul_in_the_last_line_without_newline", r, b"abc\nla\0st", val + rec(kv(("log", "la")), 4))
    add("ld_nul_at_line_start", r, b"abc\n\0st\nzzz\n", val)
    add("ld_entry_percent_exact", r, b"%\n", rec(kv(("log", "%")), 1) + rec(kv(("log", "abc")), 2))
    add("ld_entry_percent_partial", r + [("mode", "partial")], b"%\n", rec(kv(("log", "%")), 1) + rec(kv(("log", "")), 2) + rec(kv(("log", 5)), 3))
    add("ld_ignore_case_high_bytes", r + [("ignore_case", "on")], b"\xc3\x89COLE\n\xc0Z\xff\n",
        rec(kv(("log", sv(b"\xc3\x89cole"))), 1) + rec(kv(("log", sv(b"\xc3\xa9cole"))), 2) + rec(kv(("log", sv(b"\xc0z\xff"))), 3) +
        rec(kv(("log", sv(b"\xe0Z\xff"))), 4))
    add("ld_ignore_case_partial", r + [("ignore_case", "on"), ("mode", "partial")], b"AB_d\n", rec(kv(("log", "abXD-")), 1) + rec(kv(("log", "aBxd")), 2) +
        rec(kv(("log", "abd")), 3))
    # ---- the lookup value
    lk = [("file", LIST), ("record", "k v")]
    add("lk_value_types", lk, lst, rec(kv(("log", R(b"\xc4\x03hit"))), 1) + rec(kv(("log", 5)), 2) + rec(kv(("log", kv(("hit", 1)))), 3) +
        rec(kv(("log", None)), 4) + rec(kv(("log", ["hit"])), 5) + rec(kv(("log", True)), 6) + rec(kv(("log", 1.5)), 7) + rec(kv(("log", "hit")), 8))
    add("lk_duplicate_key_str_then_int", lk, lst, rec(kv(("log", "hit"), ("log", 5)), 1) + rec(kv(("x", 1)), 2) + rec(kv(("log", "hit")), 3))
    add("lk_duplicate_key_int_then_str", lk, lst, rec(kv(("log", 5), ("log", "hit")), 1) + rec(kv(("x", 1)), 2))
    deep = kv(("m", kv(("a", kv(("b", "hit"))), ("l", ["x", "hit", kv(("z", "other"))]))), ("s", "9"))
    add("lk_subkey_path", lk + [("lookup_key", "$m['a']['b']")], lst, rec(deep, 1) + rec(kv(("m", kv(("a", 1)))), 2))
    add("lk_path_ends_on_index", lk + [("lookup_key", "$m['l'][1]")], lst, rec(deep, 1) + rec(kv(("m", kv(("l", ["hit"])))), 2))
    add("lk_index_then_key", lk + [("lookup_key", "$m['l'][2]['z']")], lst, rec(deep, 1) + rec(kv(("m", 1)), 2))
    add("lk_subkeys_on_a_str_ignored", lk + [("lookup_key", "$s['a']")], b"9\n", rec(deep, 1))
    add("lk_empty_str_value", lk, b"hit\n", rec(kv(("log", "")), 1) + rec(kv(("log", "hit")), 2))
    add("lk_empty_str_value_partial", lk + [("mode", "partial")], b"hit\n", rec(kv(("log", "")), 1) + rec(kv(("log", "hit")), 2))
    add("lk_value_with_nul", lk, b"ab\n", rec(kv(("log", sv(b"ab\0cd"))), 1) + rec(kv(("log", "ab")), 2))
    add("lk_value_with_nul_partial", lk + [("mode", "partial")], b"ab%d\nzz\n", rec(kv(("log", sv(b"ab\0cd"))), 1) + rec(kv(("log", sv(b"zz\0"))), 2))
    add("lk_partial_utf8", lk + [("mode", "partial")], b"a_b\n", rec(kv(("log", sv(b"a\xc3\xa9\xa9\xa9b"))), 1) + rec(kv(("log", sv(b"a\xa9b"))), 2) +
        rec(kv(("log", sv(b"a\xc3\xa9\xc3\xa9b"))), 3))
    add("lk_partial_overlong", lk + [("mode", "partial")], b"a\xc1\x81b\n", rec(kv(("log", sv(b"a\xc0\x80b"))), 1) + rec(kv(("log", "aAb")), 2))
    # ---- the writer
    w = [("file", LIST), ("record", "k v"), ("record", "flag true")]
    add("wr_keys_that_are_no_str", w, lst, rec(kv((R(b"\xc4\x01b"), 1), ("log", "hit"), (7, "seven"), (None, 1), ("m", kv((1, 2), ("a", [1, {}])))), 1))
    add("wr_non_canonical_encodings", w, lst, rec(R(b"\xde\x00\x04" + b"\xd9\x03log" + b"\xd9\x03hit" + b"\xa1i" + b"\xd3" + struct.pack(">q", 1) +
                                                    b"\xda\x00\x01j" + b"\xd2\xff\xff\xff\xff" + b"\xa1u" + b"\xcf" + struct.pack(">Q", 5)), 1))
    add("wr_float32_and_ext", w, lst, rec(kv(("log", "hit"), ("f", f32(1.5)), ("e", R(b"\xc7\x03\x05abc")), ("x", R(b"\xd6\x01abcd")), ("d", 2.5)), 1))
    add("wr_record_key_in_body_twice", w, lst, rec(kv(("k", 1), ("log", "hit"), ("k", 2), ("flag", "old")), 1))
    add("wr_metadata", w, lst, rec(kv(("log", "hit")), 5, 6, kv(("m", 1), ("z", [1, 2]))) +
        synth.mp([[synth.ext_ts(7, 8), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("log", "hit"))]))
    add("wr_integer_and_float_time", w, lst, synth.mp([1700000000, kv(("log", "hit"))]) + synth.mp([1700000000.25, kv(("log", "hit"))]) +
        synth.mp([1700000001, kv(("log", "no"))]))
    big_t = R(b"\xcf" + struct.pack(">Q", 2 ** 33))
    add("wr_time_the_encoder_refuses", w, lst, rec(kv(("log", "no")), 1) + synth.mp([big_t, kv(("log", "hit"))]) + rec(kv(("log", "no")), 3))
    add("wr_refused_first_record_then_nothing", w, lst, synth.mp([big_t, kv(("log", "hit"))]) + rec(kv(("log", "no")), 3))
    add("wr_refused_first_record_then_a_match", w, lst, synth.mp([big_t, kv(("log", "hit"))]) + rec(kv(("log", "no")), 3) + rec(kv(("log", "hit")), 4) +
        rec(kv(("log", "no")), 5))
    add("wr_wide_body_header", w, lst, rec(R(b"\xde\x00\x11" + b"".join(synth.mp("k%d" % i) + synth.mp(i) for i in range(16)) + synth.mp("log") + synth.mp("hit")), 1))
    # ---- one call
    hit, no = kv(("log", "hit")), kv(("log", "no"))
    add("call_matches_only_at_the_end", w, lst, rec(no, 1) + rec(no, 2) + rec(no, 3) + rec(hit, 4))
    add("call_matches_only_at_the_start", w, lst, rec(hit, 1) + rec(no, 2) + rec(no, 3))
    add("call_no_match", w, lst, rec(no, 1) + rec(no, 2))
    add("call_every_record_matches", w, lst, rec(hit, 1) + rec(hit, 2))
    add("call_group_markers_in_front_of_a_match", w, lst, rec(no, 1) + GROUP_START + rec(hit, 2) + GROUP_END + rec(no, 3))
    add("call_group_markers_in_front_of_an_unmatched_record", w, lst, rec(hit, 1) + GROUP_START + rec(no, 2) + GROUP_END + rec(no, 3) + GROUP_START + GROUP_END)
    add("call_group_markers_before_the_first_match", w, lst, GROUP_START + rec(no, 1) + GROUP_END + rec(no, 2) + GROUP_START + rec(hit, 3) + rec(no, 4))
    add("call_garbage_reserved_byte", w, lst, rec(hit, 1) + rec(no, 2) + b"\xc1\xff")
    add("call_garbage_cut_record", w, lst, rec(no, 1) + rec(hit, 2) + rec(kv(("log", "long value of a cut record")), 3)[:-4])
    add("call_garbage_without_a_match", w, lst, rec(no, 1) + b"\xc1")
    add("call_non_map_body_ends_the_loop", w, lst, rec(hit, 1) + synth.mp([[synth.ext_ts(3), {}], "text"]) + rec(hit, 4))
    add("call_empty_chunk", w, lst, b"")
    return c


def build_reference(reference, engine, tmp, sqlite=None):
    """compiles the plugin (with src/flb_sqldb.c) and tools/checklist_ref_host.c into tmp: (host, plugin)"""
    sqlite = sqlite or next(iter(sorted(glob.glob("/usr/lib*/**/libsqlite3.so.0", recursive=True))), None)
    hdr = sorted(glob.glob(os.path.join(reference, "lib", "sqlite-amalgamation-*", "sqlite3.h")))
    if not sqlite or not hdr:
        sys.exit("need libsqlite3.so.0 on this machine and sqlite3.h in the reference tree")
    so, host = os.path.join(tmp, "flb-filter_checklist.so"), os.path.join(tmp, "checklist_ref_host")
    src = os.path.join(reference, "plugins", "filter_checklist")
    inc = includes(reference, engine) + ["-I" + os.path.dirname(hdr[0]), "-DFLB_HAVE_SQLDB"]
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-maybe-uninitialized", "-D__FLB_FILENAME__=__FILE__"] + inc +
                   ["-I" + os.path.join(reference, "lib"), "-I" + src, "-o", so, os.path.join(src, "checklist.c"),
                    os.path.join(reference, "src", "flb_sqldb.c"), sqlite], check=True)
    subprocess.run(["gcc", "-O2", "-Wall"] + inc + ["-o", host, os.path.join(ROOT, "tools", "checklist_ref_host.c"),
                    "-L" + os.path.join(engine, "lib"), "-lfluent-bit", "-Wl,-rpath," + os.path.join(engine, "lib"), "-lpthread", "-ldl", "-lm"], check=True)
    return host, so


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "checklist_ref_cases.json"))
    ap.add_argument("--sqlite", default=None, help="libsqlite3.so.0 to link (default: the first one under /usr/lib*)")
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_checklist")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(os.path.join(engine, "lib", "libfluent-bit.so")):
        sys.exit("build the reference engine first: make -C oracle engine")
    out = []
    with tempfile.TemporaryDirectory(prefix="checklist_golden_") as tmp:
        host, so = build_reference(a.reference, engine, tmp, a.sqlite)
        fin, fout, flist = (os.path.join(tmp, n) for n in ("in.mp", "out.mp", "list.txt"))
        for c in cases():
            e = dict(name=c["name"], props=c["props"], list=base64.b64encode(c["list"]).decode() if c["list"] is not None else None,
                     **{"in": base64.b64encode(c["data"]).decode()})
            with open(fin, "wb") as f:
                f.write(c["data"])
            for p in (fout, flist):
                if os.path.exists(p):
                    os.unlink(p)
            if c["list"] is not None:
                with open(flist, "wb") as f:
                    f.write(c["list"])
            sub = {"@LIST@": flist, "@MISSING@": os.path.join(tmp, "no_such_file")}
            cmd = [host, so, fin, fout] + ["%s=%s" % (k, sub.get(v, v)) for k, v in c["props"]]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if r.returncode < 0 or r.returncode >= 128:
                if c["name"] not in CRASHES:
                    sys.exit("%s: checklist_ref_host died (%d): %s" % (c["name"], r.returncode, r.stderr.decode()[-600:]))
                e["crashed"] = True
            elif r.returncode != 0 or not lines:
                sys.exit("%s: checklist_ref_host failed (%d): %s" % (c["name"], r.returncode, r.stderr.decode()[-600:]))
            else:
                res = json.loads(lines[-1])
                if not res["init"]:
                    e["refused"] = True
                else:
                    e["ret"] = res["ret"]
                    e["out"] = base64.b64encode(open(fout, "rb").read()).decode() if res["ret"] == 1 else None
            out.append(e)
    with open(a.out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d cases (%d refused, %d crashed), %d bytes -> %s" % (len(out), sum(1 for e in out if e.get("refused")),
                                                                sum(1 for e in out if e.get("crashed")), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()

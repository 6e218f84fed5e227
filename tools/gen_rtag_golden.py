#!/usr/bin/env python3
"""Records the answers of the real filter_rewrite_tag for tests/golden/rtag_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of
`make -C oracle engine` (oracle/_ref/engine).  The plugin's own source is compiled where it lies, as a loadable
flb-filter_rewrite_tag.so in a scratch directory outside the repository, next to tools/rtag_ref_host.c -- this project's own host,
which creates the filter instance in the reference engine library, calls the plugin's cb_init / cb_filter and stands where the
emitter stands (it defines in_emitter_add_record and records what it is handed; on request it answers -1 for chosen emissions).
oracle/engine_host cannot do that: its two modes show neither cb_filter's answer nor the emitted tags.  Nothing compiled and no
reference text enters the repository, only the fixture: per case the properties, the tag, the input (base64), cb_filter's return
value, the output when it is FLB_FILTER_MODIFIED, the list of (tag, bytes, refused) the emitter saw -- or "refused": the filter did
not start.  A case at which the host dies ends the recording.

The runtime test of the reference (tests/runtime/filter_rewrite_tag.c) is transcribed first: its configurations on the records it
pushes."""
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
from rtag_chunks import GROUP_END, GROUP_START, R, f32, f64bits, kv, rec  # noqa: E402


def cases():
    c = []

    def add(name, props, data, tag=b"rewrite", refuse=()):
        c.append(dict(name=name, props=[list(p) for p in props], data=data, tag=tag, refuse=list(refuse)))
    # ---- tests/runtime/filter_rewrite_tag.c (legacy integer times, as the test's JSON input gives them)
    def rt(body, t=1448403340):
        return synth.mp([t, body])
    add("rt_matched", [("Rule", "$key1 ^(rewrite)$ updated false")], rt(kv(("key1", "rewrite"))))
    add("rt_not_matched", [("Rule", "$key1 ^(rewrite)$ updated false")], rt(kv(("key1", "not_match"))))
    add("rt_keep_true", [("Rule", "$key1 ^(rewrite)$ updated true")], rt(kv(("key1", "rewrite"))))
    add("rt_heavy_input_pause_emitter", [("Rule", "$key1 ^(rewrite)$ updated false"), ("emitter_mem_buf_limit", "1kb")],
        b"".join(rt(kv(("key1", "rewrite"), ("n", i))) for i in range(8)))
    add("rt_issue_4793", [("Rule", "$destination $TAG[0] updated false")],                      # never matches: the pattern is taken literally
        rt(kv(("destination", "server"))), tag=b"rewrite")
    add("rt_issue_4793_subkey", [("Rule", "$log['destination'] ^(server)$ $TAG.$1 false")], rt(kv(("log", kv(("destination", "server"))))))
    add("rt_issue_4518", [("Rule", "$test ^(true)$ updated true"), ("Rule", "$test ^(hello)$ updated2 true")],
        rt(kv(("test", "hello"))) + rt(kv(("test", "true"))) + rt(kv(("test", "other"))))
    add("rt_issue_5846_tag_as_key", [("Rule", "$TAG ^(rewrite)$ updated false"), ("Rule", "$TAG[0] ^(rewrite)$ updated false")],
        rt(kv(("key1", "rewrite"), ("TAG", "rewrite"))))
    add("rt_busy_emitter_keeps_original", [("Rule", "$key1 ^(rewrite)$ updated false")], rt(kv(("key1", "rewrite"))), refuse=[0])
    # ---- front end
    one = rec(kv(("a", "xyz"), ("b", "q")), 5, 6)
    add("fe_names_without_case", [("RULE", "$a ^x r1 false"), ("Emitter_Name", "e1"), ("EMITTER_STORAGE.TYPE", "Memory"), ("emitter_mem_buf_limit", "5M")], one)
    # ("emitter_storage.type filesystem" passes cb_init's check and then depends on the service's own storage: not recorded)
    add("fe_quoted_entries", [("Rule", '"$a" "^x y?z" "new tag" "false"')], one)
    add("fe_three_entries", [("Rule", "$a ^x r1")], one)
    add("fe_three_entries_next_to_a_good_rule", [("Rule", "$a ^x r1 false"), ("Rule", "$b ^q r2")], one)
    add("fe_fifth_word", [("Rule", "$a ^x r1 true and more words")], one)
    add("fe_fifth_word_keep_false", [("Rule", "$a ^x r1 false true")], one)
    for w in ("true", "TRUE", "on", "On", "yes", "YES", "false", "off", "no", "1", "0", "y", "truee", ""):
        add("fe_keep_%s" % (w or "empty"), [("Rule", '$a ^x r1 "%s"' % w)], one)
    add("fe_bad_regex", [("Rule", "$a ^(x r1 false")], one)
    add("fe_bad_regex_next_to_a_good_rule", [("Rule", "$a ^x r1 false"), ("Rule", "$b [q r2 false")], one)
    add("fe_bad_storage_type", [("Rule", "$a ^x r1 false"), ("emitter_storage.type", "disk")], one)
    add("fe_no_rule", [], one)
    add("fe_no_rule_but_emitter_name", [("emitter_name", "e2")], one)
    add("fe_unknown_property", [("Rule", "$a ^x r1 false"), ("Match_Rule", "x")], one)
    add("fe_regex_options", [("Rule", "$a /^XYZ$/i r1 false")], one)
    add("fe_key_accessor_refused", [("Rule", "$a['x ^x r1 false")], one)
    add("fe_tag_accessor_refused", [("Rule", "$a ^x r.$a[x] false")], one)
    # ---- keys
    dup = rec(kv(("a", "first"), ("b", 1), ("a", "second")), 1)
    add("key_duplicate_last_wins", [("Rule", "$a ^second$ t false")], dup)
    add("key_duplicate_first_is_not_seen", [("Rule", "$a ^first$ t false")], dup)
    add("key_plain_name", [("Rule", "a ^second$ t.$a false")], dup)
    add("key_text_in_front_of_dollar", [("Rule", "a$b ^second$ t false")], dup)
    add("key_bin_never_matches", [("Rule", "$a ^x t false")], rec(kv((R(b"\xc4\x01a"), "x")), 1) + rec(kv(("a", "x")), 2))
    vals = [5, -5, 2 ** 63 + 5, 1.5, f32(2.0), True, False, None, R(b"\xc4\x01x"), ["x"], kv(("x", "x")), R(b"\xd5\x01xx")]
    add("key_values_of_other_types", [("Rule", "$v . t.$v true")], b"".join(rec(kv(("v", v)), i) for i, v in enumerate(vals)))
    deep = kv(("m", kv(("a", kv(("b", "7"))), ("l", ["x1", "x2", kv(("z", "x3"))]), ("a", kv(("b", "8"))))), ("s", "x9"), ("n", 5))
    add("key_subkeys", [("Rule", "$m['a']['b'] ^8$ t1 true"), ("Rule", "$m['l'][1] ^x2$ t2 true")], rec(deep, 1))
    add("key_subkeys_map_then_array_then_map", [("Rule", "$m['l'][2]['z'] ^x3$ t3.$m['l'][2]['z'].$m['l'][0] false")], rec(deep, 1))
    add("key_subkey_missing", [("Rule", "$m['nope'] . t true"), ("Rule", "$m['l'][9] . t true"), ("Rule", "$m . t true")], rec(deep, 1))
    add("key_subkey_on_scalar", [("Rule", "$s['a']['b'] ^x9$ t.$s['q'] false"), ("Rule", "$n['q'] . t true")], rec(deep, 1))
    add("key_first_rule_wins", [("Rule", "$s ^x t1 true"), ("Rule", "$s ^x9 t2 false")], rec(deep, 1))
    add("key_regex_id_never_matches", [("Rule", "$0 . t false"), ("Rule", "$s ^x t2 true")], rec(deep, 1))
    # ---- templates
    types = kv(("s", "text"), ("i", -42), ("u", 2 ** 63 + 1), ("big", 2 ** 64 - 1), ("f", 1.5), ("f32", f32(0.1)), ("nz", -0.0), ("huge", 1e300),
               ("nan", f64bits(0x7ff8000000000000)), ("nnan", f64bits(0xfff8000000000000)), ("inf", float("-inf")), ("t", True), ("fa", False),
               ("nil", None), ("bin", R(b"\xc4\x03\x00\xab\xff")), ("arr", [1, 2]), ("ext", R(b"\xd5\x01ab")),
               ("map", kv(("k", "é\"\\\n"), ("n", 1), ("f", 2.5), ("l", [1, kv(("x", None))]), ("k", "dup"))), ("e", ""), ("log", "go"))
    for k in ("s", "i", "u", "big", "f", "f32", "nz", "huge", "nan", "nnan", "inf", "t", "fa", "nil", "bin", "arr", "ext", "map", "e", "missing"):
        add("tpl_value_%s" % k, [("Rule", "$log ^go$ v.$%s.w false" % k)], rec(types, 1))
    add("tpl_f_just_under_the_buffer", [("Rule", "$log ^go$ $a,$b,$c false")],
        rec(kv(("log", "go"), ("a", 1e22), ("b", 1e23), ("c", -1e22)), 1))                          # "%f": 30, 31 and 31 characters
    add("tpl_all_kinds", [("Rule", "$log ^(g)(o)$ lit.$TAG.$TAG[1].$1$2.$0.$s.$m['k'] false")], rec(kv(("log", "go"), ("s", "v"), ("m", kv(("k", "w")))), 1), tag=b"a.b.c")
    add("tpl_text_around_keys", [("Rule", "$log ^go$ pre-$s,post.$TAG false")], rec(types, 1), tag=b"tg")
    add("tpl_key_ends_at_dot", [("Rule", "$log ^go$ $s.x false")], rec(types, 1))
    add("tpl_dollar_alone", [("Rule", "$log ^go$ a$ false")], rec(types, 1))
    add("tpl_only_dollar", [("Rule", "$log ^go$ $ false")], rec(types, 1))
    for tag in (b"plain", b"a.b", b"a.b.c.d", b"", b".", b"a..b", b"a.", b".a"):
        add("tpl_tag_parts_of_%s" % (tag.decode() or "empty"), [("Rule", "$log ^go$ [$TAG[0]|$TAG[1]|$TAG[2]|$TAG[3]|$TAG[7]|$TAG] false")], rec(types, 1), tag=tag)
    add("tpl_tag_part_forms", [("Rule", "$log ^go$ [$TAG[]|$TAG[x]|$TAG[-1]|$TAG[1|$TAGS|$TAG[01]] false")], rec(types, 1), tag=b"a.b.c")
    cap = rec(kv(("log", "ab-12 tail")), 1)
    add("tpl_captures", [("Rule", "$log ^([a-z]+)-(\\d+)(x)?(?:\\s)(.*)$ $0|$1|$2|$3|$4|$5|$9 false")], cap)
    add("tpl_capture_not_at_start", [("Rule", "$log (\\d)(\\d) $0|$1|$2 false")], cap)
    add("tpl_captures_no_groups", [("Rule", "$log ^ab $0|$1 false")], cap)
    add("tpl_captures_named", [("Rule", "$log ^(?<w>[a-z]+)-(\\d+) $0|$1|$2 false")], cap)
    add("tpl_captures_two_digits", [("Rule", "$log ^(a)(b) $10|$1 false")], cap)
    add("tpl_captures_utf8", [("Rule", "$log ^(\\S+)\\s(.)(.*)$ $2|$1|$3 false")], rec(kv(("log", "café €uro")), 1))
    add("tpl_empty_tag", [("Rule", '$log ^go$ "" false')], rec(types, 1))
    add("tpl_empty_tag_from_missing_key", [("Rule", "$log ^go$ $missing true")], rec(types, 1))
    add("tpl_300_byte_tag", [("Rule", "$log ^go$ $long.$TAG false")], rec(kv(("log", "go"), ("long", "t" * 290)), 1), tag=b"123456789")
    # ---- calls
    m = [("Rule", "$log ^m t.$n false")]
    mk = [("Rule", "$log ^m t.$n true")]
    recs = [rec(kv(("log", "m" if i % 2 else "x"), ("n", i)), 10 + i) for i in range(6)]
    add("call_group_marker_in_front_of_a_match", m, recs[0] + GROUP_START + recs[1] + GROUP_END + recs[2] + recs[3])
    add("call_group_markers_and_keep", mk, GROUP_START + recs[1] + recs[3] + GROUP_END + GROUP_START + GROUP_END + recs[5])
    add("call_legacy_times", m, synth.mp([1700000000, kv(("log", "m"), ("n", 1))]) + synth.mp([1700000000.25, kv(("log", "m"), ("n", 2))]) +
        synth.mp([R(b"\xd7\x00" + struct.pack(">II", 5, 6)), kv(("log", "m"), ("n", 3))]) + synth.mp([1700000001, kv(("log", "x"))]))
    add("call_metadata", m, rec(kv(("log", "m"), ("n", 1)), 5, 6, kv(("meta", 1))) + rec(kv(("log", "x")), 7, 8, kv(("meta", 2))))
    add("call_trailing_garbage", m, recs[1] + recs[2] + recs[3] + b"\xc1\xff")
    add("call_cut_record", m, recs[1] + recs[2] + recs[3][:-3])
    add("call_bad_record_in_the_middle", m, recs[1] + synth.mp([[synth.ext_ts(3), {}], "text"]) + recs[3])
    add("call_bad_record_first", m, synth.mp([[synth.ext_ts(3), {}], "text"]) + recs[3])
    add("call_all_matched_keep_false", m, recs[1] + recs[3] + recs[5])
    add("call_all_matched_keep_true", mk, recs[1] + recs[3] + recs[5])
    add("call_none_matched", m, recs[0] + recs[2] + recs[4])
    add("call_refused_in_the_middle", m, b"".join(recs), refuse=[1])
    add("call_all_refused", m, b"".join(recs), refuse=[0, 1, 2])
    add("call_refused_with_keep_true", mk, b"".join(recs), refuse=[0, 2])
    add("call_refused_in_front_of_garbage", m, recs[1] + recs[3] + b"\xc1", refuse=[0])
    add("call_empty_maps", m, rec({}, 1) + recs[1] + rec(R(b"\xde\x00\x00"), 3))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rtag_ref_cases.json"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_rewrite_tag")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(os.path.join(engine, "lib", "libfluent-bit.so")):
        sys.exit("build the reference engine first: make -C oracle engine")
    out = []
    with tempfile.TemporaryDirectory(prefix="rtag_golden_") as tmp:
        so, host = os.path.join(tmp, "flb-filter_rewrite_tag.so"), os.path.join(tmp, "rtag_ref_host")
        src = os.path.join(a.reference, "plugins", "filter_rewrite_tag")
        inc = includes(a.reference, engine)
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__FLB_FILENAME__=__FILE__"] + inc +
                       ["-I" + os.path.join(a.reference, "lib"), "-I" + src, "-o", so, os.path.join(src, "rewrite_tag.c")], check=True)
        subprocess.run(["gcc", "-O2", "-Wall", "-rdynamic"] + inc + ["-o", host, os.path.join(ROOT, "tools", "rtag_ref_host.c"),
                        "-L" + os.path.join(engine, "lib"), "-lfluent-bit", "-Wl,-rpath," + os.path.join(engine, "lib"), "-lpthread", "-ldl", "-lm"], check=True)
        fin, fout, fem = (os.path.join(tmp, n) for n in ("in.mp", "out.mp", "emitted.bin"))
        for c in cases():
            e = dict(name=c["name"], props=c["props"], tag=base64.b64encode(c["tag"]).decode(), refuse=c["refuse"],
                     **{"in": base64.b64encode(c["data"]).decode()})
            with open(fin, "wb") as f:
                f.write(c["data"])
            for p in (fout, fem):
                if os.path.exists(p):
                    os.unlink(p)
            cmd = [host, so, fin, fout, fem, c["tag"].hex() or "-", ",".join(str(i) for i in c["refuse"]) or "-"] + ["%s=%s" % (k, v) for k, v in c["props"]]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                sys.exit("%s: rtag_ref_host failed (%d): %s" % (c["name"], r.returncode, r.stderr.decode()[-600:]))
            res = json.loads(lines[-1])
            if not res["init"]:
                e["refused"] = True
            else:
                e["ret"] = res["ret"]
                e["out"] = base64.b64encode(open(fout, "rb").read()).decode() if res["ret"] == 1 else None
                em, raw, p = [], open(fem, "rb").read(), 0
                while p < len(raw):
                    tl = struct.unpack_from("<I", raw, p)[0]
                    tag = raw[p + 4:p + 4 + tl]
                    p += 4 + tl
                    bl = struct.unpack_from("<I", raw, p)[0]
                    buf = raw[p + 4:p + 4 + bl]
                    p += 4 + bl
                    em.append([base64.b64encode(tag).decode(), base64.b64encode(buf).decode(), raw[p]])
                    p += 1
                assert len(em) == res["emitted"] + res["refused"], (c["name"], res, len(em))
                e["emitter"] = em
            out.append(e)
    with open(a.out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d cases (%d refused), %d bytes -> %s" % (len(out), sum(1 for e in out if e.get("refused")), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()

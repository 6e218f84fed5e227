#!/usr/bin/env python3
"""Records the answers of the real filter_record_modifier for tests/golden/recmod_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of `make -C oracle`
(oracle/_ref/engine).  The plugin's own source is compiled where it lies, as a loadable flb-filter_record_modifier.so in a scratch
directory outside the repository (the engine of oracle/build_engine.sh is a minimal build without it), with the include paths and
flags fluent-bit_amd/plugin/build.sh uses for the drop-in plugins.  Every case is one chunk through
`engine_host processor -e <.so> <in> <out> --unit record_modifier k=v ...`; the file holds the properties, the input chunk, the output
chunk (base64) and ret.  The processor does not hand the callback's answer on, and it copies what it has through its own group
normalisation (src/flb_processor.c:1811-1852: the records the decoder takes, nothing when there is none), so ret is read from the
bytes: 2 (FLB_FILTER_NOTOUCH, not told from -1) when the input came back byte for byte or nothing came back -- this filter never
answers MODIFIED with an empty buffer (:469-477) and every MODIFIED answer differs from its input --, else 1 (FLB_FILTER_MODIFIED)
with the output.  "refused": the filter did not start.

The runtime test of the reference (tests/runtime/filter_record_modifier.c) is transcribed first: its configurations with the record
each one pushes.  json_long's body is cut to 20 entries (the original's input alone is larger than this file may be; wide maps are
covered on the device against the model); uuid_key is listed as refused here and not recorded (its value is random)."""
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
import synth  # noqa: E402

R = synth.Raw


def rec(body, sec=0, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def kv(*items):
    return synth.KV(list(items))


BIN_K = R(b"\xc4\x01k")
ABC3 = [("aaa", "ok"), ("ccc", "removed"), ("bbb", "ok")]


def cases():
    c = []

    def add(name, props, data, **kw):
        c.append(dict(name=name, props=[list(p) for p in props], data=data, **kw))
    # ---- tests/runtime/filter_record_modifier.c
    add("rt_json_long", [], rec(kv(*[("key_%d" % i, "val_%d" % i) for i in range(20)]), 1448403340))
    add("rt_remove_keys", [("remove_key", "ccc"), ("remove_key", "ddd")],
        rec(kv(("aaa", "ok"), ("ccc", "removed"), ("ddd", "removed"), ("bbb", "ok"))))
    add("rt_records", [("record", "new_key new_val"), ("record", "add_key add_val")], rec(kv(("k", "sample"))))
    add("rt_allowlist_keys", [("allowlist_key", "aaa"), ("allowlist_key", "bbb")], rec(kv(*ABC3)))
    add("rt_whitelist_keys", [("whitelist_key", "aaa"), ("whitelist_key", "bbb")], rec(kv(*ABC3)))
    add("rt_multiple", [("record", "new_key new_val"), ("allowlist_key", "new_key"), ("allowlist_key", "aaa")],
        rec(kv(("aaa", "ok"), ("ddd", "removed"), ("bbb", "ok"))))
    add("rt_exclusive_setting", [("allowlist_key", "aaa"), ("remove_key", "bbb")], rec(kv(("aaa", 1))))
    add("rt_uuid_key", [("uuid_key", "uuid")], rec(kv(("key_name", "sample"))), refused_here=True)
    # ---- the rest of the pin
    add("case_fold", [("Remove_Key", "CcC"), ("remove_key", "É")],
        rec(kv(("ccc", 1), ("CCC", 2), ("cCc", 3), ("ccd", 4), ("é", 5), ("É", 6))))
    add("prefix", [("remove_key", "ab*")], rec(kv(("a", 1), ("ab", 2), ("abc", 3), ("ABx", 4), ("b", 5), (b"ab\0", 6), ("aB", 7))))
    add("allow_mixed_alias", [("Whitelist_key", "x*"), ("Allowlist_key", "B")], rec(kv(("b", 1), ("xy", 2), ("c", 3), ("X", 4))))
    keys = kv(("k", 1), (BIN_K, 2), (7, 3), (None, 4), (R(b"\xc4\x01K"), 5), ("z", 6), (True, 7))
    add("star_remove", [("remove_key", "*")], rec(keys))
    add("star_allow", [("allowlist_key", "*")], rec(keys))
    add("bin_int_remove", [("remove_key", "k")], rec(keys))
    add("bin_int_allow", [("allowlist_key", "k")], rec(keys))
    add("empty_map_record", [("record", "h v")], rec({}) + rec(kv(("a", 1))))
    add("loses_all_next_to_kept", [("remove_key", "x")], rec(kv(("x", 1)), 1) + rec(kv(("x", 1), ("y", 2)), 2) + rec({}, 3))
    add("all_lose_all", [("remove_key", "x")], rec(kv(("x", 1)), 1) + rec(kv(("X", 1), ("x", 2)), 2) + rec({}, 3))
    add("non_map_body", [("remove_key", "x")],
        rec(kv(("x", 1), ("y", 2)), 1) + synth.mp([[synth.ext_ts(2), {}], "text"]) + rec(kv(("x", 1), ("y", 2)), 3))
    add("non_map_body_first", [("record", "a b")], synth.mp([[synth.ext_ts(2), {}], [1]]) + rec(kv(("y", 2)), 3))
    add("legacy_rows", [("record", "a b")],
        synth.mp([1700000000, kv(("k", 1))]) + synth.mp([1700000000.25, kv(("k", 2))]) + synth.mp([2 ** 33, kv(("k", 3))]) +
        synth.mp([R(b"\xd7\x00" + struct.pack(">II", 5, 6)), kv(("k", 4))]))
    add("metadata", [("remove_key", "x")],
        rec(kv(("x", 1), ("y", 2)), 5, 6, kv(("m", 1), ("z", [1, 2]))) +
        synth.mp([[synth.ext_ts(7, 8), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("x", 1), ("y", 2))]))
    add("non_canonical", [("remove_key", "x")],
        synth.mp([[synth.ext_ts(1), {}], R(b"\xde\x00\x02" + b"\xda\x00\x03abc" + b"\xd1\x01\x00" + b"\xa1x\x01")]) +
        synth.mp([[synth.ext_ts(2), {}], R(b"\xdf\x00\x00\x00\x03\xa1x\x01\xd9\x01q\xdc\x00\x01\xcd\x00\x07\xa1r\xc5\x00\x01b")]))
    add("record_one_token", [("record", "lonely")], rec(kv(("a", 1))))
    add("record_three_tokens", [("record", "a b c d"), ("record", "k v")], rec(kv(("a", 1))))
    add("record_quoted", [("record", 'k "v w"'), ("record", '"a b" c'), ("Record", 'q "x \\" y"')], rec(kv(("a", 1))))
    add("garbage_reserved_byte", [("remove_key", "x")], rec(kv(("x", 1), ("y", 2))) + b"\xc1\xff")
    add("garbage_cut_record", [("record", "a b")], rec(kv(("y", 2))) + rec(kv(("y", "long value")))[:-4])
    add("notouch", [("remove_key", "zzz"), ("remove_key", "yy*")], rec(kv(("a", 1), ("y", 2))) + rec({}) + rec(kv(("zz", 1))))
    add("group_markers", [("record", "a b")],
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), kv(("g", 1))], kv(("r", 1))]) + rec(kv(("k", 1)), 4) +
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xfe\x00\x00\x00\x00"), {}], {}]) + rec(kv(("k", 2)), 5))
    return c


def includes(ref, engine):
    def up2(pattern):
        hits = glob.glob(os.path.join(ref, "lib", "**", pattern), recursive=True)
        return os.path.dirname(os.path.dirname(sorted(hits)[0]))
    inc = [os.path.join(engine, "include"), os.path.join(engine, "include", "monkey")]
    inc += [os.path.join(ref, p) for p in (
        "include", "lib/monkey/include", "lib/monkey/include/monkey", "lib/cfl/include", "lib/cfl/lib/xxhash", "lib/cmetrics/include",
        "lib/ctraces/include", "lib/msgpack-c/include", "lib/flb_libco", "lib/onigmo", "lib/cprofiles/include", "lib/rbtree",
        "lib/chunkio/include", "lib/jsmn", "lib/miniz", "lib/tutf8e/include", "lib/lwrb/lwrb/src/include")]
    inc += [up2("nghttp2.h"), up2("mpack.h")]
    return ["-I" + p for p in inc]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "recmod_ref_cases.json"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    host = os.path.join(engine, "engine_host")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_record_modifier")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(host):
        sys.exit("build the reference engine first: make -C oracle")
    out = []
    with tempfile.TemporaryDirectory(prefix="recmod_golden_") as tmp:
        so = os.path.join(tmp, "flb-filter_record_modifier.so")
        src = os.path.join(a.reference, "plugins", "filter_record_modifier")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function"] + includes(a.reference, engine) +
                       ["-I" + src, "-o", so, os.path.join(src, "filter_modifier.c")], check=True)
        for c in cases():
            e = dict(name=c["name"], props=c["props"], **{"in": base64.b64encode(c["data"]).decode()})
            if c.get("refused_here"):
                e["refused_here"] = True
                out.append(e)
                continue
            fin, fout = os.path.join(tmp, "in.mp"), os.path.join(tmp, "out.mp")
            with open(fin, "wb") as f:
                f.write(c["data"])
            cmd = [host, "processor", "-e", so, fin, fout, "--unit", "record_modifier"] + ["%s=%s" % (k, v) for k, v in c["props"]]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if not lines:
                # a property the config map refuses is reported before the processor starts
                if r.returncode == 3 or b"refused" in r.stderr:
                    e["refused"] = True
                    out.append(e)
                    continue
                sys.exit("%s: engine_host said nothing (exit %d): %s" % (c["name"], r.returncode, r.stderr.decode()[-400:]))
            res = json.loads(lines[-1])
            if not res.get("init", True):
                e["refused"] = True
            else:
                got = open(fout, "rb").read()
                if got == c["data"] or not got:
                    e["ret"], e["out"] = 2, None
                else:
                    e["ret"], e["out"] = 1, base64.b64encode(got).decode()
            out.append(e)
    with open(a.out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d cases, %d bytes -> %s" % (len(out), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()

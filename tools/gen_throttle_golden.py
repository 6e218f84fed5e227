#!/usr/bin/env python3
"""Records the answers of the real filter_throttle_size and filter_throttle for tests/golden/throttle_size_ref_cases.json and
tests/golden/throttle_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of
`make -C oracle engine` (oracle/_ref/engine).  Each plugin's own sources are compiled where they lie as a loadable
flb-filter_<name>.so in a scratch directory outside the repository, linked with --wrap=sleep, --wrap=flb_time_get and --wrap=flb_log_print, next to
tools/throttle_ref_host.c -- this project's own host, which defines the wrappers (the log lines are dropped: the plugin formats a freed window's name into one), creates the filter instance in the reference
engine library and walks a script of steps: `now T` (the clock cb_filter sees), `tick T` (one trip of the plugin's own ticker thread,
at T and at no other time), `chunk <bytes>` (one cb_filter call).  Nothing compiled and no reference text enters the repository, only
the fixtures: per case the properties and the steps, every chunk step with cb_filter's return value and, when it is
FLB_FILTER_MODIFIED, the output -- or "refused": the filter did not start.  The cases are tests/throttle_chunks.py's: the runtime
tests of the reference (tests/runtime/filter_throttle_size.c, filter_throttle.c) transcribed first.  The two cases of
throttle_chunks.DEVIATES are marked "deviates": the product does not reproduce them."""
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
from gen_recmod_golden import includes  # noqa: E402
import throttle_chunks as tc  # noqa: E402

PLUGINS = {"throttle_size": ("filter_throttle_size", ["throttle_size.c", "size_window.c"]), "throttle": ("filter_throttle", ["throttle.c", "window.c"])}


def build_reference(reference, engine, tmp):
    """compiles both plugins and tools/throttle_ref_host.c into tmp: (host, {kind: plugin})"""
    inc = includes(reference, engine)
    host = os.path.join(tmp, "throttle_ref_host")
    sos = {}
    for kind, (d, files) in PLUGINS.items():
        src = os.path.join(reference, "plugins", d)
        sos[kind] = os.path.join(tmp, "flb-%s.so" % d)
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-format", "-Wno-format-extra-args", "-D__FLB_FILENAME__=__FILE__"] + inc +
                       ["-I" + os.path.join(reference, "lib"), "-I" + src, "-Wl,--wrap=sleep", "-Wl,--wrap=flb_time_get", "-Wl,--wrap=flb_log_print", "-o", sos[kind]] +
                       [os.path.join(src, f) for f in files], check=True)
    subprocess.run(["gcc", "-O2", "-Wall", "-rdynamic"] + inc + ["-o", host, os.path.join(ROOT, "tools", "throttle_ref_host.c"),
                    "-L" + os.path.join(engine, "lib"), "-lfluent-bit", "-Wl,-rpath," + os.path.join(engine, "lib"), "-lpthread", "-ldl", "-lm"], check=True)
    return host, sos


def run_case(host, so, kind, props, steps, tmp, extra=(), name=""):
    """the host over one script: (init, [(ret, out bytes | None)] per chunk step, the other JSON lines)"""
    script = os.path.join(tmp, "script.txt")
    with open(script, "w") as f:
        for st in steps:
            f.write("chunk " + bytes(st[1]).hex() + "\n" if st[0] == "chunk" else "%s %d\n" % (st[0], st[1]))
    cmd = [host, so, kind, script] + list(extra) + ["%s=%s" % (k, v) for k, v in props]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    lines = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.exit("%s: throttle_ref_host failed (%d): %s" % (name, r.returncode, r.stderr.decode(errors="replace")[-800:]))
    res = [(ln["ret"], bytes.fromhex(ln["out"]) if ln["ret"] == 1 else None) for ln in lines if "ret" in ln]
    return lines[0]["init"], res, [ln for ln in lines[1:] if "ret" not in ln]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_throttle_size")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(os.path.join(engine, "lib", "libfluent-bit.so")):
        sys.exit("build the reference engine first: make -C oracle engine")
    with tempfile.TemporaryDirectory(prefix="throttle_golden_") as tmp:
        host, sos = build_reference(a.reference, engine, tmp)
        for kind, cases in (("throttle_size", tc.size_cases()), ("throttle", tc.throttle_cases())):
            out = []
            for name, props, steps in cases:
                e = dict(name=name, props=[list(p) for p in props])
                if name in tc.DEVIATES:
                    e["deviates"] = True
                init, res, _ = run_case(host, sos[kind], kind, props, steps, tmp, name=name)
                if not init:
                    e["refused"] = True
                else:
                    if len(res) != sum(1 for s in steps if s[0] == "chunk"):
                        sys.exit("%s: %d answers for its chunk steps" % (name, len(res)))
                    it = iter(res)
                    e["steps"] = []
                    for st in steps:
                        if st[0] != "chunk":
                            e["steps"].append([st[0], st[1]])
                            continue
                        ret, ob = next(it)
                        e["steps"].append(["chunk", base64.b64encode(st[1]).decode(), ret, base64.b64encode(ob).decode() if ob is not None else None])
                out.append(e)
            path = os.path.join(a.out_dir, "%s_ref_cases.json" % kind)
            with open(path, "w") as f:
                f.write('{"recorded_from": "whole plugin", "cases": [\n' + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
            print("%s: %d cases (%d refused), %d bytes -> %s" % (kind, len(out), sum(1 for e in out if e.get("refused")), os.path.getsize(path), path))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""filter_type_converter on 10 M apache-shaped parsed records resident in HBM, next to filter_record_modifier on the same chunk.

  T1  str_key status status_i int + str_key latency latency_f float   (the filter that most often sits behind filter_parser)
  R1  filter_record_modifier: Record hostname h                       (the yardstick: the same copy-everything traffic)

The chunk is the one of tools/perf_recmod.py -- the same value generators -- with `code` named `status` and a `latency` string
("0.123") in the place of `referer`.  Per program: ms per call from the library's own device timing (event pairs around every launch
of the call: the size pass, the scan, the emit pass -- flbgpu_filter_profile), the wall time of the call next to it, records per
second and input plus output bytes per second of the kernel time as a fraction of the 8 TB/s roof.  The two filters alternate call
by call on the same chunk; the spread is the range over the repeated calls.  Needs a GPU: there is no CPU path.  Where --ref-plugin
names a flb-filter_type_converter.so built against oracle/_ref/engine (tools/gen_typeconv_golden.py shows the compile line), one
block of the chunk also goes through `engine_host processor` and its wall time is recorded as the reference's CPU time per record.
Usage: perf_typeconv.py [--records N] [--repeats K] [--ref-plugin SO] [--out profiles/typeconv_perf.json]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flbamd_loader  # noqa: E402
import synth  # noqa: E402
from perf_recmod import AGENTS, BLOCK, ROOF, kernel_ms  # noqa: E402

T1 = [("str_key", "status status_i int"), ("str_key", "latency latency_f float")]
R1 = [("Record", "hostname h")]


def block(seed):
    r = random.Random(seed)
    out = []
    for i in range(BLOCK):
        out.append(synth.mp([[synth.ext_ts(1700000000 + i, r.randrange(10 ** 9)), {}], synth.KV([
            (b"host", "%d.%d.%d.%d" % (r.randrange(256), r.randrange(256), r.randrange(256), r.randrange(256))), (b"user", "-"),
            (b"time", "10/Oct/2023:13:55:%02d +0000" % (i % 60)), (b"method", r.choice(["GET", "POST", "PUT"])),
            (b"path", "/api/v1/items/%d?page=%d" % (r.randrange(100000), r.randrange(50))), (b"status", r.choice(["200", "404", "500", "503"])),
            (b"size", str(r.randrange(100000))), (b"latency", "%d.%03d" % (r.randrange(3), r.randrange(1000))), (b"agent", r.choice(AGENTS))])]))
    return b"".join(out)


def reference_cpu(so, blk):
    """seconds per record of the real plugin on one block, through the reference's processor; None when it cannot run here"""
    host = os.path.join(ROOT, "oracle", "_ref", "engine", "engine_host")
    if not so or not os.path.exists(so) or not os.path.exists(host):
        return None
    with tempfile.TemporaryDirectory(prefix="typeconv_perf_") as tmp:
        fin, fout = os.path.join(tmp, "in.mp"), os.path.join(tmp, "out.mp")
        with open(fin, "wb") as f:
            f.write(blk)
        cmd = [host, "processor", "-e", so, fin, fout, "--unit", "type_converter"] + ["%s=%s" % kv for kv in T1]
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            if subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
                return None
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    return best / BLOCK


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ref-plugin", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "typeconv_perf.json"))
    a = ap.parse_args()
    g = flbamd_loader.load()
    g.init(0)
    L = g.lib()
    blk = block(1)
    reps = max(1, a.records // BLOCK)
    nbytes = len(blk) * reps
    d = L.flbgpu_dev_alloc(nbytes + 16)
    if not d:
        sys.exit(g.last_error())
    for i in range(reps):
        if L.flbgpu_memcpy_h2d(ctypes.c_void_p(d + i * len(blk)), blk, len(blk)) != 0:
            sys.exit("upload failed")
    ix = g.Indexer()
    chunk, consumed = ix.index_dev(d, nbytes)
    assert consumed == nbytes and chunk.n == reps * BLOCK
    fs = {"T1": g.FilterTypeConverter(T1), "R1": g.FilterRecordModifier(R1)}
    stat = {k: dict(kernel_ms=[], wall_ms=[]) for k in fs}
    seen, outs = {k: {} for k in fs}, {}
    for f in fs.values():
        f.profile(True)
    for it in range(a.repeats + 2):                          # two warm-up calls of each filter, then the two alternate
        for k, f in fs.items():
            t0 = time.perf_counter()
            ret, out = f.filter_dev(chunk)
            wall = (time.perf_counter() - t0) * 1e3
            ms, seen[k] = kernel_ms(f, seen[k])
            assert ret == g.MODIFIED, (k, ret, g.last_error())
            if it >= 2:
                stat[k]["kernel_ms"].append(ms)
                stat[k]["wall_ms"].append(wall)
            outs[k] = int(out.bytes)
    res = dict(records=int(chunk.n), in_bytes=nbytes, roof_bytes_per_s=ROOF, repeats=a.repeats, programs=dict(T1=T1, R1=R1), configs={})
    for k, s in stat.items():
        med = statistics.median(s["kernel_ms"])
        res["configs"][k] = dict(filter="record_modifier" if k == "R1" else "type_converter", out_bytes=outs[k], kernel_ms_median=med,
                                 kernel_ms_min=min(s["kernel_ms"]), kernel_ms_max=max(s["kernel_ms"]),
                                 wall_ms_median=statistics.median(s["wall_ms"]), kernel_ms_all=s["kernel_ms"],
                                 records_per_s=int(chunk.n) / (med * 1e-3), gb_per_s=(nbytes + outs[k]) / (med * 1e-3) / 1e9,
                                 roof_fraction=(nbytes + outs[k]) / (med * 1e-3) / ROOF,
                                 per_kernel={kn: v[0] / (a.repeats + 2) for kn, v in seen[k].items()})
    c = fs["T1"].counters()
    res["configs"]["T1"]["counters_per_call"] = [x // (a.repeats + 2) for x in c]
    assert c[3] == 0
    res["configs"]["T1"]["over_recmod_R1"] = res["configs"]["T1"]["kernel_ms_median"] / res["configs"]["R1"]["kernel_ms_median"]
    ref = reference_cpu(a.ref_plugin, blk)
    res["reference_cpu_s_per_record"] = ref
    for k, f in fs.items():
        c = res["configs"][k]
        print("%-3s kernel ms median %.3f (min %.3f max %.3f)  wall %.3f  %.1f M records/s  %.1f GB/s  %.1f%% of roof  %s" %
              (k, c["kernel_ms_median"], c["kernel_ms_min"], c["kernel_ms_max"], c["wall_ms_median"], c["records_per_s"] / 1e6, c["gb_per_s"],
               100 * c["roof_fraction"], "" if k == "R1" else "x%.2f of R1" % c["over_recmod_R1"]))
        print("    per kernel ms:", {kn: round(v, 3) for kn, v in c["per_kernel"].items()})
        f.close()
    print("reference plugin: %s" % ("not measured" if ref is None else "%.0f ns per record on one CPU core" % (ref * 1e9)))
    L.flbgpu_dev_free(d)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

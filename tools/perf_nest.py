#!/usr/bin/env python3
"""filter_nest on 10 M apache-shaped parsed records resident in HBM, next to filter_record_modifier's R1 on the same chunk.

  N1  nest 3 of the 8 scalar keys (Wildcard host, Wildcard req_*) under `request`
  L1  lift the 6-entry map under `kubernetes` with Add_prefix k8s_
  R1  filter_record_modifier: Record hostname h + Remove_key agent        (the yardstick, tools/perf_recmod.py)

The chunk is the one of tools/perf_recmod.py -- nine entries a record, the same value generators -- with `method` and `path` named
`req_method` and `req_path` (so that one prefix wildcard takes two keys) and the `referer` string replaced by a six-entry
`kubernetes` map (so that there is something to lift).  Per program: ms per call from the library's own device timing (event pairs
around every launch of the call: the size pass, the scan, the emit pass -- flbgpu_filter_profile), the wall time of the call next to
it, input plus output bytes per second of the kernel time as a fraction of the 8 TB/s roof.  The three filters alternate call by call
on the same chunk; the spread is the range over the repeated calls.  Needs a GPU: there is no CPU path.
Usage: perf_nest.py [--records N] [--repeats K] [--out profiles/nest_perf.json]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flbamd_loader  # noqa: E402
import synth  # noqa: E402
from perf_recmod import AGENTS, BLOCK, ROOF, kernel_ms  # noqa: E402

N1 = [("Operation", "nest"), ("Wildcard", "host"), ("Wildcard", "req_*"), ("Nest_under", "request")]
L1 = [("Operation", "lift"), ("Nested_under", "kubernetes"), ("Add_prefix", "k8s_")]
R1 = [("Record", "hostname h"), ("Remove_key", "agent")]


def block(seed):
    r = random.Random(seed)
    out = []
    for i in range(BLOCK):
        k8s = synth.KV([(b"pod_name", "web-%d" % r.randrange(5000)), (b"namespace_name", r.choice(["default", "prod", "staging"])),
                        (b"container_name", "nginx"), (b"host", "node-%d" % r.randrange(200)),
                        (b"pod_id", "%032x" % r.getrandbits(128)), (b"container_image", "nginx:1.25.%d" % r.randrange(5))])
        out.append(synth.mp([[synth.ext_ts(1700000000 + i, r.randrange(10 ** 9)), {}], synth.KV([
            (b"host", "%d.%d.%d.%d" % (r.randrange(256), r.randrange(256), r.randrange(256), r.randrange(256))), (b"user", "-"),
            (b"time", "10/Oct/2023:13:55:%02d +0000" % (i % 60)), (b"req_method", r.choice(["GET", "POST", "PUT"])),
            (b"req_path", "/api/v1/items/%d?page=%d" % (r.randrange(100000), r.randrange(50))), (b"code", r.choice(["200", "404", "500", "503"])),
            (b"size", str(r.randrange(100000))), (b"kubernetes", k8s), (b"agent", r.choice(AGENTS))])]))
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nest_perf.json"))
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
    fs = {"N1": g.FilterNest(N1), "L1": g.FilterNest(L1), "R1": g.FilterRecordModifier(R1)}
    stat = {k: dict(kernel_ms=[], wall_ms=[]) for k in fs}
    seen, outs = {k: {} for k in fs}, {}
    for f in fs.values():
        f.profile(True)
    for it in range(a.repeats + 2):                          # two warm-up calls of each filter, then the three alternate
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
    res = dict(records=int(chunk.n), in_bytes=nbytes, roof_bytes_per_s=ROOF, repeats=a.repeats, programs=dict(N1=N1, L1=L1, R1=R1), configs={})
    for k, s in stat.items():
        med = statistics.median(s["kernel_ms"])
        res["configs"][k] = dict(filter="record_modifier" if k == "R1" else "nest", out_bytes=outs[k], kernel_ms_median=med,
                                 kernel_ms_min=min(s["kernel_ms"]), kernel_ms_max=max(s["kernel_ms"]),
                                 wall_ms_median=statistics.median(s["wall_ms"]), kernel_ms_all=s["kernel_ms"],
                                 bytes_per_s=(nbytes + outs[k]) / (med * 1e-3), roof_fraction=(nbytes + outs[k]) / (med * 1e-3) / ROOF,
                                 per_kernel={kn: v[0] / (a.repeats + 2) for kn, v in seen[k].items()})
    for k in ("N1", "L1"):
        res["configs"][k]["built"] = fs[k].counters()[0] // (a.repeats + 2)
        res["configs"][k]["over_recmod_R1"] = res["configs"][k]["kernel_ms_median"] / res["configs"]["R1"]["kernel_ms_median"]
    for k, f in fs.items():
        c = res["configs"][k]
        print("%-3s kernel ms median %.3f (min %.3f max %.3f)  wall %.3f  %.1f%% of roof  %s" %
              (k, c["kernel_ms_median"], c["kernel_ms_min"], c["kernel_ms_max"], c["wall_ms_median"], 100 * c["roof_fraction"],
               "" if k == "R1" else "x%.2f of R1" % c["over_recmod_R1"]))
        f.close()
    L.flbgpu_dev_free(d)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

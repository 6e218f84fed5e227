#!/usr/bin/env python3
"""filter_record_modifier on 10 M apache-shaped parsed records resident in HBM, next to filter_modify with the equivalent program.

  R1  Record hostname h + Remove_key agent        yardstick: FilterModify  Remove agent + Add hostname h
  R2  Allowlist_key host / code / size            yardstick: FilterModify  Remove of the six other keys

Per configuration and filter: ms per call from the library's own device timing (event pairs around every launch of the call: the
size pass, the scan, the emit pass -- flbgpu_filter_profile), the wall time of the call next to it, input plus output bytes per second
of the kernel time as a fraction of the 8 TB/s roof.  The two filters alternate call by call on the same chunk; the spread is the
range over the repeated calls.  The two outputs are compared by length (the same entries; record_modifier's map32 header is four
bytes more per record).  Needs a GPU: there is no CPU path.  Usage: perf_recmod.py [--records N] [--repeats K] [--out profiles/recmod_perf.json]"""
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

ROOF = 8.0e12
BLOCK = 100000
CONFIGS = {
    "R1": ([("Record", "hostname h"), ("Remove_key", "agent")], [("Remove", "agent"), ("Add", "hostname h")]),
    "R2": ([("Allowlist_key", "host"), ("Allowlist_key", "code"), ("Allowlist_key", "size")],
           [("Remove", k) for k in ("user", "method", "path", "referer", "agent", "time")]),
}
AGENTS = ["Mozilla/5.0 (X11; Linux x86_64) AppleWebKit/537.36 (KHTML, like Gecko) Chrome/120.0 Safari/537.36", "curl/8.4.0",
          "Mozilla/5.0 (Macintosh; Intel Mac OS X 10_15_7) AppleWebKit/605.1.15 (KHTML, like Gecko) Version/17.1 Safari/605.1.15"]


def block(seed):
    r = random.Random(seed)
    out = []
    for i in range(BLOCK):
        out.append(synth.mp([[synth.ext_ts(1700000000 + i, r.randrange(10 ** 9)), {}], synth.KV([
            (b"host", "%d.%d.%d.%d" % (r.randrange(256), r.randrange(256), r.randrange(256), r.randrange(256))), (b"user", "-"),
            (b"time", "10/Oct/2023:13:55:%02d +0000" % (i % 60)), (b"method", r.choice(["GET", "POST", "PUT"])),
            (b"path", "/api/v1/items/%d?page=%d" % (r.randrange(100000), r.randrange(50))), (b"code", r.choice(["200", "404", "500", "503"])),
            (b"size", str(r.randrange(100000))), (b"referer", "https://example.com/list/%d" % r.randrange(1000)), (b"agent", r.choice(AGENTS))])]))
    return b"".join(out)


def kernel_ms(f, before):
    now = f.profile_read()
    return sum(ms - before.get(k, (0.0, 0))[0] for k, (ms, _) in now.items()), now


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recmod_perf.json"))
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
    res = dict(records=int(chunk.n), in_bytes=nbytes, roof_bytes_per_s=ROOF, repeats=a.repeats, configs={})
    for name, (rprops, mprops) in CONFIGS.items():
        fs = {"record_modifier": g.FilterRecordModifier(rprops), "modify": g.FilterModify(mprops)}
        stat = {k: dict(kernel_ms=[], wall_ms=[]) for k in fs}
        seen, outs = {k: {} for k in fs}, {}
        for f in fs.values():
            f.profile(True)
        for it in range(a.repeats + 2):                      # two warm-up calls of each filter, then the two alternate
            for k, f in fs.items():
                t0 = time.perf_counter()
                ret, out = f.filter_dev(chunk)
                wall = (time.perf_counter() - t0) * 1e3
                ms, seen[k] = kernel_ms(f, seen[k])
                assert ret == g.MODIFIED, (name, k, ret, g.last_error())
                if it >= 2:
                    stat[k]["kernel_ms"].append(ms)
                    stat[k]["wall_ms"].append(wall)
                outs[k] = (int(out.bytes),)
        # the two outputs hold the same entries; they differ in the body's map header alone (filter_modify packs the smallest one,
        # record_modifier's encoder always writes map32: four bytes more per record)
        same = outs["record_modifier"][0] == outs["modify"][0] + 4 * int(chunk.n)
        cfg = dict(out_bytes=outs["record_modifier"][0], modify_out_bytes=outs["modify"][0], same_entries_as_modify=same,
                   kernels=sorted(seen["record_modifier"]))
        for k, s in stat.items():
            med = statistics.median(s["kernel_ms"])
            cfg[k] = dict(kernel_ms_median=med, kernel_ms_min=min(s["kernel_ms"]), kernel_ms_max=max(s["kernel_ms"]),
                          wall_ms_median=statistics.median(s["wall_ms"]), kernel_ms_all=s["kernel_ms"],
                          bytes_per_s=(nbytes + outs[k][0]) / (med * 1e-3), roof_fraction=(nbytes + outs[k][0]) / (med * 1e-3) / ROOF,
                          per_kernel={kn: v[0] / (a.repeats + 2) for kn, v in seen[k].items()})
        cfg["record_modifier_over_modify"] = cfg["record_modifier"]["kernel_ms_median"] / cfg["modify"]["kernel_ms_median"]
        res["configs"][name] = cfg
        for f in fs.values():
            f.close()
        print(name, json.dumps({k: cfg[k] for k in ("out_bytes", "same_entries_as_modify", "record_modifier_over_modify")}))
        for k in fs:
            print("  %-16s kernel ms median %.3f (min %.3f max %.3f)  wall %.3f  %.1f%% of roof" %
                  (k, cfg[k]["kernel_ms_median"], cfg[k]["kernel_ms_min"], cfg[k]["kernel_ms_max"], cfg[k]["wall_ms_median"],
                   100 * cfg[k]["roof_fraction"]))
    L.flbgpu_dev_free(d)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

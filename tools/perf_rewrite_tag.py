#!/usr/bin/env python3
"""filter_rewrite_tag on a 10 M-record chunk of the bench's apache-style records resident in HBM, next to filter_grep with the same
regex on the same chunk -- the yardstick: the same key lookup, the same automaton and the same copy of the kept records, minus tags.

  W1  Rule $log ^.*error.*$ err.$TAG false           G1  Regex log ^.*error.*$
  W2  Rule $log ^.*(error).*$ err.$1 false           (the same with a capturing pattern: the capture walk on the matched rows)
  W3  Rule $log "\\" (5\\d\\d) " s.$1.$TAG[0] false    G3  Regex log " (5\\d\\d)     (a pattern some of the generator's lines do match)

The bench's generator writes no line with "error" in it, so W1 / W2 / G1 time the pass that matches nothing (the filter answers
NOTOUCH, filter_grep an empty chunk); W3 / G3 time a call that emits.  Per configuration: ms per call from the library's own device
timing (event pairs around every launch of the call -- flbgpu_filter_profile), the wall time of the call next to it, records per
second, what each kernel took, the emissions of a call and the ratio to the grep configuration next to it.  The filters alternate
call by call on the same chunk; the spread is the range over the repeated calls.  Needs a GPU: there is no CPU path.
Usage: perf_rewrite_tag.py [--records N] [--repeats K] [--out profiles/rewrite_tag_perf.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flbamd_loader  # noqa: E402
import synth  # noqa: E402
from perf_recmod import BLOCK, ROOF, kernel_ms  # noqa: E402

RULES = {"W1": "$log ^.*error.*$ err.$TAG false", "W2": "$log ^.*(error).*$ err.$1 false", "W3": '$log " (5\\d\\d) " s.$1.$TAG[0] false'}
GREPS = {"G1": "log ^.*error.*$", "G3": 'log  (5\\d\\d) '}
YARDSTICK = {"W1": "G1", "W2": "G1", "W3": "G3"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rewrite_tag_perf.json"))
    a = ap.parse_args()
    g = flbamd_loader.load()
    g.init(0)
    L = g.lib()
    data, off, ep = synth.apache_records(BLOCK)
    blk = bytes(data)
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
    fs = {k: g.FilterRewriteTag([("Rule", v)], b"apache.access") for k, v in RULES.items()}
    fs.update({k: g.FilterGrep([("regex", v)]) for k, v in GREPS.items()})
    stat = {k: dict(kernel_ms=[], wall_ms=[]) for k in fs}
    seen, outs, rets = {k: {} for k in fs}, {}, {}
    for f in fs.values():
        f.profile(True)
    for it in range(a.repeats + 2):                          # two warm-up calls of each filter, then they alternate
        for k, f in fs.items():
            t0 = time.perf_counter()
            ret, out = f.filter_dev(chunk)
            wall = (time.perf_counter() - t0) * 1e3
            ms, seen[k] = kernel_ms(f, seen[k])
            if it >= 2:
                stat[k]["kernel_ms"].append(ms)
                stat[k]["wall_ms"].append(wall)
            outs[k], rets[k] = (int(out.bytes) if ret == g.MODIFIED else None), ret
    res = dict(records=int(chunk.n), in_bytes=nbytes, roof_bytes_per_s=ROOF, repeats=a.repeats, rules=RULES, greps=GREPS, configs={})
    for k, s in stat.items():
        med = statistics.median(s["kernel_ms"])
        res["configs"][k] = dict(ret=rets[k], out_bytes=outs[k], kernel_ms_median=med, kernel_ms_min=min(s["kernel_ms"]), kernel_ms_max=max(s["kernel_ms"]),
                                 wall_ms_median=statistics.median(s["wall_ms"]), kernel_ms_all=s["kernel_ms"], records_per_s=int(chunk.n) / (med * 1e-3),
                                 in_gb_per_s=nbytes / (med * 1e-3) / 1e9, per_kernel={kn: v[0] / (a.repeats + 2) for kn, v in seen[k].items()})
    for k, y in YARDSTICK.items():
        c = res["configs"][k]
        cnt = fs[k].counters()
        assert cnt[2] == 0
        c["emitted_per_call"], c["tag_bytes_per_call"] = cnt[0] // (a.repeats + 2), cnt[3] // (a.repeats + 2)
        c["over_grep"] = c["kernel_ms_median"] / res["configs"][y]["kernel_ms_median"]
    for k, f in fs.items():
        c = res["configs"][k]
        print("%-3s ret %d  kernel ms median %.3f (min %.3f max %.3f)  wall %.3f  %.1f M records/s  %.1f GB/s read  %s" %
              (k, c["ret"], c["kernel_ms_median"], c["kernel_ms_min"], c["kernel_ms_max"], c["wall_ms_median"], c["records_per_s"] / 1e6, c["in_gb_per_s"],
               "" if k not in YARDSTICK else "x%.2f of %s, %d emitted" % (c["over_grep"], YARDSTICK[k], c["emitted_per_call"])))
        print("    per kernel ms:", {kn: round(v, 3) for kn, v in c["per_kernel"].items()})
        f.close()
    L.flbgpu_dev_free(d)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""filter_expect on 4 M apache-shaped parsed records resident in HBM, next to filter_record_modifier on the same chunk.

  K1   action result_key, one key_exists rule        K4   action result_key, four key_exists rules
  W4   action warn, the same four rules (no emit: the call answers NOTOUCH)
  F4   action result_key, four rules of which every record fails the last (the failure table holds every record)
  R    filter_record_modifier adding `matched true` (the yardstick of DESIGN 4j: the existing filter that does the same writer work)

The chunk is the one of tools/perf_checklist.py.  Per configuration: ms per call from the library's own device timing (event pairs
around every launch of the call -- flbgpu_filter_profile), the median of the repeated calls after two warm-up calls, with the range
as the spread; the wall time next to it, records per second, and the ratio over R measured in the same run, the calls in turn.
Needs a GPU: there is no CPU path.
--cpu-reference (no GPU; a development machine with a fluent-bit source tree and `make -C oracle engine`): the real plugin's cb_filter
on a 2 MB chunk of the same records, through tools/expect_ref_host.c, the fastest of five calls; written into the same file under
"reference_cpu", marked as a CPU number of the machine it ran on.
Usage: perf_expect.py [--records N] [--repeats K] [--configs K4,W4] [--out profiles/expect_perf.json] [--cpu-reference --reference TREE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402
from perf_recmod import BLOCK, ROOF, kernel_ms  # noqa: E402
from perf_checklist import block  # noqa: E402

FOUR = [("key_exists", k) for k in ("$host", "$status", "$size", "$agent")]
CONFIGS = {
    "K1": [("action", "result_key"), ("key_exists", "$host")],
    "K4": [("action", "result_key")] + FOUR,
    "W4": [("action", "warn")] + FOUR,
    "F4": [("action", "result_key")] + FOUR[:3] + [("key_val_is_null", "$nothing")],
}
CHECKLIST_EXACT_OVER_R = 1.29       # filter_checklist, mode exact, over the same yardstick


def cpu_reference(a):
    import subprocess
    from gen_expect_golden import build_reference
    import modify_model as mm
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    blk, _ = block(1)
    p = 0
    while p < 2 * 1024 * 1024:                               # whole records up to 2 MB
        p = mm.decode_event(blk, p)[0]
    chunk = blk[:p]
    nrec = len(synth.unpack_all(chunk))
    res = dict(machine="CPU, one core of the development machine (not the GPU host)", chunk_bytes=len(chunk), records=nrec, configs={})
    with tempfile.TemporaryDirectory(prefix="expect_perf_") as tmp:
        host, so = build_reference(a.reference, engine, tmp)
        fin, fout = os.path.join(tmp, "in.mp"), os.path.join(tmp, "out.mp")
        with open(fin, "wb") as f:
            f.write(chunk)
        for k in ("K1", "K4", "W4"):
            r = subprocess.run([host, so, fin, fout, "--repeat", "5"] + ["%s=%s" % kv for kv in CONFIGS[k]], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                               check=True)
            ans = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
            assert ans["init"] and ans["ret"] == (2 if k == "W4" else 1), ans
            ns = ans["filter_ns"]
            res["configs"][k] = dict(filter_ms=ns / 1e6, ns_per_record=ns / nrec, ms_per_2MB_chunk=ns / 1e6 * 2097152 / len(chunk), ms_per_4M_records=ns / nrec * 4e6 / 1e6)
            print("%-3s reference plugin: %.3f ms for %d records (%d bytes), %.0f ns a record" % (k, ns / 1e6, nrec, len(chunk), ns / nrec))
    cur = json.load(open(a.out)) if os.path.exists(a.out) else {}
    cur["reference_cpu"] = res
    with open(a.out, "w") as f:
        json.dump(cur, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4000000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expect_perf.json"))
    ap.add_argument("--configs", default=None, help="comma-separated subset of K1,K4,W4,F4 (R always runs)")
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree (--cpu-reference)")
    a = ap.parse_args()
    if a.cpu_reference:
        return cpu_reference(a)
    import flbamd_loader
    g = flbamd_loader.load()
    g.init(0)
    L = g.lib()
    blk, _ = block(1)
    reps = max(1, a.records // BLOCK)
    nbytes = len(blk) * reps
    d = L.flbgpu_dev_alloc(nbytes + 16)
    if not d:
        sys.exit(g.last_error())
    for i in range(reps):
        if L.flbgpu_memcpy_h2d(ctypes.c_void_p(d + i * len(blk)), blk, len(blk)) != 0:
            sys.exit("upload failed")
    ix = g.Indexer()                                         # (it owns the chunk's offset column: it has to outlive the calls)
    chunk, consumed = ix.index_dev(d, nbytes)
    assert consumed == nbytes and chunk.n == reps * BLOCK
    fs = {k: g.FilterExpect(p) for k, p in CONFIGS.items() if a.configs is None or k in a.configs.split(",")}
    fs["R"] = g.FilterRecordModifier([("Record", "matched true")])
    stat = {k: dict(kernel_ms=[], wall_ms=[]) for k in fs}
    seen, outs = {k: {} for k in fs}, {}
    for f in fs.values():
        f.profile(True)
    for it in range(a.repeats + 2):                          # two warm-up calls of each filter, then they run in turn
        for k, f in fs.items():
            t0 = time.perf_counter()
            ret, out = f.filter_dev(chunk)
            wall = (time.perf_counter() - t0) * 1e3
            ms, seen[k] = kernel_ms(f, seen[k])
            assert ret == (g.NOTOUCH if k == "W4" else g.MODIFIED), (k, ret, g.last_error())
            if it >= 2:
                stat[k]["kernel_ms"].append(ms)
                stat[k]["wall_ms"].append(wall)
            outs[k] = int(out.bytes) if ret == g.MODIFIED else 0
    res = dict(records=int(chunk.n), in_bytes=nbytes, roof_bytes_per_s=ROOF, repeats=a.repeats, checklist_exact_over_record_modifier=CHECKLIST_EXACT_OVER_R, configs={})
    for k, s in stat.items():
        med = statistics.median(s["kernel_ms"])
        res["configs"][k] = dict(filter="record_modifier" if k == "R" else "expect", props=CONFIGS.get(k), out_bytes=outs[k], kernel_ms_median=med,
                                 kernel_ms_min=min(s["kernel_ms"]), kernel_ms_max=max(s["kernel_ms"]), wall_ms_median=statistics.median(s["wall_ms"]),
                                 kernel_ms_all=s["kernel_ms"], records_per_s=int(chunk.n) / (med * 1e-3),
                                 per_kernel={kn: v[0] / (a.repeats + 2) for kn, v in seen[k].items()})
    r = res["configs"]["R"]
    for k, f in fs.items():
        c = res["configs"][k]
        if k != "R":
            cn = f.counters()
            calls = a.repeats + 2
            assert cn[3] == 0 and cn[0] == calls * int(chunk.n) and cn[1] == (calls * int(chunk.n) if k == "F4" else 0), (k, cn)
            c["failed_per_call"] = cn[1] // calls
            c["record_modifier_kernel_ms_median"] = r["kernel_ms_median"]
            c["over_record_modifier"] = c["kernel_ms_median"] / r["kernel_ms_median"]
            # the run's own spread: the widest and the narrowest ratio the repeated calls allow
            c["over_record_modifier_range"] = [c["kernel_ms_min"] / r["kernel_ms_max"], c["kernel_ms_max"] / r["kernel_ms_min"]]
        print("%-3s kernel ms median %.3f (min %.3f max %.3f)  wall %.3f  %.1f M records/s  %s" %
              (k, c["kernel_ms_median"], c["kernel_ms_min"], c["kernel_ms_max"], c["wall_ms_median"], c["records_per_s"] / 1e6,
               "" if k == "R" else "x%.2f of R (%.2f .. %.2f)" % (c["over_record_modifier"], *c["over_record_modifier_range"])))
        print("      per kernel ms:", {kn: round(v, 3) for kn, v in c["per_kernel"].items()})
        f.close()
    del ix
    L.flbgpu_dev_free(d)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out) and "reference_cpu" in json.load(open(a.out)):
        res["reference_cpu"] = json.load(open(a.out))["reference_cpu"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

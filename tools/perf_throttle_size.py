#!/usr/bin/env python3
"""filter_throttle_size on a chunk of records of about 250 bytes resident in HBM (default 4 M records).

Three name distributions -- `one` (one name for all rows: the skewed case the wave path of k_tsz_admit exists for), `k1000` (1000 names
evenly), `each` (a name per row) -- each with a rate that keeps almost everything (`keep`) and one that drops almost everything
(`drop`).  Per configuration a fresh filter per call (so that every call meets the same empty state): ms per call from the library's
own device timing (event pairs around every launch of the call -- flbgpu_filter_profile), the median of the repeated calls after one
warm-up call, the wall time next to it, the per-kernel times of the median call's filter and the share of the call spent in
k_tsz_admit (its two launches, <lane> and <wave>; k_tsz_keys and the sort are timed apart).  The switch FLBGPU_TSZ_WAVE_MIN is read when a filter is created: with --wave-min-compare the
skewed configurations run again in a child each under FLBGPU_TSZ_WAVE_MIN=100000 (the tests' setting: a segment of more rows than
that still takes a wave, so at 4 M rows this shows only the cost of telling the segment's length) and =2147483647 (every segment on one
lane), and the ratios are written down, whichever way they fall.  Needs a GPU: there is no CPU path.
--cpu-reference (no GPU; a development machine with a fluent-bit source tree and `make -C oracle engine`): the real plugin's cb_filter on
20 000 of the same records, through tools/throttle_ref_host.c, the fastest of five calls; written into the same file under
"reference_cpu", marked as a CPU number of the machine it ran on.
Usage: perf_throttle_size.py [--records N] [--repeats K] [--wave-min-compare] [--out profiles/throttle_size_perf.json] [--cpu-reference --reference TREE]"""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LOG = b"x" * 200
PROPS = [("window", "5"), ("name_field", "n"), ("log_field", "log")]
RATES = {"keep": "1G", "drop": "50"}             # 5 GB a window; 250 bytes a window: the first record of a name, then nothing


def record(name, i):
    """92 92 d7 00 <sec> <nsec> 80 {n: <10-byte name>, log: <200 bytes>, i: <u32>}: 240 bytes (RECORD_BYTES)"""
    return (b"\x92\x92\xd7\x00" + struct.pack(">II", 1700000000 + (i >> 10), i & 1023) + b"\x80\x83\xa1n\xaa" + name + b"\xa3log\xc4\xc8" + LOG +
            b"\xa1i\xce" + struct.pack(">I", i))


RECORD_BYTES = len(record(b"0" * 10, 0))


def chunk(dist, n):
    names = {"one": 1, "k1000": 1000, "each": n}[dist]
    return b"".join(record(b"%010d" % (i % names), i) for i in range(n))


def dev_chunk(g, blob, n):
    L = g.lib()
    step = len(blob) // n
    d = L.flbgpu_dev_alloc(len(blob) + 16)
    L.flbgpu_memcpy_h2d(d, blob, len(blob))
    ro = struct.pack("<%dQ" % (n + 1), *range(0, len(blob) + 1, step))
    d_off = L.flbgpu_dev_alloc(len(ro))
    L.flbgpu_memcpy_h2d(d_off, ro, len(ro))
    return g.DevChunk(d, d_off, n, len(blob)), (d, d_off)


def measure(g, ch, props, repeats):
    runs = []
    for r in range(repeats + 1):
        f = g.FilterThrottleSize(props)
        try:
            f.set_now(1700000000)
            f.profile(True)
            t0 = time.perf_counter()
            ret, _ = f.filter_dev(ch)
            wall = (time.perf_counter() - t0) * 1e3
            prof = f.profile_read()
            c = f.counters()
        finally:
            f.close()
        if r:
            runs.append((sum(ms for ms, _ in prof.values()), wall, prof, ret, c))
    runs.sort(key=lambda x: x[0])
    dev, wall, prof, ret, c = runs[len(runs) // 2]
    admit = sum(ms for k, (ms, _) in prof.items() if k.startswith("k_tsz_admit"))      # <lane> and <wave>; the order has a scope of its own
    return dict(device_ms=round(dev, 3), device_ms_range=[round(runs[0][0], 3), round(runs[-1][0], 3)], wall_ms=round(statistics.median(x[1] for x in runs), 3),
                kernels_ms={k: round(ms, 3) for k, (ms, _) in prof.items()}, admit_share=round(admit / dev, 3) if dev else None, ret=ret,
                kept=c["kept"], dropped=c["dropped"], windows=c["live"])


def cpu_reference(a):
    import gen_throttle_golden as gt
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    out = {}
    with tempfile.TemporaryDirectory(prefix="throttle_perf_") as tmp:
        host, sos = gt.build_reference(a.reference, engine, tmp)
        n = 20000
        for dist in ("one", "k1000", "each"):
            for rk, rate in RATES.items():
                steps = [("now", 1700000000), ("tick", 1700000000), ("chunk", chunk(dist, n))]
                _, _, rest = gt.run_case(host, sos["throttle_size"], "throttle_size", PROPS + [("rate", rate)], steps, tmp, extra=("--repeat-ns", "5"))
                ns = [x["filter_ns"] for x in rest if "filter_ns" in x][0]
                out["%s_%s" % (dist, rk)] = dict(records=n, filter_ms=round(ns / 1e6, 3), records_per_s=round(n / (ns / 1e9)))
    return dict(note="the real plugin on one CPU core of the machine this ran on (calls after the first: the windows are warm)", configs=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "throttle_size_perf.json"))
    ap.add_argument("--wave-min-compare", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--reference", default=os.environ.get("REF"))
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.cpu_reference:
        res["reference_cpu"] = cpu_reference(a)
    else:
        import flbamd_loader
        g = flbamd_loader.load()
        g.init(0)
        dists = [a.child] if a.child else ["one", "k1000", "each"]
        out = {}
        for dist in dists:
            print("building", dist, flush=True)
            blob = chunk(dist, a.records)
            ch, mem = dev_chunk(g, blob, a.records)
            for rk, rate in RATES.items():
                print("measuring", dist, rk, flush=True)
                out["%s_%s" % (dist, rk)] = measure(g, ch, PROPS + [("rate", rate)], a.repeats)
                print(dist, rk, json.dumps(out["%s_%s" % (dist, rk)]), flush=True)
            for d in mem:
                g.lib().flbgpu_dev_free(d)
            del blob
        if a.child:
            print("CHILD " + json.dumps(out))
            return
        res.update(records=a.records, record_bytes=RECORD_BYTES, measured_on="one MI355X, one run", configs=out)
        if a.wave_min_compare:
            # 100000 is the setting the tests use; a segment of more rows than that still takes a wave, so the one-lane path over the
            # whole skewed chunk needs a threshold no chunk reaches
            import subprocess
            adm = lambda x: sum(ms for k, ms in x["kernels_ms"].items() if k.startswith("k_tsz_admit"))
            for wm in ("100000", "2147483647"):
                env = dict(os.environ, FLBGPU_TSZ_WAVE_MIN=wm)
                print("child under FLBGPU_TSZ_WAVE_MIN=" + wm, flush=True)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "one", "--records", str(a.records), "--repeats", "1"], env=env,
                                   stdout=subprocess.PIPE, timeout=900)
                line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("CHILD ")]
                if r.returncode == 0 and line:
                    lane = json.loads(line[0][6:])
                    res["wave_min_" + wm] = lane
                    res["admit_ms_over_default_wave_min_" + wm] = {k: round(adm(lane[k]) / adm(out[k]), 2) if adm(out[k]) else None for k in lane}
                    res["call_ms_over_default_wave_min_" + wm] = {k: round(lane[k]["device_ms"] / out[k]["device_ms"], 2) for k in lane}
                else:
                    res["wave_min_" + wm] = "missing: the child run failed"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k.startswith(("admit_ms_over", "call_ms_over"))}))


if __name__ == "__main__":
    main()

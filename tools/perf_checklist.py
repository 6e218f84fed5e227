#!/usr/bin/env python3
"""filter_checklist on 4 M apache-shaped parsed records resident in HBM, next to filter_record_modifier on the same chunk.

  E1k   mode exact,   1 000 entries          E1M   mode exact,   1 000 000 entries
  P100  mode partial, 100 literal entries    P10k  mode partial, 10 000 literal entries
  A100  mode partial, 100 entries in the `any` bucket (they begin with '_' or '%')
  R     filter_record_modifier adding the same pair (the yardstick: the existing filter that also rewrites every record it touches)

The chunk is the one of tools/perf_typeconv.py with a `host` of which one record in ten starts with "10." -- the lists hold those
hosts (exact) or their first two octets (partial); every other entry is filler that no record meets.  Each run has a 10 % match
share.  Per configuration: ms per call from the library's own device timing (event pairs around every launch of the call --
flbgpu_filter_profile), the wall time next to it, records per second, and the ratio over R measured in the same run, call by call
in turn; the spread is the range over the repeated calls.  Needs a GPU: there is no CPU path.
--cpu-reference (no GPU; a development machine with a fluent-bit source tree and `make -C oracle engine`): the real plugin's cb_filter
on a 2 MB chunk of the same records with the same lists, through tools/checklist_ref_host.c, best of three; written into the same
file under "reference_cpu", marked as a CPU number of the machine it ran on.
Usage: perf_checklist.py [--records N] [--repeats K] [--out profiles/checklist_perf.json] [--cpu-reference --reference TREE]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402
from perf_recmod import AGENTS, BLOCK, ROOF, kernel_ms  # noqa: E402

PAIR = ("flagged", "yes")
OTHER_OCTETS = [o for o in range(11, 256) if o % 10]


def block(seed):
    """BLOCK records; (bytes, the hosts of the one record in ten whose host starts with "10.")"""
    r = random.Random(seed)
    out, hits = [], []
    for i in range(BLOCK):
        if i % 10 == 3:
            host = "10.%d.%d.%d" % (r.randrange(50), r.randrange(4), r.randrange(3))
            hits.append(host)
        else:
            # (no first octet ends in 0: "_0.k." of the `any` list meets the "10." hosts alone)
            host = "%d.%d.%d.%d" % (r.choice(OTHER_OCTETS), r.randrange(256), r.randrange(256), r.randrange(256))
        out.append(synth.mp([[synth.ext_ts(1700000000 + i, r.randrange(10 ** 9)), {}], synth.KV([
            (b"host", host), (b"user", "-"), (b"time", "10/Oct/2023:13:55:%02d +0000" % (i % 60)), (b"method", r.choice(["GET", "POST", "PUT"])),
            (b"path", "/api/v1/items/%d?page=%d" % (r.randrange(100000), r.randrange(50))), (b"status", r.choice(["200", "404", "500", "503"])),
            (b"size", str(r.randrange(100000))), (b"latency", "%d.%03d" % (r.randrange(3), r.randrange(1000))), (b"agent", r.choice(AGENTS))])]))
    return b"".join(out), sorted(set(hits))


def lists(hits):
    r = random.Random(7)

    def filler(n, fmt):
        return [fmt % (r.randrange(300, 1000), r.randrange(256), r.randrange(256), i) for i in range(n)]
    assert len(hits) <= 600
    two = ["10.%d." % k for k in range(50)]
    return {
        "E1k": ("exact", hits + filler(1000 - len(hits), "%d.%d.%d.%d")),
        "E1M": ("exact", hits + filler(1000000 - len(hits), "%d.%d.%d.%d")),
        "P100": ("partial", two + filler(50, "%d.%d.%d.%d")),
        "P10k": ("partial", two + filler(9950, "%d.%d.%d.%d")),
        "A100": ("partial", ["_0.%d." % k for k in range(50)] + ["%%zz%d.%d.%d.%d" % (a, b, c, i) for i, (a, b, c) in
                                                                  enumerate((r.randrange(256), r.randrange(256), r.randrange(256)) for _ in range(50))]),
    }


def cpu_reference(a):
    import subprocess
    from gen_checklist_golden import build_reference
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    blk, hits = block(1)
    # whole records up to 2 MB
    import modify_model as mm
    p = 0
    while p < 2 * 1024 * 1024:
        p = mm.decode_event(blk, p)[0]
    chunk = blk[:p]
    nrec = len(synth.unpack_all(chunk))
    res = dict(machine="CPU, one core of the development machine (not the GPU host)", chunk_bytes=len(chunk), records=nrec, configs={})
    with tempfile.TemporaryDirectory(prefix="checklist_perf_") as tmp:
        host, so = build_reference(a.reference, engine, tmp)
        fin, fout = os.path.join(tmp, "in.mp"), os.path.join(tmp, "out.mp")
        with open(fin, "wb") as f:
            f.write(chunk)
        for k, (mode, ents) in lists(hits).items():
            path = os.path.join(tmp, k + ".txt")
            with open(path, "w") as f:
                f.write("".join(e + "\n" for e in ents))
            best = None
            for _ in range(3):
                r = subprocess.run([host, so, fin, fout, "file=" + path, "lookup_key=host", "mode=" + mode, "record=%s %s" % PAIR],
                                   stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
                ans = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
                assert ans["init"] and ans["ret"] == 1, ans
                best = ans["filter_ns"] if best is None else min(best, ans["filter_ns"])
            res["configs"][k] = dict(entries=len(ents), filter_ms=best / 1e6, ns_per_record=best / nrec, ms_per_4M_records=best / nrec * 4e6 / 1e6)
            print("%-5s reference plugin: %.2f ms for %d records, %.0f ns a record" % (k, best / 1e6, nrec, best / nrec))
    cur = json.load(open(a.out)) if os.path.exists(a.out) else {}
    cur["reference_cpu"] = res
    with open(a.out, "w") as f:
        json.dump(cur, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4000000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checklist_perf.json"))
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree (--cpu-reference)")
    a = ap.parse_args()
    if a.cpu_reference:
        return cpu_reference(a)
    import flbamd_loader
    g = flbamd_loader.load()
    g.init(0)
    L = g.lib()
    blk, hits = block(1)
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
    fs, entries = {}, {}
    with tempfile.TemporaryDirectory(prefix="checklist_perf_") as tmp:
        for k, (mode, ents) in lists(hits).items():
            path = os.path.join(tmp, k + ".txt")
            with open(path, "w") as f:
                f.write("".join(e + "\n" for e in ents))
            fs[k] = g.FilterChecklist([("file", path), ("lookup_key", "host"), ("mode", mode), ("record", "%s %s" % PAIR)])
            entries[k] = len(ents)
    fs["R"] = g.FilterRecordModifier([("Record", "%s %s" % PAIR)])
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
            assert ret == g.MODIFIED, (k, ret, g.last_error())
            if it >= 2:
                stat[k]["kernel_ms"].append(ms)
                stat[k]["wall_ms"].append(wall)
            outs[k] = int(out.bytes)
    res = dict(records=int(chunk.n), in_bytes=nbytes, roof_bytes_per_s=ROOF, repeats=a.repeats, pair=list(PAIR), match_share=0.1, configs={})
    for k, s in stat.items():
        med = statistics.median(s["kernel_ms"])
        res["configs"][k] = dict(filter="record_modifier" if k == "R" else "checklist", entries=entries.get(k), out_bytes=outs[k], kernel_ms_median=med,
                                 kernel_ms_min=min(s["kernel_ms"]), kernel_ms_max=max(s["kernel_ms"]), wall_ms_median=statistics.median(s["wall_ms"]),
                                 kernel_ms_all=s["kernel_ms"], records_per_s=int(chunk.n) / (med * 1e-3),
                                 per_kernel={kn: v[0] / (a.repeats + 2) for kn, v in seen[k].items()})
    rmed = res["configs"]["R"]["kernel_ms_median"]
    for k, f in fs.items():
        c = res["configs"][k]
        if k != "R":
            cn = f.counters()
            assert cn[3] == 0 and cn[0] == (a.repeats + 2) * int(chunk.n) // 10, (k, cn)
            c["matched_per_call"] = cn[0] // (a.repeats + 2)
            c["record_modifier_kernel_ms_median"] = rmed
            c["over_record_modifier"] = c["kernel_ms_median"] / rmed
        print("%-5s kernel ms median %.3f (min %.3f max %.3f)  wall %.3f  %.1f M records/s  %s" %
              (k, c["kernel_ms_median"], c["kernel_ms_min"], c["kernel_ms_max"], c["wall_ms_median"], c["records_per_s"] / 1e6,
               "" if k == "R" else "x%.2f of R" % c["over_record_modifier"]))
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

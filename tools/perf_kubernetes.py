#!/usr/bin/env python3
"""filter_kubernetes on 4 M docker-JSON records resident in HBM, a 600-byte pod blob appended to every record.

  M    merge_log on (keep_log on, trim on): every record's `log` is a JSON object of five pairs that is parsed and merged
  MK   the same under merge_log_key          MO   keep_log off          N    merge_log off (re-encode and append only)
  MH   M with the LDS budget of the tail at 0 (FLBGPU_KUBE_LDS_BLOB=0, set before the filter is created): the tail from HBM / L2

Per configuration: ms per call from the library's own device timing (event pairs around every launch of the call --
flbgpu_filter_profile), the median of the repeated calls after two warm-up calls, the range as the spread; records per second, GB/s
over the bytes the call must move (chunk in + chunk out) and that figure as a share of the 8 TB/s roof.  Needs a GPU: there is no CPU
path.
--cpu-reference (no GPU; a development machine with a fluent-bit source tree and `make -C oracle engine`): the real plugin's cb_filter
on a 2 MB chunk of the same records with the same blob from a preloaded meta file, through tools/kube_ref_host.c, the fastest of five
calls; written into the same file under "reference_cpu", marked as a CPU number of the machine it ran on.
Usage: perf_kubernetes.py [--records N] [--repeats K] [--out profiles/kube_perf.json] [--cpu-reference --reference TREE]"""
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
from kube_chunks import docker, json_line, kv  # noqa: E402

CONFIGS = {
    "M": [("merge_log", "on")],
    "MK": [("merge_log", "on"), ("merge_log_key", "parsed")],
    "MO": [("merge_log", "on"), ("keep_log", "off")],
    "N": [("merge_log", "off")],
    "MH": [("merge_log", "on")],
}
BLOB_BYTES = 600


def pod_blob():
    """a pod map of BLOB_BYTES bytes in the reference's shape"""
    base = [("pod_name", "apache-logs-5d8f7c9b6d-x2x7q"), ("namespace_name", "default"), ("pod_id", "e9f2963f-55f2-4c85-8d52-6a9a38e2a78c"),
            ("host", "node-1.cluster.local"), ("container_name", "apache"), ("docker_id", "0123456789abcdef" * 4), ("container_image", "apache:2.4")]
    labels = [("app.kubernetes.io/label-%d" % i, "value-%d" % i) for i in range(6)]
    for pad in range(400):
        b = synth.mp(kv(*(base[:3] + [("labels", kv(*labels)), ("annotations", kv(("note", "x" * pad)))] + base[3:])))
        if len(b) == BLOB_BYTES:
            return b
    raise AssertionError("no blob of %d bytes" % BLOB_BYTES)


def block():
    return b"".join(docker(i, json_line(i) + "\n") for i in range(BLOCK))


def cpu_reference(a):
    import subprocess
    from gen_kube_golden import KUBE_URL, build_reference, tag_of
    import modify_model as mm
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    blk = b"".join(docker(i, json_line(i) + "\n") for i in range(16000))
    p = 0
    while p < 2 * 1024 * 1024:                               # whole records up to 2 MB
        p = mm.decode_event(blk, p)[0]
    chunk = blk[:p]
    nrec = len(synth.unpack_all(chunk))
    res = dict(machine="CPU, one core of the development machine (not the GPU host)", chunk_bytes=len(chunk), records=nrec, configs={})
    with tempfile.TemporaryDirectory(prefix="kube_perf_") as tmp:
        host, so = build_reference(a.reference, engine, tmp)
        fin, fout, cache = os.path.join(tmp, "in.mp"), os.path.join(tmp, "out.mp"), os.path.join(tmp, "meta")
        os.mkdir(cache)
        # a preloaded file whose merged map is about the blob's size: labels and an annotation of the padding's length
        with open(os.path.join(cache, "default_apache-logs.meta"), "w") as f:
            json.dump({"metadata": {"name": "apache-logs", "namespace": "default", "uid": "e9f2963f-55f2-4c85-8d52-6a9a38e2a78c",
                                    "labels": {"app.kubernetes.io/label-%d" % i: "value-%d" % i for i in range(6)}, "annotations": {"note": "x" * 150}},
                       "spec": {"nodeName": "node-1.cluster.local"}}, f)
        with open(fin, "wb") as f:
            f.write(chunk)
        for k in ("M", "MK", "MO", "N"):
            props = CONFIGS[k] + [("kube_url", KUBE_URL), ("kube_meta_preload_cache_dir", cache)]
            r = subprocess.run([host, so, fin, fout, tag_of("apache-logs"), "--repeat", "5"] + ["%s=%s" % x for x in props], stdout=subprocess.PIPE,
                               stderr=subprocess.DEVNULL, check=True)
            ans = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
            assert ans["init"] and ans["ret"] == 1, ans
            ns = ans["filter_ns"]
            res["configs"][k] = dict(filter_ms=ns / 1e6, ns_per_record=ns / nrec, out_bytes=ans["out_bytes"], ms_per_4M_records=ns / nrec * 4e6 / 1e6)
            print("%-3s reference plugin: %.3f ms for %d records (%d -> %d bytes), %.0f ns a record" % (k, ns / 1e6, nrec, len(chunk), ans["out_bytes"], ns / nrec))
    cur = json.load(open(a.out)) if os.path.exists(a.out) else {}
    cur["reference_cpu"] = res
    with open(a.out, "w") as f:
        json.dump(cur, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4000000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kube_perf.json"))
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree (--cpu-reference)")
    a = ap.parse_args()
    if a.cpu_reference:
        return cpu_reference(a)
    import flbamd_loader
    g = flbamd_loader.load()
    g.init(0)
    L = g.lib()
    blk = block()
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
    blob = pod_blob()
    fs = {}
    for k, p in CONFIGS.items():
        if k == "MH":
            os.environ["FLBGPU_KUBE_LDS_BLOB"] = "0"         # read when the filter is created
        fs[k] = g.FilterKubernetes(p)
        os.environ.pop("FLBGPU_KUBE_LDS_BLOB", None)
        fs[k].set_meta(blob, None)
        assert fs[k].layout()["in_lds"] == (k != "MH")
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
    res = dict(records=int(chunk.n), in_bytes=nbytes, blob_bytes=len(blob), roof_bytes_per_s=ROOF, repeats=a.repeats, configs={})
    for k, s in stat.items():
        med = statistics.median(s["kernel_ms"])
        moved = nbytes + outs[k]
        c = dict(props=CONFIGS[k], tail_in_lds=k != "MH", out_bytes=outs[k], kernel_ms_median=med, kernel_ms_min=min(s["kernel_ms"]), kernel_ms_max=max(s["kernel_ms"]),
                 wall_ms_median=statistics.median(s["wall_ms"]), kernel_ms_all=s["kernel_ms"], records_per_s=int(chunk.n) / (med * 1e-3),
                 moved_bytes=moved, gb_per_s=moved / (med * 1e-3) / 1e9, of_the_roof=moved / (med * 1e-3) / ROOF,
                 per_kernel={kn: v[0] / (a.repeats + 2) for kn, v in seen[k].items()})
        res["configs"][k] = c
        cn = fs[k].counters()
        assert cn[3] == 0 and cn[0] == (0 if k == "N" else (a.repeats + 2) * int(chunk.n)), (k, cn)
        print("%-3s kernel ms median %.3f (min %.3f max %.3f)  wall %.3f  %.1f M records/s  %.0f GB/s = %.3f of the roof" %
              (k, med, c["kernel_ms_min"], c["kernel_ms_max"], c["wall_ms_median"], c["records_per_s"] / 1e6, c["gb_per_s"], c["of_the_roof"]))
        print("      per kernel ms:", {kn: round(v, 3) for kn, v in c["per_kernel"].items()})
        fs[k].close()
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

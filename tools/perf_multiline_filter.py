#!/usr/bin/env python3
"""filter_multiline on the device next to the multiline core on text: the Java-log lines of tools/perf_ml.py, once as text through
flbgpu_ml_append_dev and once wrapped as {"log": line} records through FilterMultiline (mode parser, buffer off, built-in java), on
the same machine.  Wall time per call, scaled to 4 M lines, and the ratio record form / text form go to
profiles/multiline_filter_perf.json.  The record form reads msgpack around every line and re-packs maps, so a ratio above 1 is
expected; no threshold is set.  usage: perf_multiline_filter.py [lines] [reps]"""
import json
import os
import random
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flbamd_loader
import ml_synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
g = flbamd_loader.load()
g.init(0)
L = g.lib()
block = ml_synth.java_service_log(random.Random(1), 20000)
lines = block.split(b"\n")[:-1]


def record(line, i):
    n_ = len(line)
    hdr = bytes([0xa0 | n_]) if n_ < 32 else bytes([0xd9, n_]) if n_ < 256 else b"\xda" + struct.pack(">H", n_) if n_ < 65536 else b"\xdb" + struct.pack(">I", n_)
    return b"\x92\x92\xd7\x00" + struct.pack(">II", 1700000000 + i // 1000, i % 1000 + 1) + b"\x80\x81\xa3log" + hdr + line


rblock = b"".join(record(ln, i) for i, ln in enumerate(lines))
k = max(n // len(lines), 1)
text, recs = block * k, rblock * k
nl = len(lines) * k


def timed(fn):
    best = None
    for _ in range(reps):
        L.flbgpu_sync()
        t0 = time.perf_counter()
        fn()
        L.flbgpu_sync()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best


d_text = L.flbgpu_dev_alloc(len(text))
L.flbgpu_memcpy_h2d(d_text, text, len(text))
s = g.MultilineParser(builtin="java").stream()
t_text = timed(lambda: s.append_dev(d_text, len(text), 1700000000, 5, flush=True))
d_recs = L.flbgpu_dev_alloc(len(recs))
L.flbgpu_memcpy_h2d(d_recs, recs, len(recs))
f = g.FilterMultiline([("multiline.parser", "java"), ("multiline.key_content", "log"), ("buffer", "off")])
res = {}


def run_filter():
    res["ret"], res["out"] = f.filter_dev(g.DevChunk(d_recs, None, 0, len(recs)))


t_rec = timed(run_filter)
assert res["ret"] == g.MODIFIED, g.last_error()
scale = 4_000_000 / nl
out = dict(lines=nl, text_bytes=len(text), record_bytes=len(recs), reps=reps, text_ms_per_4m_lines=t_text * 1e3 * scale, filter_ms_per_4m_lines=t_rec * 1e3 * scale,
           ratio=t_rec / t_text, filter_records_out=int(res["out"].n), counters=f.counters())
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "multiline_filter_perf.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))

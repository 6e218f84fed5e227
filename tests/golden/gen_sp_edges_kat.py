#!/usr/bin/env python3
"""Generates tests/golden/sp_edges_kat.json: what the reference's OWN stream processor (src/stream_processor/*.c compiled in place:
oracle/_ref/ref_sp, `make -C oracle ref`) answers for every named case of tests/sp_chunks.py -- per case the SHA-256 of its chunks, the
record counts of its steps, SHA-256 and length of the output bytes.  grid/second_trip (an answer scaled from one block) is recorded as constructed, its construction
being held against the binary at small repeat counts.  Needs the reference tree; the JSON file is committed so that the oracle's
restatement stays pinned where the reference is absent."""
import json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_sp
import sp_chunks as sc

assert ref_sp.available(), "oracle/_ref/ref_sp is not built"
out = []
for c in sc.all_cases():
    want = c.want()
    if c.ref:
        r = ref_sp.RefSp(c.sql, str_conv=c.str_conv)
        got = c.run(r)
        r.close()
        assert got == want, c.name
    out.append(c.digest())
json.dump({"generator": "tests/golden/gen_sp_edges_kat.py", "source": "oracle/_ref/ref_sp (src/stream_processor/*.c)", "cases": out},
          open(os.path.join(HERE, "sp_edges_kat.json"), "w"), indent=0)
print(len(out), "cases")

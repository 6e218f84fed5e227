#!/usr/bin/env python3
"""Generates tests/golden/dec_edges_kat.json: what the reference's OWN filter_parser (plugins/filter_parser/filter_parser.c over
src/flb_parser*.c and src/flb_parser_decoder.c, compiled in place: oracle/_ref/ref_filters, `make -C oracle ref`) answers for every
named case of tests/dec_chunks.py: return code, SHA-256 and length of the output bytes, SHA-256 of the chunk.  Needs the reference
tree; the JSON file is committed so that the oracle's restatement stays pinned where the reference is absent."""
import hashlib, json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dec_chunks as dc
import ref_filters as rf

cs = dc.all_cases()
res = rf.run([rf.parser_case(c.key, c.parsers, c.data, c.reserve, c.preserve) for c in cs])
out = [{"case": c.name, "ret": ret, "sha256": hashlib.sha256(o).hexdigest(), "bytes": len(o), "chunk_sha256": hashlib.sha256(c.data).hexdigest()}
       for c, (ret, o) in zip(cs, res)]
json.dump({"generator": "tests/golden/gen_dec_edges_kat.py", "source": "oracle/_ref/ref_filters (filter_parser.c + flb_parser_decoder.c, yyjson backend)",
           "cases": out}, open(os.path.join(HERE, "dec_edges_kat.json"), "w"), indent=0)
print(len(out), "cases")

"""in_tail's line packing: the oracle's restatement (oracle/oflb.c oflb_tail_process: process_content's loop + the record
layout of flb_tail_file_pack_line) against the reference's REAL event encoder driven through the same call sequence
(oracle/_ref/ref_filters kind 4) on the CPU, and the device path (tail_kernels.inc, through the C ABI) against the oracle.
The named texts of tests/tail_chunks.py run through the same two CPU comparisons and through the plain Python restatement of
tests/tail_model.py; the floors below keep each of them on the edge of the kernels it was written for (the device side of them:
tests/test_tail_gpu.py)."""
import os, random, re, sys
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_binding as ob
import ref_filters as rf
import tail_chunks as tc
import tail_model as tm

TS = dict(sec=1700000000, nsec=123456789)


def _texts(seed, n=40):
    rng = random.Random(seed)
    out = [b"", b"\n", b"\r\n", b"no newline at all", b"\0\0\0", b"\0\0abc\n", b"a\n\n\r\nb\r\n", b"x\r\r\n", b"\r\n\r\n", b"last\nline without newline",
           b"long " + b"y" * 70000 + b"\nshort\n", b"\xff\xfe\n\xc3\xa9\n", b"tab\there\n \n"]
    for _ in range(n):
        parts = []
        for _ in range(rng.randrange(0, 400)):
            r = rng.random()
            if r < 0.1: line = b""
            elif r < 0.15: line = b"\r"
            elif r < 0.8: line = bytes(rng.choice(b"abcdefghij 0123456789\"[]/-.:") for _ in range(rng.randrange(1, 300)))
            else: line = bytes(rng.randrange(1, 256) for _ in range(rng.randrange(1, 40))).replace(b"\n", b" ")
            parts.append(line + rng.choice([b"\n", b"\n", b"\r\n"]))
        t = b"".join(parts)
        if rng.random() < 0.5: t += b"partial line"
        if rng.random() < 0.2: t = b"\0" * rng.randrange(1, 200) + t
        out.append(t)
    return out


CONFIGS = [dict(), dict(skip_empty_lines=False), dict(key="message", path_key="file", path="/var/log/app/a.log"),
           dict(offset_key="offset", stream_offset=123456789012), dict(path_key="p", path="", offset_key="o", stream_offset=250, skip_empty_lines=False)]


@pytest.mark.skipif(not rf.available(), reason="oracle/_ref/ref_filters not built (no reference tree)")
def test_oracle_against_the_real_encoder():
    cases, wants = [], []
    for t in _texts(1):
        for c in CONFIGS:
            cases.append(rf.tail_case(t, sec=1700000000, nsec=123456789, **c))
            wants.append(ob.tail_process(t, sec=1700000000, nsec=123456789, **c))
    for _, _, t, c in tc.cases():
        cases.append(rf.tail_case(t, **TS, **c))
        wants.append(ob.tail_process(t, **TS, **c))
    for res, want in zip(rf.run(cases), wants):
        assert rf.tail_result(res) == want


def test_model_against_the_oracle():
    """tail_model.records, written from the reference's rules, gives the oracle's bytes, line count and consumed bytes on every
    named text (and on the hand-written ones above)"""
    named = tc.cases() + [("random", "text %d" % i, t, c) for i, t in enumerate(_texts(3, 6)) for c in CONFIGS]
    for grp, label, text, c in named:
        rows, processed = tm.records(text, **TS, **c)
        want = ob.tail_process(text, **TS, **c)
        assert len(rows) == text.count(b"\n"), (grp, label, c)
        assert (sum(1 for r in rows if r), processed) == (want[0], want[2]), (grp, label, c)
        assert b"".join(rows) == want[1], (grp, label, c)


def _csrc(name):
    return open(os.path.join(HERE, "..", "fluent-bit_amd", "csrc", name)).read()


def test_model_constants_match_the_kernels():
    """emit_paths and the corpus are laid out for these numbers: a change to one of them must come back here"""
    src = _csrc("tail_kernels.inc")
    const = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, src).group(1))
    assert (const("TL_TILE"), const("TL_TILE_T"), const("TL_STG")) == (tm.TL_TILE, tm.TL_TILE_T, tm.TL_STG)
    assert tm.TL_TILE == 64 * tm.TL_TILE_T
    size = re.search(r"void launch_tl_size\(.*?\n}", src, re.S).group(0)
    assert re.search(r"\(a\.nl \+ 255\) / 256;\s*if \(blocks > (\d+)\) blocks = \1;", size).group(1) == str(tm.SIZE_BLOCKS)
    assert "dim3(256)" in size
    emit = re.search(r"void launch_tl_emit\(.*?\n}", src, re.S).group(0)
    assert re.search(r"tiles = \(a\.nl \+ 63\) / 64, blocks = \(tiles \+ 3\) / 4, cap = \(uint64_t\) cus \* (\d+);", emit).group(1) == str(tm.EMIT_BLOCKS_PER_CU)
    assert "dim3(256), (size_t) 4 * TL_STG" in emit
    assert int(re.search(r"uint8_t pre\[(\d+)\];", _csrc("dev.hpp")).group(1)) == 1024


def _sizes(text, **c):
    return [len(r) for r in tm.records(text, **c)[0]]


def test_staging_text_reaches_every_path_of_the_emit_kernel():
    (_, text, cfgs), = tc.group("staging")
    assert cfgs[0] == {}
    sizes = _sizes(text)
    assert {18943, 18944, 18945} <= set(sizes)
    ep = tm.emit_paths(sizes)
    assert {(0, 63), (1, 0), (1, 31)} <= set(ep["direct"]), ep["direct"]
    assert any(t == len(ep["batches"]) - 1 for t, _ in ep["direct"]) and len(sizes) % 64 != 0          # in a partial last tile
    assert {l for _, l in ep["direct"]} >= {0, 31, 63}
    off = [sum(sizes[:i]) for i in range(len(sizes))]
    assert any(sizes[64 * t + l] == 18945 and off[64 * t + l] % 16 == 0 for t, l in ep["direct"])     # one byte over at align 0
    assert len(ep["exact"]) >= 2 and {0, 1} <= {a for _, _, a in ep["exact"]}, ep["exact"]
    assert ep["aligns"] == set(range(16)), ep["aligns"]
    assert max(ep["batches"]) >= 4, ep["batches"]
    # skipped rows inside a batch: an empty row that is neither the first nor the last row of the rows a batch covers
    assert sizes[1] == 0 and (0, 0, 0) in ep["exact"] and sizes[0] == 18944
    assert any(sizes[64 + l] == 0 for l in range(20, 26))
    # the second config moves every boundary: it must still meet the direct path and several batches per tile
    ep2 = tm.emit_paths(_sizes(text, **cfgs[1]))
    assert len(ep2["direct"]) >= 4 and max(ep2["batches"]) >= 4


def test_many_lines_text_takes_a_second_trip():
    (_, text, cfgs), = tc.group("many_lines")
    nl = text.count(b"\n")
    assert nl >= 1_100_000 and len(text) < 2_500_000
    assert nl > tm.SIZE_BLOCKS * 256 and nl > 256 * tm.EMIT_BLOCKS_PER_CU * 256          # 256 CUs: the MI355X
    assert tm.second_trips(nl, 256) == (True, True)
    assert set(text[:13].split(b"\n")[:-1]) == {b"a", b"ab\r", b"", b"\r", b"b"} and text == text[:13] * (len(text) // 13)
    so = cfgs[1]["stream_offset"]
    assert so < 2 ** 32 <= so + len(text) - 16 and cfgs[1]["offset_key"]


def test_edge_texts_sit_on_the_edges():
    texts = {label: text for label, text, _ in tc.group("edges")}
    for p in (62, 63, 64, 65, 16382, 16383, 16384, 16385, 32767, 32768):
        assert texts["newline at byte %d" % p].index(b"\n") == p
    for n in (63, 64, 65, 16383, 16384, 16385):
        a, b = texts["%d bytes, final newline" % n], texts["%d bytes, no final newline" % n]
        assert len(a) == len(b) == n and a.endswith(b"\n") and not b.endswith(b"\n") and b.count(b"\n") >= 4
    t = texts["64 newlines in one mask word"]
    assert t[64:128] == b"\n" * 64 and len(tm.records(t, skip_empty_lines=False)[0]) == 65
    t = texts["a tile without a newline"]
    assert b"\n" not in t[tm.TL_TILE:2 * tm.TL_TILE] and b"\n" in t[:tm.TL_TILE] and b"\n" in t[2 * tm.TL_TILE:]
    assert texts["CR LF across a 64-byte edge"][63:65] == texts["CR LF across a 16 KB edge"][16383:16385] == b"\r\n"
    assert texts["a lone CR across a 64-byte edge"][62:65] == texts["a lone CR across a 16 KB edge"][16382:16385] == b"\n\r\n"
    # every value next to a newline, the newline in every byte lane of a dword, in both halves of a thread's 64 bytes
    nb = tc.group("neighbours")[0][1]
    seen = {}
    for i in range(1, len(nb) - 3):
        if nb[i] == 10 and nb[i - 1] == nb[i + 1]:
            seen.setdefault(("vnv", nb[i + 1]), set()).add((i % 4, i % 64 // 32))
        if nb[i] == 10 and nb[i + 1] == nb[i + 2] == nb[i + 3]:
            seen.setdefault(("nvvv", nb[i + 1]), set()).add((i % 4, i % 64 // 32))
    full = {(lane, half) for lane in range(4) for half in range(2)}
    assert all(seen.get((k, v)) == full for k in ("vnv", "nvvv") for v in range(256)), [k for k in seen if seen[k] != full][:8]
    noise = tc.group("neighbours")[1][1]
    assert len(noise) == 65536 and set(noise) == set(range(256)) and noise[0] != 0


def test_encoding_texts_cross_every_header_size():
    (_, lengths, _), (_, walk, wcfgs), (_, _, kcfgs) = tc.group("encodings")
    lines = lengths.split(b"\n")[:-1]
    assert [len(l) for l in lines] == [n + k for n in tc.LENGTHS for k in (0, 1)] and all(l.endswith(b"\r") for l in lines[1::2])
    starts, pos = [], 0
    for l in walk.split(b"\n")[:-1]:
        starts.append((pos, l))
        pos += len(l) + 1
    for bound in tc.BOUNDS:
        for c in (c for c in wcfgs if bound - 64 < c["stream_offset"] < bound):
            kept = [c["stream_offset"] + s for s, l in starts if l or not c["skip_empty_lines"]]
            assert any(v < bound for v in kept) and bound in kept, (bound, c)
        assert any(bound - 2 in [c["stream_offset"] + s for s, l in starts if l] for c in wcfgs if c["skip_empty_lines"])
        assert any(bound - 1 in [c["stream_offset"] + s for s, l in starts] for c in wcfgs if not c["skip_empty_lines"])
    for name in ("key", "path_key", "path", "offset_key"):
        assert {len(c[name]) for c in kcfgs if name in c} >= {31, 32, 255}
    assert any(c.get("path_key") and c.get("path") == "" for c in kcfgs)


@pytest.mark.gpu
def test_device_against_the_oracle():
    import flbamd_loader
    g = flbamd_loader.load()
    g.init(0)
    for c in CONFIGS:
        so = c.get("stream_offset", 0)
        kw = {k: v for k, v in c.items() if k != "stream_offset"}
        t = g.TailLines(**kw)
        for text in _texts(2, 25):
            want = ob.tail_process(text, sec=1700000000, nsec=5, **c)
            got = t.process(text, stream_offset=so, sec=1700000000, nsec=5)
            assert got[0] == want[0] and got[2] == want[2], (c, len(text), got[0], want[0], got[2], want[2])
            assert got[1] == want[1], (c, len(text))
        t.close()


@pytest.mark.gpu
def test_device_lines_feed_the_filters():
    """text -> events on the device -> filter_parser + filter_grep without leaving HBM: the chain's output equals the oracle's"""
    import flbamd_loader, synth
    from bench import APACHE2, TIME_FMT, GREP_RULE
    g = flbamd_loader.load()
    g.init(0)
    data, off, _ = synth.apache_records(5000)
    blob = bytes(data)
    text = b"".join(blob[int(off[i]) + 21:int(off[i + 1])] + b"\n" for i in range(5000))
    L = g.lib()
    d = L.flbgpu_dev_alloc(len(text)); L.flbgpu_memcpy_h2d(d, text, len(text))
    t = g.TailLines()
    lines, chunk, processed = t.process_dev(d, len(text), sec=7, nsec=8)
    assert lines == 5000 and processed == len(text)
    p = g.Parser(APACHE2, time_fmt=TIME_FMT, time_key="time")
    fp = g.FilterParser("log", [p]); fg = g.FilterGrep([GREP_RULE])
    r, o = g.FilterChain([fp, fg]).filter_dev(chunk)
    import ctypes
    host = (ctypes.c_uint8 * int(o.bytes))()
    L.flbgpu_memcpy_d2h(host, ctypes.c_void_p(o.data), int(o.bytes))
    ev = ob.tail_process(text, sec=7, nsec=8)[1]
    w1 = ob.FilterParser("log", [ob.Parser(APACHE2, time_fmt=TIME_FMT, time_key="time")]).filter(ev)[1]
    w2 = ob.Grep([GREP_RULE]).filter(w1)[1]
    assert bytes(host) == w2


def test_nul_texts_stop_where_they_say():
    texts = {label: text for label, text, _ in tc.group("nuls")}
    for z in (0, 1, 63, 64, 65, 127, 128, 16384):
        for tail in ("abc", "newline", "no newline"):
            t = texts["%d NULs, %s" % (z, tail)]
            assert len(t) - len(t.lstrip(b"\0")) == z and t[z:z + 1] == (b"\n" if tail == "newline" else b"a")
        assert tm.records(texts["%d NULs, no newline" % z]) == ([], z)                    # processed == lead
        assert tm.records(texts["%d NULs, newline" % z])[0][0] == b""                     # the NULs end right at the first newline
    sizes = sorted(len(t) for label, t, _ in tc.group("nuls") if label.startswith("all NUL"))
    assert sizes == [1, 64, 100, 16384] and all(tm.records(b"\0" * n) == ([], n) for n in sizes)

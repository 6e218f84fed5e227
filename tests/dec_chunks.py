"""Named cases for a parser's Decode_Field / Decode_Field_As rules on the device (csrc/dec_dev.inc, k_parser_dec in csrc/kernels.hip and
the sizing in run_parser_dev, csrc/flbgpu.cpp): every case sits on one edge of that code --

  scratch   the input that fills each scratch region of dec_dev.inc most per byte of the record (the parser's map A, the decoded map B,
            the text halves, the Decode_Field object O / the extra-keys buffer E, the merged map in region 0), at a record size where
            three times the record plus 4 KB (the first room a call gives a region) holds and at one where it does not; one large
            record among 399 small ones
  grid      1, 63, 64, 65 and 129 rows; fewer lanes than rows (a small FLBGPU_DEC_BUDGET_MB, and once the default budget with a row of
            1 MB): a lane's second row finds the slab of a longer first row whose decoded text continues its own
  widths    the msgpack headers the decoders write: strings of 31 / 32, 255 / 256, 65 535 / 65 536 bytes, merged maps of 15 / 16 / 17
            pairs, the regex parser's patched map header kept or made canonical, an extra-keys object without pairs
  rules     the rule bookkeeping: the 60 random rule lists of tests/test_decoders_oracle.py, MAX_DEC_KEYS keys and MAX_DEC_RULES rules,
            do_next chains of Decode_Field_As (the two text halves taking turns), a failing backend behind a success, a key twice in
            one map, values that are no strings, two keys with Decode_Field
  time      Format json's time lookup in the DECODED map: the time key among the extra keys, Time_Keep off, a text that does not parse,
            a time of 0 s 0 ns, a time the encoder refuses
  record    metadata, Reserve_Data / Preserve_Key over a body map of 65 keys, Key_Name as a record accessor
  paths     one chunk for FilterParser.filter, filter_dev and a [parser with decoders, grep] chain

A case is (records, Key_Name, parser list with its decoder rules, Reserve_Data, Preserve_Key) plus a predicate that says, from the chunk
and the ORACLE's answer alone, that the case is on its edge (tests/test_dec_chunks.py runs the predicates on the CPU and holds the
oracle's answers against the reference binary and tests/golden/dec_edges_kat.json; tests/test_dec_edges_gpu.py runs the cases on the
device).  The extra-keys buffer can never hold two objects (src/flb_parser_decoder.c:398-407 starts a new buffer at every key whose
rules can fill it), so "only the first object is merged" has no input; the nearest one, two keys with Decode_Field, is in `rules`."""
import itertools
import json
import random
import struct

import oracle_binding as ob
import synth

MODIFIED, NOTOUCH = 1, 2
MAX_DEC_KEYS = MAX_DEC_RULES = 8           # csrc/dev.hpp (tests/test_dec_chunks.py reads them from there and compares)
P_LOG = dict(regex=r"^<(?<log>.*)>$")
TFMT = "%Y-%m-%dT%H:%M:%S.%L"


# ------------------------------------------------------------------------------------------ msgpack, as far as the predicates need it
def mp_hdr(b, p):
    """(kind, count or payload bytes, header bytes) of the object at p"""
    c = b[p]
    if c <= 0x7f or c >= 0xe0 or c in (0xc0, 0xc2, 0xc3): return "x", 0, 1
    if c <= 0x8f: return "map", c & 15, 1
    if c <= 0x9f: return "arr", c & 15, 1
    if c <= 0xbf: return "str", c & 31, 1
    if c in (0xc4, 0xc5, 0xc6): w = 1 << (c - 0xc4); return "bin", int.from_bytes(b[p + 1:p + 1 + w], "big"), 1 + w
    if c in (0xc7, 0xc8, 0xc9): w = 1 << (c - 0xc7); return "ext", int.from_bytes(b[p + 1:p + 1 + w], "big") + 1, 1 + w
    if c in (0xca, 0xce, 0xd2): return "x", 0, 5
    if c in (0xcb, 0xcf, 0xd3): return "x", 0, 9
    if c in (0xcc, 0xd0): return "x", 0, 2
    if c in (0xcd, 0xd1): return "x", 0, 3
    if 0xd4 <= c <= 0xd8: return "ext", (1 << (c - 0xd4)) + 1, 1
    if c in (0xd9, 0xda, 0xdb): w = 1 << (c - 0xd9); return "str", int.from_bytes(b[p + 1:p + 1 + w], "big"), 1 + w
    if c in (0xdc, 0xdd): w = 2 << (c - 0xdc); return "arr", int.from_bytes(b[p + 1:p + 1 + w], "big"), 1 + w
    if c in (0xde, 0xdf): w = 2 << (c - 0xde); return "map", int.from_bytes(b[p + 1:p + 1 + w], "big"), 1 + w
    raise ValueError("0x%02x is no msgpack type byte" % c)


def mp_skip(b, p):
    kind, n, h = mp_hdr(b, p)
    p += h
    if kind in ("str", "bin", "ext"): return p + n
    if kind == "arr": n, kind = n, "seq"
    if kind == "map": n, kind = 2 * n, "seq"
    if kind == "seq":
        for _ in range(n):
            p = mp_skip(b, p)
    return p


def records(out):
    """[(start, body map offset, end)] of a chunk of [[time, metadata], body] events"""
    res, p = [], 0
    while p < len(out):
        body = mp_skip(out, p + 1)
        end = mp_skip(out, body)
        res.append((p, body, end))
        p = end
    return res


def pairs(b, p):
    """[(key bytes or None, value offset, value end)] of the map at p"""
    kind, n, h = mp_hdr(b, p)
    assert kind == "map", (kind, p)
    p += h
    res = []
    for _ in range(n):
        kk, kn, kh = mp_hdr(b, p)
        v = mp_skip(b, p)
        e = mp_skip(b, v)
        res.append((bytes(b[p + kh:p + kh + kn]) if kk == "str" else None, v, e))
        p = e
    return res


def keys(b, p):
    return [k for k, _, _ in pairs(b, p)]


# ------------------------------------------------------------------------------------------ the case
def rec(line, i=0, key="log", extra=(), meta=None):
    return synth.v2_record(1600000000 + i, i, synth.KV([(key.encode(), line)] + list(extra)), meta)


class Case:
    def __init__(self, name, recs, parsers, pred, key="log", reserve=False, preserve=False, env=None, notes=None):
        self.name, self.recs, self.parsers, self.pred, self.key = name, list(recs), list(parsers), pred, key
        self.reserve, self.preserve, self.env, self.notes = reserve, preserve, dict(env or {}), dict(notes or {})
        self.data = b"".join(self.recs)
        self._want = self._recs = None

    def want(self):
        """the oracle's (return code, output or None), computed once"""
        if self._want is None:
            self._want = ob.FilterParser(self.key, [ob.Parser(**p) for p in self.parsers], self.reserve, self.preserve).filter(self.data)
        return self._want

    def out(self):
        return self.want()[1] or b""

    def out_records(self):
        if self._recs is None:
            self._recs = records(self.out())
        return self._recs

    def out_pairs(self, r):
        return pairs(self.out(), self.out_records()[r][1])

    def max_row(self):
        return max(len(r) for r in self.recs)

    def first_room(self):
        """what a call first gives each scratch region (the whole room the parent commit had)"""
        return 3 * self.max_row() + 4096

    def largest_map(self):
        return max(e - b for _, b, e in self.out_records())

    def check(self):
        assert self.want()[0] == MODIFIED, (self.name, self.want()[0])
        assert self.pred(self), self.name


def with_decs(p, decs):
    return dict(p, decoders=list(decs))


# ------------------------------------------------------------------------------------------ scratch
RULESETS = {
    "field_json": [(False, "json", "log")],                                           # O, E: 2.25; region 0: the string + E = 3.25
    "as_json": [(True, "json", "log")],                                               # a text half, B: 2.25
    "field_json+as_json": [(False, "json", "log", "do_next"), (True, "json", "log")],  # B 2.25 + E 2.25: region 0 holds 4.5
    "as_escaped+field_json": [(True, "escaped", "log", "do_next"), (False, "json", "log")],   # both text halves; region 0: 1 + 2.25
}
WORST_JSON = b"1e5,"                       # 4 bytes of text, a 9-byte double
WORST_LOGFMT = b"a "                       # Types a:float: a bare key is 2 bytes of text, "a" + a 9-byte double
WORST_LTSV = b"a:\t"                       # 3 bytes of text, the same 11 bytes


def json_value(n, escaped=False):
    v = b'{"a":[' + WORST_JSON * n + b"1e5]}"
    return v.replace(b'"', b'\\"') if escaped else v


def _scratch_pred(ratio, past):
    def pred(c):
        big = c.largest_map()
        return abs(big / c.max_row() - ratio) < c.notes["slack"] and (big > c.first_room()) == past
    return pred


def scratch_cases():
    """every worst case at a record of 1 KB or less and at the size where 3 x record + 4 KB stops holding (where its ratio passes 3)"""
    out = []
    small = lambda i: rec(b'<{"i":%d}>' % i, i)

    def add(name, parsers, line_of, sizes, ratio):
        for n, past in sizes:
            line = line_of(n)
            recs = [small(0), rec(line, 1), small(2)]
            c = Case("scratch/%s/%d" % (name, n), recs, parsers, _scratch_pred(ratio, past), notes=dict(slack=0.35 if len(line) < 1024 else 0.06, past=past, big=1))
            assert (len(line) <= 1024) == (n == sizes[0][0]), (name, n, len(line))
            out.append(c)
    for rs, big, ratio in (("field_json", 5000, 3.25), ("as_json", 5000, 2.25), ("field_json+as_json", 1000, 4.5), ("as_escaped+field_json", 5000, 3.25)):
        add(rs, [with_decs(P_LOG, RULESETS[rs])], lambda n, rs=rs: b"<" + json_value(n, rs.startswith("as_escaped")) + b">",
            [(200, False), (big, ratio > 3)], ratio)
    # map A alone: Format json's own walk of the record text, and the kv parsers' Types
    add("json_parser", [dict(format="json", decoders=[(True, "escaped", "log")])], lambda n: b'{"log":"x\\\\n","a":[' + WORST_JSON * n + b"1e5]}",
        [(200, False), (5000, False)], 2.25)
    add("logfmt_float", [dict(format="logfmt", types="a:float", decoders=[(True, "escaped", "log")])], lambda n: b"log=x\\n " + WORST_LOGFMT * n + b"z=1",
        [(500, False), (2000, True)], 5.5)
    add("ltsv_float", [dict(format="ltsv", types="a:float", decoders=[(True, "escaped", "log")])], lambda n: b"log:x\\n\t" + WORST_LTSV * n + b"z:1",
        [(330, False), (6800, True)], 11 / 3)
    return out


def one_large():
    """400 records, one of 4 KB under the two-rule set; around it small ones, every third unparsed, every third won by a parser
    without decoders (the longest record of the CHUNK sizes the scratch, whoever wins it)"""
    parsers = [with_decs(P_LOG, RULESETS["field_json+as_json"]), dict(regex=r"^\[(?<m>.*)\]$")]
    recs = []
    for i in range(400):
        line = (b'<{"i":%d,"s":"%s"}>' % (i, b"s" * (i % 40)), b"[plain %d]" % i, b"nobody parses %d" % i)[i % 3]
        recs.append(rec(line, i))
    recs[201] = rec(b"<" + json_value(1000) + b">", 201)

    def pred(c):
        o = c.out_records()
        big = [r for r, (_, b, e) in enumerate(o) if e - b > c.first_room()]
        return len(o) == 400 and big == [201] and keys(c.out(), o[1][1]) == [b"m"] and keys(c.out(), o[2][1]) == [b"log"] and keys(c.out(), o[0][1]) == [b"log", b"i", b"s"]
    return Case("scratch/one_large", recs, parsers, pred, notes=dict(past=True, big=201))


def growth(pieces, line_of, parser, reps=(8, 14)):
    """bytes the oracle's output record grows by per byte of `piece`, for every piece: two records per piece (the piece reps[0] and
    reps[1] times), one filter call over all of them"""
    recs = []
    for i, t in enumerate(pieces):
        recs += [rec(line_of(t, reps[0]), 2 * i), rec(line_of(t, reps[1]), 2 * i + 1)]
    ret, out = ob.FilterParser("log", [ob.Parser(**parser)]).filter(b"".join(recs))
    assert ret == MODIFIED
    pos, p = [], 0
    for i in range(len(recs)):                     # (every record starts with its own time: no need to walk 100 000 maps in Python)
        q = out.find(b"\x92\x92\xd7\x00" + struct.pack(">II", 1600000000 + i, i), p)
        assert q >= 0, i
        pos.append(q); p = q + 12
    pos.append(len(out))
    return [(pos[2 * i + 2] - pos[2 * i + 1] - (pos[2 * i + 1] - pos[2 * i])) / float((reps[1] - reps[0]) * len(t)) for i, t in enumerate(pieces)]


JSON_ALPHABET = b'015-.eE+"a[]{}:,'


def json_tokens():
    """every text of 1 .. 4 characters of the alphabet (numbers, strings, containers, separators, garbage), true and null, each followed
    by the comma that makes it an array element"""
    toks = [bytes(x) for k in (1, 2, 3, 4) for x in itertools.product(JSON_ALPHABET, repeat=k)] + [b"true", b"null"]
    return [t + b"," for t in toks]


def json_growth(tokens, ruleset):
    esc = ruleset.startswith("as_escaped")
    return growth(tokens, lambda t, k: b"<" + (b'{\\"a\\":[' if esc else b'{"a":[') + t.replace(b'"', b'\\"' if esc else b'"') * k + b"1]}>",
                  with_decs(P_LOG, RULESETS[ruleset]))


def kv_pieces(fmt):
    vals = [b""] + [bytes(x) for k in (1, 2, 3) for x in itertools.product(b"019-+.e", repeat=k)]
    if fmt == "logfmt":
        return [b"a=" + v + b" " for v in vals] + [b"a "]
    return [b"a:" + v + b"\t" for v in vals]


def kv_growth(pieces, fmt):
    head, tail = (b"log=x ", b"z=1") if fmt == "logfmt" else (b"log:x\t", b"z:1")
    return growth(pieces, lambda t, k: head + t * k + tail, dict(format=fmt, types="a:float", decoders=[(True, "escaped", "log")]), reps=(4, 12))


# ------------------------------------------------------------------------------------------ grid
DOCKER = [(True, "escaped", "log", "do_next"), (False, "json", "log")]


def _esc(obj):
    return json.dumps(obj, separators=(",", ":")).encode().replace(b'"', b'\\"')


def grid_rows(n):
    recs = [rec(b"<" + _esc({"i": i, "s": "r" * (i % 29)}) + b">", i) for i in range(n)]
    return Case("grid/rows/%d" % n, recs, [with_decs(P_LOG, DOCKER)],
                lambda c: len(c.out_records()) == n and all(keys(c.out(), b) == [b"log", b"i", b"s"] for _, b, _ in c.out_records()))


def _trip_pred(c):
    """rows r + 64 and r + 128 hold the first bytes of row r's text: a broken text that the bytes row r left behind it would complete
    (the JSON backend must fail: the row keeps `log` alone), and a complete one that ends earlier"""
    o, ok = c.out_records(), True
    for r in c.notes["long"]:
        ok &= keys(c.out(), o[r][1]) == [b"log", b"a", b"b"] and len(c.recs[r]) > 0.9 * c.max_row()
        for d in (64, 128):
            if r + d + 1 >= len(c.recs):
                continue
            ok &= keys(c.out(), o[r + d][1]) == [b"log"] and keys(c.out(), o[r + d + 1][1]) == [b"log", b"a"]
            text = lambda q: c.recs[q][c.recs[q].index(b"<") + 1:c.recs[q].rindex(b">")]
            ok &= text(r).startswith(text(r + d)) and text(r).startswith(text(r + d + 1)[:-3])
    return ok


def second_trip(name, n, big, env, long_rows=(0, 3)):
    """row r: the Decode_Field_As escaped text in one half, its JSON object in the other, extra keys; rows r + 64 / r + 128 (whichever
    the lanes come to): the same text cut short inside the string, and cut short and closed"""
    full = lambda k: b'<{\\"a\\":\\"' + b"x" * k + b'\\",\\"b\\":1}>'
    recs = [rec(b"<" + _esc({"i": i}) + b">", i) for i in range(n)]
    for r in long_rows:
        recs[r] = rec(full(big - 64 * r), r)
        for d in (64, 128):
            if r + d + 1 < n:
                recs[r + d] = rec(b'<{\\"a\\":\\"' + b"x" * 40 + b">", r + d)
                recs[r + d + 1] = rec(b'<{\\"a\\":\\"' + b"x" * 40 + b'\\"}>', r + d + 1)
    return Case("grid/second_trip/%s" % name, recs, [with_decs(P_LOG, DOCKER)], _trip_pred, env=env, notes=dict(long=list(long_rows), trip=True))


def grid_cases():
    out = [grid_rows(n) for n in (1, 63, 64, 65, 129)]
    # 200 rows, the longest 4 KB: 256 lanes x 6 regions x 16 KB are 25 MB -- a budget of 16 MB halves the lanes once, one of 8 MB twice
    out.append(second_trip("budget16", 200, 4000, {"FLBGPU_DEC_BUDGET_MB": "16"}))
    out.append(second_trip("budget8", 200, 4000, {"FLBGPU_DEC_BUDGET_MB": "8"}))
    # the default budget of 2 GiB: 130 rows, one of 1 MB (6 regions x 3 MB x 128 lanes pass 2 GiB: 64 lanes, 1.2 GB of scratch)
    out.append(second_trip("default", 130, 1000000, {}, long_rows=(0,)))
    return out


# ------------------------------------------------------------------------------------------ header widths
STR_EDGES = (31, 32, 255, 256, 65535, 65536)


def str_widths(backend):
    """decoded strings of exactly the edge lengths: from a text of that length, and from a text one escape longer"""
    recs, want = [], []
    q = b"'" if backend == "mysql_quoted" else b""                 # (decode_mysql_quoted only touches a quoted text)
    for L in STR_EDGES:
        recs.append(rec(b"<" + q + b"s" * L + q + b">", len(recs))); want.append(L)
        recs.append(rec(b"<" + q + b"s" * (L - 1) + b"\\n" + q + b">", len(recs))); want.append(L)

    def pred(c):
        got = []
        for r in range(len(recs)):
            (k, v, e), = c.out_pairs(r)
            kind, n, h = mp_hdr(c.out(), v)
            got.append((kind, n, h))
        return got == [("str", L, 1 if L < 32 else 2 if L < 256 else 3 if L < 65536 else 5) for L in want]
    return Case("widths/str/%s" % backend, recs, [with_decs(P_LOG, [(True, backend, "log")])], pred)


MERGE_COUNTS = ((14, 1), (1, 14), (15, 1), (1, 15), (8, 8), (16, 1), (1, 16), (15, 0), (16, 0))


def merged_counts():
    """ltsv: nb pairs in the record, ne in the object Decode_Field json finds in `log`; the merged map has nb + ne"""
    recs = []
    for i, (nb, ne) in enumerate(MERGE_COUNTS):
        obj = b"{" + b",".join(b'"e%d":%d' % (q, q) for q in range(ne)) + b"}"
        recs.append(rec(b"\t".join([b"log:" + obj] + [b"k%d:v" % q for q in range(nb - 1)]), i))

    def pred(c):
        ok = True
        for r, (nb, ne) in enumerate(MERGE_COUNTS):
            _, b, _ = c.out_records()[r]
            kind, n, h = mp_hdr(c.out(), b)
            ok &= kind == "map" and n == nb + ne and h == (1 if nb + ne < 16 else 3)
        return ok
    return Case("widths/merged_counts", recs, [dict(format="ltsv", decoders=[(False, "json", "log")])], pred)


NGROUPS = 17
P_GROUPS = dict(regex="^" + ",".join("(?<g%d>[^,]*)" % q for q in range(NGROUPS)) + "$", skip_empty=True)


def patched_header(decoded):
    """17 named groups, Skip_Empty_Values leaves 3 and 16: the regex parser patches the count into its map16 header.  No key with a
    decoder in the map: the map goes out as the parser packed it (de 00 03); a key with one: flb_parser_decoder_do packs a new map (83)"""
    recs = [rec(b",".join(b"v%d" % q if q in (0, 5, 16) else b"" for q in range(NGROUPS)), 0),
            rec(b",".join(b"" if q == 7 else b"w%d" % q for q in range(NGROUPS)), 1)]
    decs = [(True, "escaped", "g5")] if decoded else [(True, "escaped", "nokey")]

    def pred(c):
        o = c.out()
        (_, b0, _), (_, b1, _) = c.out_records()
        return o[b0:b0 + 3] == (b"\x83\xa2g" if decoded else b"\xde\x00\x03") and o[b1:b1 + 3] == b"\xde\x00\x10"
    return Case("widths/patched_header/%s" % ("canonical" if decoded else "kept"), recs, [with_decs(P_GROUPS, decs)], pred)


def empty_extra():
    recs = [rec(b"<{}>", 0), rec(b"< {} >", 1), rec(b'<{"a":{}}>', 2)]
    return Case("widths/empty_extra", recs, [with_decs(P_LOG, RULESETS["field_json"])],
                lambda c: [keys(c.out(), b) for _, b, _ in c.out_records()] == [[b"log"], [b"log"], [b"log", b"a"]])


def width_cases():
    return [str_widths("escaped"), str_widths("escaped_utf8"), str_widths("mysql_quoted"), merged_counts(), patched_header(False), patched_header(True),
            empty_extra()]


# ------------------------------------------------------------------------------------------ rule bookkeeping
def random_rule_sets():
    """the 60 configurations of tests/test_decoders_oracle.py::test_random_decoder_sets_against_the_real_parser_decoder, same seed"""
    import test_decoders_oracle as T
    data = T._chunks()
    rng = random.Random(77)
    out = []
    for q in range(60):
        rules = []
        for _ in range(rng.randint(1, 4)):
            r = [rng.random() < 0.6, rng.choice(["json", "escaped", "escaped_utf8", "mysql_quoted"]), rng.choice(["log", "log", "other", "nokey", "n"])]
            a = rng.choice([None, None, "try_next", "do_next", "bogus"])
            if a:
                r.append(a)
            rules.append(tuple(r))
        pa = rng.choice(T.PARSERS)
        rp = rng.random() < 0.5
        c = Case("rules/random/%d" % q, [data], [with_decs(pa, rules)], lambda c: True, key="msg", reserve=rp, preserve=rp, notes=dict(bogus=any(len(r) > 3 and r[3] == "bogus" for r in rules)))
        out.append(c)
    return out


def _chain_value(depth):
    """a text that needs `depth` rounds of `escaped` to lose its backslashes: each round halves the runs"""
    v = b'{"k":"v"}'
    for _ in range(depth):
        v = v.replace(b"\\", b"\\\\").replace(b'"', b'\\"')
    return v


def rule_cases():
    out = random_rule_sets()
    # MAX_DEC_KEYS keys / MAX_DEC_RULES rules on one key, all of them at work
    many = [(True, "escaped", "k%d" % q) for q in range(MAX_DEC_KEYS)]
    line = b"\t".join(b"k%d:a\\tb%d" % (q, q) for q in range(MAX_DEC_KEYS + 1))
    out.append(Case("rules/max_keys", [rec(line, 0)], [dict(format="ltsv", decoders=many)],
                    lambda c: [c.out()[v:e] for _, v, e in c.out_pairs(0)] == [synth.mp(b"a\tb%d" % q) for q in range(MAX_DEC_KEYS)] + [synth.mp(b"a\\tb%d" % MAX_DEC_KEYS)],
                    notes=dict(over=many + [(True, "escaped", "k%d" % MAX_DEC_KEYS)])))
    deep = [(True, "json", "log", "try_next")] * (MAX_DEC_RULES - 1) + [(True, "escaped", "log")]
    out.append(Case("rules/max_rules", [rec(b"<a\\nb>", 0), rec(b'<{"a":1}>', 1)], [with_decs(P_LOG, deep)],
                    lambda c: c.out()[c.out_pairs(0)[0][1]:c.out_pairs(0)[0][2]] == synth.mp(b"a\nb") and mp_hdr(c.out(), c.out_pairs(1)[0][1])[0] == "map",
                    notes=dict(over=deep + [(True, "escaped", "log")])))
    # do_next chains of Decode_Field_As: every round reads the half the last one wrote
    for depth in (3, 4):
        chain = [(True, "escaped", "log", "do_next")] * depth + [(False, "json", "log")]
        recs = [rec(b"<" + _chain_value(depth) + b">", 0), rec(b"<" + _chain_value(depth - 1) + b">", 1), rec(b"<" + _chain_value(depth) * 30 + b">", 2)]
        out.append(Case("rules/as_chain/%d" % depth, recs, [with_decs(P_LOG, chain)],
                        lambda c: keys(c.out(), c.out_records()[0][1]) == [b"log", b"k"] and c.out()[c.out_pairs(0)[0][1]:c.out_pairs(0)[0][2]] == synth.mp(b'{"k":"v"}')
                        and keys(c.out(), c.out_records()[1][1]) == [b"log", b"k"] and keys(c.out(), c.out_records()[2][1]) == [b"log"]))
    # a failing backend behind a success: with try_next the rules go on, without the key is done
    for act in ("try_next", None):
        rules = [(True, "escaped", "log", "do_next"), (True, "json", "log") + ((act,) if act else ()), (False, "json", "log", "do_next"), (True, "mysql_quoted", "log")]
        recs = [rec(b"<'not\\tjson'>", 0), rec(b'<{\\"a\\":1}>', 1), rec(b'<{"a":1} {"b":2}>', 2)]
        out.append(Case("rules/fail_after_success/%s" % (act or "stop"), recs, [with_decs(P_LOG, rules)],
                        lambda c, act=act: c.out()[c.out_pairs(0)[0][1]:c.out_pairs(0)[0][2]] == synth.mp(b"not\tjson" if act else b"'not\tjson'")
                        and mp_hdr(c.out(), c.out_pairs(1)[0][1])[0] == "map" and keys(c.out(), c.out_records()[2][1]) == [b"log"]))
    # a key twice in one map: each occurrence is decoded, the extra keys are those of the LAST one
    out.append(Case("rules/key_twice", [rec(b'log="{\\"a\\":1}" mid=m log="{\\"b\\":2}"', 0), rec(b'log="{\\"a\\":1}" log=plain', 1)],
                    [dict(format="logfmt", decoders=RULESETS["field_json"])],
                    lambda c: keys(c.out(), c.out_records()[0][1]) == [b"log", b"mid", b"log", b"b"] and keys(c.out(), c.out_records()[1][1]) == [b"log", b"log"]))
    # a decoder key whose value is no string, and one in front of / behind a pair that is none
    js = [dict(format="json", decoders=[(False, "json", "log"), (True, "escaped", "other")])]
    lines = [b'{"log": 5, "other": "a\\\\tb"}', b'{"log": {"a": 1}, "other": "a\\\\tb"}', b'{"other": "a\\\\tb", "n": [1, 2], "log": "{\\"x\\": 1}"}',
             b'{"log": "{\\"x\\": 1}", "n": 7, "other": "a\\\\tb", "log2": null}', b'{"n": 1, "m": 2}']
    out.append(Case("rules/not_a_string", [rec(l, i) for i, l in enumerate(lines)], js,
                    lambda c: [keys(c.out(), b) for _, b, _ in c.out_records()] == [[b"log", b"other"], [b"log", b"other"], [b"other", b"n", b"log", b"x"],
                                                                                    [b"log", b"n", b"other", b"log2", b"x"], [b"n", b"m"]]))
    # two keys with Decode_Field: the buffer of the earlier key is dropped, also when the later key's backend fails
    two = [dict(regex=r"^<(?<log>.*)> <(?<other>.*)>$", decoders=[(False, "json", "log"), (False, "json", "other")])]
    recs = [rec(b'<{"a":1}> <{"b":2}>', 0), rec(b'<{"a":1}> <plain>', 1), rec(b'<plain> <{"b":2}>', 2)]
    out.append(Case("rules/two_field_keys", recs, two,
                    lambda c: [keys(c.out(), b) for _, b, _ in c.out_records()] == [[b"log", b"other", b"b"], [b"log", b"other"], [b"log", b"other", b"b"]]))
    return out


# ------------------------------------------------------------------------------------------ Format json's second look at the time
def time_cases():
    out = []

    def line(t, extra=b""):
        return json.dumps({"log": json.dumps({"z": 9, "time": t, "y": "after"}), "n": 1}).encode()
    for keep in (True, False):
        p = [dict(format="json", time_key="time", time_fmt=TFMT, time_keep=keep, decoders=[(False, "json", "log")])]
        recs = [rec(line("2020-01-02T03:04:05.5"), 0), rec(line("not a time"), 1), rec(line("1970-01-01T00:00:00.0"), 2), rec(line("1960-01-01T00:00:00.5"), 3),
                rec(line(5), 4), rec(line("2021-05-06T07:08:09.25"), 5)]

        def pred(c, keep=keep):
            o, r = c.out(), c.out_records()
            found = [b"log", b"n", b"z"] + ([b"time"] if keep else []) + [b"y"]
            whole = [b"log", b"n", b"z", b"time", b"y"]
            ts = lambda q: struct.unpack(">II", o[r[q][0] + 4:r[q][0] + 12])
            return (len(r) == 5 and ts(0) == (1577934245, 500000000) and keys(o, r[0][1]) == found          # the refused time: no record
                    and ts(1) == (1600000001, 1) and keys(o, r[1][1]) == whole                               # does not parse: kept as it is
                    and ts(2) == (1600000002, 2) and keys(o, r[2][1]) == found                               # 0 s 0 ns: the event's own time stays
                    and ts(3) == (1600000004, 4) and keys(o, r[3][1]) == whole                               # no string
                    and ts(4) == (1620284889, 250000000))
        out.append(Case("time/extra_keys/keep%d" % keep, recs, p, pred))
    return out


# ------------------------------------------------------------------------------------------ around the record
def record_cases():
    out = []
    wide = [(b"f%02d" % q, b"v%d" % q if q % 5 else None) for q in range(64)]
    body = lambda i: [(b"first", i)] + wide[:31] + [(b"log", b'<{\\"a\\":%d}>' % i)] + wide[31:]
    recs = [synth.v2_record(1600000000 + i, i, synth.KV(body(i)), synth.KV([(b"meta", b"m%d" % i), (b"deep", [1, synth.KV([(b"x", None)])])]) if i % 2 else None) for i in range(70)]
    for reserve, preserve in ((True, False), (True, True), (False, True), (False, False)):
        def pred(c, reserve=reserve, preserve=preserve):
            o = c.out()
            ks = keys(o, c.out_records()[1][1])
            want = [b"log", b"a"] + ([k for k, _ in body(1) if k != b"log" or preserve] if reserve else [b"log"] if preserve else [])
            s, b, _ = c.out_records()[1]
            return len(body(1)) == 66 and ks == want and mp_hdr(o, s + 12)[:2] == ("map", 2) and mp_hdr(o, c.out_records()[0][0] + 12)[:2] == ("map", 0)
        out.append(Case("record/meta_reserve%d_preserve%d" % (reserve, preserve), recs, [with_decs(P_LOG, DOCKER)], pred, reserve=reserve, preserve=preserve))
    # Key_Name as a record accessor
    recs = [synth.v2_record(1600000000 + i, i, synth.KV([(b"outer", synth.KV([(b"pad", i), (b"log", b'<{\\"a\\":%d}>' % i)])), (b"keep", i)])) for i in range(70)]
    for reserve in (False, True):
        out.append(Case("record/accessor/reserve%d" % reserve, recs, [with_decs(P_LOG, DOCKER)],
                        lambda c, reserve=reserve: keys(c.out(), c.out_records()[69][1]) == [b"log", b"a"] + ([b"outer", b"keep"] if reserve else []),
                        key="$outer['log']", reserve=reserve, preserve=reserve))
    return out


# ------------------------------------------------------------------------------------------ call paths
GREP = [("regex", "level ^(warn|error)$")]


def paths_case():
    """130 records: decoded ones (their `level` comes out of the decoded object: the grep behind the parser sees it), ones a parser
    without decoders wins, unparsed ones"""
    parsers = [with_decs(P_LOG, DOCKER), dict(regex=r"^\[(?<level>[a-z]+)\] (?<m>.*)$")]
    recs = []
    for i in range(130):
        lv = ("info", "warn", "error", "debug")[i % 4]
        line = (b"<" + _esc({"level": lv, "i": i, "msg": "m" * (i % 50)}) + b">", b"[%s] plain %d" % (lv.encode(), i), b"nobody parses %d" % i)[i % 3]
        recs.append(rec(line, i))

    def pred(c):
        ret, kept = ob.Grep(GREP).filter(c.out())
        n = ob.count_records(kept)
        return ret == MODIFIED and 0 < n < 130 and any(keys(c.out(), b) == [b"log", b"level", b"i", b"msg"] for _, b, _ in c.out_records())
    return Case("paths/mixed", recs, parsers, pred)


GROUPS = {
    "scratch": lambda: scratch_cases() + [one_large()],
    "grid": grid_cases,
    "widths": width_cases,
    "rules": rule_cases,
    "time": time_cases,
    "record": record_cases,
    "paths": lambda: [paths_case()],
}
_cache = {}


def cases(group):
    """the cases of one group, built once and shared (with their oracle answers) by every test that needs them"""
    if group not in _cache:
        _cache[group] = GROUPS[group]()
    return _cache[group]


def all_cases():
    return [c for g in GROUPS for c in cases(g)]

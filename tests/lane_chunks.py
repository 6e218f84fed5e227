"""Builders and case tables for the one-pass lane kernels' edge suite (csrc/jlane_kernels.inc, glane_kernels.inc, l2mlane_kernels.inc,
lane_dev.inc, lookback.inc).  tests/test_lane_chunks.py proves on the CPU that every family reaches what it claims;
tests/test_lane_edges_gpu.py runs them on the device.

Two things let a defect of these kernels hide, and the tables answer both:
  * every row has a second answer (a JSON row the pass leaves is written by k_json_rows / k_json_generic, a record the lean walk
    declines by decode_event / grep_decide / l2m_record), so every JSON case carries `taken` -- WRITTEN BY HAND from the conditions
    the kernel states (CONDS below), never computed by calling the library -- and every record carries `plain`: the shape the lean
    walk takes (plain_event() restates it from the msgpack bytes);
  * the geometry comes from the chunk's mean row length (json.cpp json_run, flbgpu.cpp lane_geometry, l2m.cpp): the functions
    *_geometry restate the host's arithmetic so that a builder can land in a given regime and say where its rows stand in a tile."""
import struct
import ndjson_synth as ns
from synth import v2_record, legacy_record, mp, Raw, KV, ext_ts

TEXT = 15872                    # text bytes of a wave at most: JL_TEXT, GL_TEXT_MAX, L2L_TEXT_MAX
COPY_LENS = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 287, 288, 289, 513]      # byte path, one lane, the overlapping last step, the second round of eight lanes
TS = (0x01020304, 0x05060708)   # a timestamp whose eight bytes differ


# ------------------------------------------------------------------------------------------------ geometry, as the host computes it
def json_geometry(nbytes, n):
    """rows per tile and the wave's text bytes (json.cpp:65-72)"""
    avg = nbytes // n + 1
    return max(1, min(64, (TEXT - 16) * 92 // 100 // avg)), TEXT


def _lane_geometry(nbytes, n, num, den):
    avg = nbytes // n + 1
    R, cap = 64, (64 * avg * num // den + 512 + 15) & ~15
    if cap > TEXT:
        R, cap = (TEXT - 16) * 92 // 100 // avg, TEXT
    return max(1, min(64, R)), max(cap, 2048)


def grep_geometry(nbytes, n):
    """flbgpu.cpp lane_geometry for a chunk of fewer than 65536 records (a larger one asks k_tile_max)"""
    assert n < 65536
    return _lane_geometry(nbytes, n, 3, 2)


def l2m_geometry(nbytes, n):
    """l2m.cpp:330-336"""
    return _lane_geometry(nbytes, n, 5, 4)


def fits(rows, geometry):
    """per row: does it stand in its wave's LDS (`have` of the three kernels: the row's end, counted from the 16-byte aligned address
    at or in front of its tile's first row, within the wave's text bytes); the chunk itself is 16-byte aligned"""
    n = len(rows)
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r))
    R, cap = geometry(off[-1], n)
    out = []
    for i in range(n):
        g0 = off[i - i % R]
        out.append(off[i + 1] - (g0 - (g0 & 15)) <= cap)
    return out, R, cap


def xs(n, salt=0):
    """n printable bytes that do not repeat with a period a copy loop has (16, 4, 32)"""
    return bytes(97 + (i * 7 + i // 26 + salt) % 26 for i in range(n))


# ------------------------------------------------------------------------------------------------ JSON: the case table (family B)
# the conditions under which k_json_lane leaves a row to the second leg; "fit" belongs to the chunk builders of family A
CONDS = ("fit", "one_object", "escape", "control", "depth", "exact_decimal", "primitive_longer", "string_moves_up", "header16_slack")
ESCAPES = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t"]
STR_LENS = [0, 1, 3, 4, 5, 14, 15, 16, 17, 19, 20, 31, 32, 33, 255, 256, 257, 300]
INTS = [0, 127, 128, 255, 256, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 2 ** 64, -1, -32, -33, -128, -129,
        -32768, -32769, -2 ** 31, -2 ** 31 - 1, -2 ** 63, -2 ** 63 - 1]
# 2^53 + 1 and a little: the first nineteen digits stand exactly half way between two doubles and the digits behind them decide
HARD_DECIMAL = b"9007199254740993.000000000000000000000001"


class JCase:
    def __init__(self, name, row, taken, cond, at_end):
        self.name, self.row, self.taken, self.cond, self.at_end = name, row, taken, cond, at_end

    def __repr__(self):
        return "JCase(%s)" % self.name


def _J(out, name, text, taken=True, cond=None, nl=b"\n", at_end=False):
    assert (cond is None) == taken and (cond is None or cond in CONDS), name
    out.append(JCase(name, text + nl, taken, cond, at_end))


def json_cases():
    """family name -> [JCase].  `taken` is written by hand from the kernel's stated conditions: the positions in the comments count
    `out` (msgpack bytes written) and `in` (text bytes read) from the row's first byte"""
    F = {}
    # ---- B.1 strings
    c = F["string_values"] = []
    for L in STR_LENS:
        _J(c, "value%d" % L, b'{"k":"' + xs(L) + b'"}')                 # L > 255: out 3 + 3 = in 6, the body stays where it is
        _J(c, "value%d_blank" % L, b'{"k": "' + xs(L) + b'"}')
    c = F["string_keys"] = []
    for L in STR_LENS:
        _J(c, "key%d" % L, b'{"a":1,"' + xs(L) + b'":1}')
    c = F["first_key"] = []
    for L in (30, 31, 32, 33):
        # behind `{"` the body stands at in 2 and out is 1: a two-byte header would put it at 3
        _J(c, "first%d" % L, b'{"' + xs(L) + b'":1}', L <= 31, None if L <= 31 else "string_moves_up")
        _J(c, "first%d_blank" % L, b'{ "' + xs(L) + b'":1}')
    _J(c, "first255_blank", b'{ "' + xs(255) + b'":1}')
    _J(c, "first256_blank", b'{ "' + xs(256) + b'":1}', False, "string_moves_up")       # three bytes of header, two of room
    _J(c, "first256_two_blanks", b'{  "' + xs(256) + b'":1}')
    c = F["escapes"] = []
    for e in ESCAPES:
        for pos in (0, 3, 4, 15, 16, 19):
            body = xs(20)
            _J(c, "esc%s@%d" % (e.decode(), pos), b'{"k":"' + body[:pos] + e + body[pos + 1:] + b'"}')
    _J(c, "run33to31", b'{"k":"\\n\\n' + xs(29) + b'"}')
    _J(c, "run34to32", b'{"k":"\\n\\n' + xs(30) + b'"}')
    _J(c, "run257to255", b'{"k":"' + xs(100) + b'\\t\\t' + xs(153) + b'"}')
    _J(c, "run258to256", b'{"k":"' + xs(100) + b'\\t\\t' + xs(154) + b'"}')
    _J(c, "quote_16th", b'{"k":"' + xs(14) + b'\\"' + xs(5) + b'"}')
    _J(c, "quote_17th", b'{"k":"' + xs(15) + b'\\"' + xs(5) + b'"}')
    _J(c, "backslash_quote_last", b'{"k":"' + xs(18) + b'\\\\"}')
    c = F["utf8"] = []
    for ch, offs in (("é", (3, 15)), ("中", (2, 3, 14, 15)), ("😀", (1, 2, 3, 13, 14, 15))):
        for o in offs:
            _J(c, "utf8_%d@%d" % (len(ch.encode()), o), b'{"k":"' + xs(o) + ch.encode() + xs(6) + b'"}')
    c = F["odd_strings"] = []
    _J(c, "u0041", b'{"k":"\\u0041"}', False, "escape")
    _J(c, "backslash_x", b'{"k":"\\x41"}', False, "escape")
    _J(c, "raw01", b'{"k":"a\x01b"}', False, "control")
    _J(c, "raw01_key", b'{"a\x01b":1}', False, "control")
    _J(c, "raw7f", b'{"k":"a\x7fb"}')
    _J(c, "unclosed", b'{"a":"abc', False, "one_object")                  # its own newline ends the scan
    _J(c, "unclosed_no_newline", b'{"a":"abc', False, "one_object", nl=b"")    # the next quote is the following row's
    _J(c, "unclosed_long_no_newline", b'{"a":"' + xs(40), False, "one_object", nl=b"")
    # ---- B.2 numbers
    c = F["numbers_alone"] = []                                          # behind `{"a":` out is 3 and in is 5
    for v in INTS:
        _J(c, "int%d" % v, b'{"a":%d}' % v)
    _J(c, "minus0", b'{"a":-0}')
    for t in (b"0.0", b"1e1", b"1E+1", b"1.5"):
        _J(c, "real_" + t.decode(), b'{"a":' + t + b'}', False, "primitive_longer")     # nine bytes where at most six were read
    _J(c, "real_7chars", b'{"a":1.50000}')                               # out 3 + 9 = 12 = the number's end
    _J(c, "real_6chars", b'{"a":1.5000}', False, "primitive_longer")
    _J(c, "hard_decimal", b'{"a":' + HARD_DECIMAL + b'}', False, "exact_decimal")
    c = F["numbers_slack"] = []                                          # behind `{"s":"<20>","a":` out is 26 and in is 32
    pre = b'{"s":"' + xs(20) + b'","a":'
    for v in INTS:
        _J(c, "int%d" % v, pre + b"%d}" % v)
    for t in (b"-0", b"0.0", b"1e1", b"1E+1", b"1.5"):
        _J(c, "num_" + t.decode(), pre + t + b"}")
    _J(c, "hard_decimal", pre + HARD_DECIMAL + b"}", False, "exact_decimal")
    c = F["real_arrays"] = []
    for k in (1, 2, 3, 4):
        # `[` leaves six bytes of slack, a `1e1` takes six and its comma gives one back
        _J(c, "reals%d" % k, pre + b"[" + b",".join([b"1e1"] * k) + b"]}", k == 1, None if k == 1 else "primitive_longer")
        # ten blanks more: sixteen; 16 - 6 + 1 - 6 + 1 - 6 + 1 = 1 in front of the fourth
        _J(c, "reals%d_blanks" % k, pre + b" " * 10 + b"[" + b",".join([b"1e1"] * k) + b"]}", k <= 3, None if k <= 3 else "primitive_longer")
    c = F["bad_literals"] = []
    for t in (b"01", b"-", b"1.", b"tru", b"nul", b"falsE"):
        _J(c, "bad_" + t.decode(), b'{"a":' + t + b'}', False, "one_object")
    for t in (b"true", b"false", b"null"):
        _J(c, "ends_" + t.decode(), b'{"a":' + t, False, "one_object", nl=b"", at_end=True)      # the literal is the last bytes of the data
    # ---- B.3 containers
    c = F["containers"] = []
    for n in (0, 1, 15, 16, 17, 40):
        _J(c, "root_obj%d" % n, b"{" + b",".join([b'"":1'] * n) + b"}")
        _J(c, "root_obj%d_long" % n, b"{" + b",".join(b'"key%02d":"' % i + xs(20, i) + b'"' for i in range(n)) + b"}")
        _J(c, "obj%d" % n, b'{"o":{' + b",".join([b'"":1'] * n) + b"}}")
        _J(c, "obj%d_long" % n, b'{"o":{' + b",".join(b'"key%02d":"' % i + xs(20, i) + b'"' for i in range(n)) + b"}}")
        for el in (b"1", b"[]", b'""', b'"' + xs(20) + b'"'):
            _J(c, "arr%d_%s" % (n, el[:2].decode()), b'{"a":[' + b",".join([el] * n) + b"]}")
    c = F["header16"] = []
    # an array of sixteen 7-character reals: each takes two bytes of slack and its comma gives one back.  `[` leaves 2 and the blanks
    # behind it add B: the sixteenth real needs 2 + B - 15 >= 2, and the array16 header needs 2 + B - 15 - 2 + 1 (its `]`) >= 2
    for B, ok in ((15, False), (16, True)):
        _J(c, "array16_slack%d" % B, b'{"a":[' + b" " * B + b",".join([b"1.50000"] * 16) + b"]}", ok, None if ok else "header16_slack")
    # an object of sixteen `"":1.500`: the key gives 1, the colon 1, the real takes 4, the comma gives 1.  B blanks behind `{`: the
    # sixteenth real needs B - 15 + 2 >= 4, the map16 header B - 15 + 2 - 4 + 1 (its `}`) >= 2
    for B, ok in ((17, False), (18, True)):
        _J(c, "map16_slack%d" % B, b"{" + b" " * B + b",".join([b'"":1.500'] * 16) + b"}", ok, None if ok else "header16_slack")
    c = F["nesting"] = []
    for d in (7, 8, 9):                                                  # open containers, the root object among them
        ok, cond = d <= 8, None if d <= 8 else "depth"
        _J(c, "objects%d" % d, b'{"a":' * d + b"1" + b"}" * d, ok, cond)
        _J(c, "arrays%d" % d, b'{"a":' + b"[" * (d - 1) + b"1" + b"]" * (d - 1) + b"}", ok, cond)
        mixed_open = b"".join(b'{"a":' if i % 2 == 0 else b"[" for i in range(d))
        mixed_close = b"".join(b"}" if i % 2 == 0 else b"]" for i in reversed(range(d)))
        _J(c, "mixed%d" % d, mixed_open + b"1" + mixed_close, ok, cond)
    c = F["roots"] = []
    _J(c, "empty_object", b"{}")
    _J(c, "empty_object_blank", b"{ }")
    for name, t in (("array_root", b"[1]"), ("two_objects", b'{"a":1}{"b":2}'), ("junk_behind", b'{"a":1} x'), ("comma_close", b'{"a":1,}'),
                    ("no_colon", b'{"a" 1}'), ("comma_only", b"{,}"), ("comma_close_array", b'{"a":[1,]}'), ("wrong_closer", b'{"a":1]')):
        _J(c, name, t, False, "one_object")
    _J(c, "blank_empty", b"", nl=b"")
    _J(c, "blank_newline", b"")
    _J(c, "blank_crlf", b"\r")
    _J(c, "blank_spaces_tabs", b"  \t \t")
    toks = [b"{", b'"a"', b":", b"[", b"1", b",", b'"x"', b",", b"{", b'"b"', b":", b"null", b"}", b"]", b",", b'"c"', b":", b"true", b"}"]
    for name, ws in (("space", b" "), ("tab", b"\t"), ("cr", b"\r"), ("mix", b" \t\r ")):
        _J(c, "blanks_" + name, ws + ws.join(toks) + ws)
    # ---- B.4 copy-out
    c = F["copy_out"] = []
    for n in COPY_LENS:
        _J(c, "body%d" % n, json_row_for_body(n))
    return F


def json_row_for_body(n):
    """a row `{"k":"..."}` whose msgpack is n bytes long (81 a1 6b + the string); 1: the empty object"""
    if n == 1:
        return b"{}"
    for L in range(0, n):
        if 3 + 1 + (L > 31) + (L > 255) + L == n:
            return b'{"k":"' + xs(L) + b'"}'
    raise ValueError(n)


_FILL = []


def json_fill(n):
    if not _FILL:
        _FILL.extend(ns.lines(640, seed=11))
    return _FILL[:n]


def json_case_chunk(case, n=320):
    """the case row as the first, a middle and the last row of a tile (and as the chunk's last row when the case is about the end of the
    data) among a service's log lines -> (rows, positions)"""
    k = 4 if case.at_end else 3
    fill = json_fill(n - k)
    R, _ = json_geometry(sum(len(r) for r in fill) + k * len(case.row), n)
    pos = [R, 2 * R + R // 2, 4 * R - 1] + ([n - 1] if case.at_end else [])
    rows, it = [], iter(fill)
    for i in range(n):
        rows.append(case.row if i in pos else next(it))
    return rows, pos


def jrow(L, salt=0):
    """a one-object row of exactly L bytes, its newline among them"""
    assert L >= 9
    return b'{"p":"' + xs(L - 9, salt) + b'"}\n'


# ------------------------------------------------------------------------------------------------ JSON: staging and geometry (family A)
def json_fit_sweep(align=5):
    """A.1: tile 1 is 64 rows whose combined length goes through the wave's capacity one byte a chunk; the tile in front ends `align`
    bytes behind a 16-byte boundary -> [(total, rows, rows the pass must leave)]"""
    out = []
    for T in range(TEXT - align - 40, TEXT - align + 41):
        rows = [jrow(112, i) for i in range(63)] + [jrow(112 + align)]
        rows += [jrow(248, i) for i in range(63)] + [jrow(T - 63 * 248)]
        rows += [jrow(112, i) for i in range(64 * 7)]
        out.append((T, rows, 1 if T + align > TEXT else 0))
    return out


def json_too_long(L, where):
    """A.2: one row longer than a wave's text at `where` of tile 2 -> (rows, rows the pass must leave: it and what stands behind it in its tile)"""
    rows = [jrow(64, i) for i in range(320)]
    rows[128 + where] = jrow(L)
    return rows, 64 - where


def json_uniform(L, n):
    return [jrow(L, i) for i in range(n)]


def json_align(a, e, tail="newline"):
    """A.4: tile 1 starts `a` bytes behind a 16-byte boundary, the last row is `e` bytes longer; 130 rows: three tiles, the last of two
    rows, the workgroup that takes it has a wave without a tile"""
    rows = [jrow(112, i) for i in range(63)] + [jrow(112 + a)] + [jrow(128, i) for i in range(65)]
    last = jrow(112 + e)
    left = 0
    if tail == "no_newline":
        last = last[:-1]
    elif tail == "open_string":
        last, left = last[:-3], 1                                        # ends inside its string: the scan for the closing quote runs to the end of the data
    return rows + [last], left


def json_big(n=40000):
    """A.6: more look-back units than one window holds, from 41 distinct rows (and a row the pass leaves now and then)"""
    d = json_fill(41)
    return [b'{"u":"\\u00e9"}\n' if i % 997 == 500 else d[(i * 7 + i // 41) % 41] for i in range(n)]


# ------------------------------------------------------------------------------------------------ log events for k_grep_lane / k_l2m_lane
LEVELS = [b"info", b"warn", b"error", b"debug"]
A_RULES = ([("regex", "level ^(info|warn)$"), ("regex", "msg ok$")], "AND")     # what the staging families of grep run
L2M_LABELS = [("label_field", "color"), ("label_field", "direction")]


def rec(body, i=0, meta=None):
    return v2_record(5, i, body, meta)


def event(i, size=None, keep=None, extra=None):
    """the i-th filler event: level / msg for the grep rules, color / direction / duration for log_to_metrics.  `size`: the whole record's
    length (the msg is padded), `keep`: whether A_RULES keep it"""
    if keep is None:
        keep = i % 3 != 1
    def make(pad, z):
        body = {b"level": LEVELS[i % 2] if keep else LEVELS[2 + i % 2], b"color": [b"red", b"green", b"blue"][i % 3],
                b"msg": b"request %06d " % (i % 10 ** 6) + xs(pad, i) + b" ok", b"direction": [b"left", b"right"][i % 2], b"duration": i % 50 + z * 1000}
        if extra:
            body.update(extra)
        return rec(body, i)
    if size is None:
        return make(20, 0)
    for z in (0, 1):                                                     # (a length just behind a header's step: a longer integer makes up the byte)
        pad = size - len(make(0, z))
        for _ in range(4):
            if pad < 0:
                break
            r = make(pad, z)
            if len(r) == size:
                return r
            pad += size - len(r)
    raise ValueError("no event of %d bytes" % size)


def fit_sweep(geometry, n=320, short=120, at=64 + 10):
    """A.1 for the kernels whose capacity follows the chunk's mean: record `at` (in tile 1) grows from "the tile fits easily" to "its last
    record misses by a few hundred bytes" in 16 steps -> [(over, records)], over = the tile's bytes - the capacity"""
    assert (64 * short) % 16 == 0                                        # tile 1 starts on a 16-byte boundary
    table = {}
    for X in range(short, TEXT - 64):
        R, cap = geometry((n - 1) * short + X, n)
        if R != 64:
            break
        table.setdefault(63 * short + X - cap, X)
    out = []
    for want in (-900, -500, -200, -64, -16, -1, 0, 1, 2, 15, 16, 17, 64, 150, 300, 420):
        o = min(table, key=lambda v: (abs(v - want), v))
        recs = [event(i, short) for i in range(n)]
        recs[at] = event(at, table[o], keep=True)
        out.append((o, recs))
    return out


def too_long(L, behind, keep, n=600, short=120):
    """A.2: a record that no wave can hold with `behind` short kept records behind it in its tile (tile 2) -> (records, index)"""
    at = 3 * 64 - 1 - behind
    recs = [event(i, short) for i in range(n)]
    for i in range(at + 1, 3 * 64):
        recs[i] = event(i, short, keep=True)
    recs[at] = event(at, L, keep=keep, extra={b"color": b"long", b"duration": 77})
    return recs, at


def uniform(L, n):
    return [event(i, L) for i in range(n)]


def aligned(a, e, n=130, short=112):
    """A.4: tile 1 starts `a` bytes behind a 16-byte boundary, the chunk ends `e` bytes behind one (+ a)"""
    recs = [event(i, short) for i in range(n)]
    recs[63] = event(63, short + a)
    recs[n - 1] = event(n - 1, short + e)
    return recs


def tile_max_chunk(last_over_16k, n=66000):
    """A.5: a chunk large enough for k_tile_max, short records with one run of 64 four times as long that straddles two tiles"""
    short = [event(i, 96) for i in range(6)]
    long_ = [event(i, 384) for i in range(6)]
    recs = [short[(i * 5 + i // 7) % 6] for i in range(n)]
    s = 33000 + 17
    for i in range(s, s + 64):
        recs[i] = long_[i % 6]
    if last_over_16k:
        recs[s + 63] = event(3, 16500, keep=True)
    return recs


def run_pattern_chunk(n=70000):
    """A.6: kept and dropped records of different lengths in runs of unequal length -> (records, kept flags)"""
    kept = [event(0, 96, keep=True), event(2, 131, keep=True), event(4, 107, keep=True)]
    drop = [event(1, 101, keep=False), event(3, 150, keep=False)]
    runs = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144)
    recs, flags, k, r = [], [], True, 0
    while len(recs) < n:
        for j in range(runs[r % len(runs)]):
            recs.append(kept[len(recs) % 3] if k else drop[len(recs) % 2])
            flags.append(k)
        k, r = not k, r + 1
    return recs[:n], flags[:n]


# ---- the shape gl_walk / l2l_record take (lane_dev.inc), restated from the bytes
def _skip(b, p, opened=None):
    """end of the object at p when it is made of what the lean walk steps over (at most eight containers in one value); None otherwise"""
    opened = [0] if opened is None else opened
    if p >= len(b):
        return None
    c = b[p]
    if c <= 0x7f or c >= 0xe0 or c in (0xc0, 0xc2, 0xc3): return p + 1
    if 0xa0 <= c <= 0xbf: return p + 1 + (c & 31)
    if c in (0xcc, 0xd0): return p + 2
    if c in (0xcd, 0xd1): return p + 3
    if c in (0xce, 0xd2, 0xca): return p + 5
    if c in (0xcf, 0xd3, 0xcb): return p + 9
    if c == 0xd9: return p + 2 + b[p + 1]
    if c == 0xda: return p + 3 + struct.unpack(">H", b[p + 1:p + 3])[0]
    if 0x80 <= c <= 0x8f: n, q = 2 * (c & 15), p + 1
    elif 0x90 <= c <= 0x9f: n, q = c & 15, p + 1
    elif c == 0xde: n, q = 2 * struct.unpack(">H", b[p + 1:p + 3])[0], p + 3
    elif c == 0xdc: n, q = struct.unpack(">H", b[p + 1:p + 3])[0], p + 3
    else: return None
    opened[0] += 1
    if opened[0] > 8:
        return None
    for _ in range(n):
        q = _skip(b, q, opened)
        if q is None:
            return None
    return q


def plain_event(b):
    """is b one V2 log event as the lean walk takes it: `92 92 d7 00 <sec> <nsec> 80`, a timestamp the decoder does not hide, a fixmap /
    map16 body of string keys (up to str16) whose values are strings, numbers, nil / booleans and small containers of those, and
    nothing behind it"""
    if len(b) < 14 or b[:4] != b"\x92\x92\xd7\x00" or b[12] != 0x80:
        return False
    sec, nsec = struct.unpack(">II", b[4:12])
    if sec >= 0xfffffffe or nsec >= 10 ** 9:
        return False
    c, p = b[13], 14
    if 0x80 <= c <= 0x8f: n = c & 15
    elif c == 0xde and len(b) >= 16: n, p = struct.unpack(">H", b[14:16])[0], 16
    else: return False
    for _ in range(n):
        if p >= len(b) or not (0xa0 <= b[p] <= 0xbf or b[p] in (0xd9, 0xda)):
            return False
        p = _skip(b, p)
        p = _skip(b, p) if p is not None else None
        if p is None or p > len(b):
            return False
    return p == len(b)


# ------------------------------------------------------------------------------------------------ k_grep_lane: walk, values, automata, verdict (family C)
NAME_LENS = [1, 3, 4, 5, 7, 8, 9, 12, 16, 31, 32]


def name(n):
    return b"abcdefghijklmnopqrstuvwxyz012345"[:n]


def name_records(n):
    """C.1: [(what, body, plain)] around the name of n bytes; a rule `<name> ^hit$` keeps exactly what holds it with the value "hit" last"""
    k = name(n)
    out = [("exact", {k: b"hit"}), ("shorter", {k[:-1]: b"hit"}), ("longer", {k + b"x": b"hit"}), ("last_byte", {k[:-1] + b"#": b"hit"}),
           ("first_byte", {b"#" + k[1:]: b"hit"}), ("forty", KV([(b"k" * 40, b"hit"), (k, b"hit")])), ("forty_only", {b"k" * 40: b"hit"}),
           ("twice_hit_last", KV([(k, b"miss"), (k, b"hit")])), ("twice_miss_last", KV([(k, b"hit"), (k, b"miss")])),
           ("twice_int_last", KV([(k, b"hit"), (k, 7)])), ("final_key", KV([(b"other", b"x"), (k, b"hit")])),
           ("final_key_empty_value", KV([(b"other", b"hit"), (k, b"")])), ("only_key_no_other", {k: b"hit "})]
    if n >= 9:
        out.append(("byte9", {k[:8] + b"#" + k[9:]: b"hit"}))
    if n >= 5:
        out.append(("byte5", {k[:4] + b"#" + k[5:]: b"hit"}))
    if n <= 31:
        out.append(("str8_name", KV([(Raw(b"\xd9" + bytes([n]) + k), b"hit")])))
    out.append(("str16_name", KV([(Raw(b"\xda" + struct.pack(">H", n) + k), b"hit")])))
    return [(w, b, True) for w, b in out]


def forced_str(v, enc):
    if enc == "str8": return Raw(b"\xd9" + bytes([len(v)]) + v)
    if enc == "str16": return Raw(b"\xda" + struct.pack(">H", len(v)) + v)
    return v


VALUE_PATTERNS = ["^a+$", "a$", "^$", ".", "b", "Q", "^.é", "[^a]$", "é"]


def value_records():
    """C.2: [(what, value, plain)] for the key `log`"""
    out = []
    for L in list(range(10)) + [31, 32, 255, 256, 700]:
        out.append(("a*%d" % L, b"a" * L, True))
        out.append(("a*%d+b" % L, b"a" * L + b"b", True))
        if L < 256:
            out.append(("a*%d as str8" % L, forced_str(b"a" * L, "str8"), True))
        out.append(("a*%d as str16" % L, forced_str(b"a" * L, "str16"), True))
    for end in (1, 2, 3, 4, 5, 8, 9):                                    # the literal's match ends at byte `end`: "match whatever follows" at every place of the 4-byte step
        out.append(("Q ends at %d" % end, b"xxxxxxxx"[:end - 1] + b"Q" + b"zzzzzz", True))
        out.append(("Q ends at %d, the end" % end, b"xxxxxxxx"[:end - 1] + b"Q", True))
    for o in range(5):                                                   # the automaton hands the value on at every place of the step
        out.append(("é at %d" % o, b"a" * o + "é".encode() + b"aaa", True))
        out.append(("é at %d, the end" % o, b"a" * o + "é".encode(), True))
    for what, v, plain in (("int", 7, True), ("negative", -70000, True), ("float", 1.5, True), ("true", True, True), ("nil", None, True),
                           ("map", {b"m": b"a"}, True), ("array", [b"a", b"b"], True), ("map16", {b"k%02d" % i: b"a" for i in range(17)}, True),
                           ("bin", Raw(b"\xc4\x02ab"), False), ("ext", Raw(b"\xd4\x05a"), False), ("str32", Raw(b"\xdb\x00\x00\x00\x02ab"), False)):
        out.append((what, v, plain))
    return out


def nonascii_offset(v):
    """offset of the first byte >= 0x80 of a value (C.2's é cases)"""
    return next(i for i, c in enumerate(v) if c >= 0x80)


SUBKEY_RULES = ["$k['a']['b'] ^hit$", "$k['a'] ^hit$", "$k[0] ^hit$"]


def subkey_records():
    """C.2: [(what, body, plain)] for `$k['a']['b']`, `$k['a']` and `$k[0]`"""
    big = {b"f%02d" % i: b"x" for i in range(16)}
    return [
        ("fixmap parents", {b"k": {b"a": {b"b": b"hit"}}}, True),
        ("map16 parent", {b"k": dict(big, a={b"b": b"hit"})}, True),
        ("map16 inner", {b"k": {b"a": dict(big, b=b"hit")}}, True),
        ("child is the value", {b"k": {b"a": b"hit"}}, True),
        ("array parent", {b"k": [b"hit", {b"a": {b"b": b"hit"}}]}, True),
        ("array in the middle", {b"k": {b"a": [b"hit", b"b"]}}, True),
        ("missing child", {b"k": {b"a": {b"c": b"hit"}}}, True),
        ("missing parent", {b"j": {b"a": {b"b": b"hit"}}}, True),
        ("child twice, hit last", {b"k": {b"a": KV([(b"b", b"miss"), (b"b", b"hit")])}}, True),
        ("child twice, miss last", {b"k": {b"a": KV([(b"b", b"hit"), (b"b", b"miss")])}}, True),
        ("parent twice", {b"k": KV([(b"a", {b"b": b"miss"}), (b"a", {b"b": b"hit"})])}, True),
        ("long child key", {b"k": {b"a": KV([(b"z" * 33, b"x"), (b"b", b"hit")])}}, True),
        ("parent is a string", {b"k": b"hit"}, True),
        ("parent is an int", {b"k": 5}, True),
        ("child is an int", {b"k": {b"a": {b"b": 5}}}, True),
    ]


RULE_COUNTS = [1, 5, 6, 7, 12, 13, 63, 64]


def count_rules(n, kind):
    """C.3: n rules over eight names (the walk's slots); rule i asks for `xII` in the value of `f<i mod 8>`"""
    return [(kind, "f%d x%02d" % (i % 8, i)) for i in range(n)]


def count_records(n):
    """C.3: [(what, body)]: which of the n rules of count_rules match"""
    def body(match):
        return {b"f%d" % j: b" ".join(b"x%02d" % i for i in range(n) if i % 8 == j and i in match) for j in range(8)}
    allr = set(range(n))
    out = [("none", body(set())), ("all", body(allr)), ("only the last", body({n - 1})), ("all but the last", body(allr - {n - 1})),
           ("only the first", body({0})), ("all but the first", body(allr - {0}))]
    if n > 6:
        out += [("only the sixth", body({5})), ("only the seventh", body({6})), ("all but the seventh", body(allr - {6}))]
    return out


def shape_records():
    """C.4: [(what, row bytes, plain, ends the call with NOTOUCH)]"""
    body = {b"level": b"info", b"msg": b"it went ok"}
    trunc = rec(body, 3)[:-4]
    return [
        ("empty body", rec({}, 1), True, False),
        ("map16 body, 16 keys", rec(dict({b"k%02d" % i: b"v" for i in range(14)}, **{"level": b"info", "msg": b"ok"}), 1), True, False),
        ("map16 body, 17 keys", rec(dict({b"k%02d" % i: b"v" for i in range(15)}, **{"level": b"warn", "msg": b"ok"}), 1), True, False),
        ("metadata", rec(body, 1, meta={b"m": 1}), False, False),
        ("legacy event", legacy_record(5, body), False, False),
        ("legacy event, float time", legacy_record(1.5, body), False, False),
        ("group start", mp([[ext_ts(0xffffffff, 0), {}], {b"g": 1}]), False, False),
        ("group end", mp([[ext_ts(0xfffffffe, 0), {}], {}]), False, False),
        ("nsec 1e9", v2_record(5, 10 ** 9, body), False, True),           # (the decoder refuses it)
        ("sec fffffffd", v2_record(0xfffffffd, 1, body), True, False),
        ("integer key", rec(KV([(5, b"x"), (b"level", b"info"), (b"msg", b"ok")]), 1), False, False),
        ("nine containers deep", rec(dict(body, deep=[[[[[[[[[1]]]]]]]]]), 1), False, False),
        ("trailing bytes", rec(body, 2) + b"\xc0", False, True),
        ("truncated", trunc, False, True),
    ]


def copy_record(size, keep):
    """C.5: a record of `size` bytes that `exclude l ^d` keeps or drops; 14 bytes: the empty map"""
    if size == 14:
        assert keep
        return rec({}, 7)
    for L in range(1, size):
        r = rec({b"l": (b"i" if keep else b"d") + xs(L - 1)}, 7)
        if len(r) == size:
            return r
    raise ValueError(size)


COPY_RULES = ([("exclude", "l ^d")], None)
REC_LENS = [14] + COPY_LENS[1:]


def copy_chunk():
    """C.5: kept / dropped / kept for every length, a tile where nothing is kept, a tile where only lane 63 is -> records; the tiles are of
    64 records (test_lane_chunks proves it)"""
    d = copy_record(160, False)                                          # (long enough for a mean that gives the waves room for the 513-byte records)
    recs = []
    for s in REC_LENS:
        recs += [copy_record(s, True), copy_record(max(s, 31), False), copy_record(s, True)]
    recs += [d] * (64 - len(recs))                                       # tile 0
    recs += [d] * 64                                                     # tile 1: nothing kept
    recs += [d] * 63 + [copy_record(65, True)]                           # tile 2: lane 63 alone
    recs += [copy_record(s, True) for s in REC_LENS] + [d] * 50          # tile 3: a run of kept records of every length
    return recs


# ------------------------------------------------------------------------------------------------ k_l2m_lane (family D)
def l2m_value_records():
    """[(what, value or None for "no such field", what log_to_metrics makes of it)] for the value field `duration`; the label `color` names
    the variant"""
    return [("int", 20, "value"), ("negative", -20, "value"), ("uint64", 2 ** 63 + 5, "value"), ("float32", Raw(b"\xca\x41\xa0\x00\x00"), "value"),
            ("float64", 20.5, "value"), ("text", b"20", "value"), ("blank_text", b" 20", "value"), ("exp_text", b"2e1", "value"), ("hex_text", b"0x10", "value"),
            ("empty_text", b"", "stale"), ("letters", b"abc", "stale"), ("hard_decimal", HARD_DECIMAL, "deferred"),
            ("str8", forced_str(b"21", "str8"), "value"), ("str16", forced_str(b"22", "str16"), "value"), ("true", True, "other"), ("nil", None, "other"),
            ("map", {b"m": 1}, "other"), ("missing", "MISSING", "other"), ("twice", "TWICE", "value")]


def l2m_value_chunk():
    recs = []
    for i, (what, v, _) in enumerate(l2m_value_records()):
        body = [(b"color", what.encode()), (b"direction", b"left"), (b"msg", b"x")]
        if v == "TWICE":
            body += [(b"duration", 1), (b"duration", 30)]
        elif v != "MISSING":
            body.insert(1, (b"duration", v))
        recs += [rec(KV(body), i)] * 2
    return recs


def l2m_label_chunk():
    mk = lambda items, i: rec(KV(items + [(b"duration", 3)]), i)
    return [mk([(b"color", b"red"), (b"direction", b"left")], 0), mk([(b"direction", b"left")], 1), mk([(b"color", b"red")], 2), mk([], 3),
            mk([(b"color", b"red"), (b"color", b"blue"), (b"direction", b"left")], 4), mk([(b"color", 7), (b"direction", b"left")], 5),
            mk([(b"color", True), (b"direction", None)], 6), mk([(b"color", 1.5), (b"direction", b"left")], 7),
            mk([(b"color", {b"m": 1}), (b"direction", [1, 2])], 8), mk([(b"color", b"x" * 300), (b"direction", forced_str(b"left", "str16"))], 9)]


def l2m_name_chunk(n):
    """C.1's names as a label key and (with its first byte changed) as the value key -> (label key, value key, records)"""
    k = name(n)
    vk = b"V" + k[1:]
    recs = []
    for i, (what, body, _) in enumerate(name_records(n)):
        items = list(body.items()) if isinstance(body, dict) else list(body.items)
        recs.append(rec(KV(items + [(vk, i + 1), (b"color", what.encode())]), i))
        recs.append(rec(KV([(b"color", what.encode()), (vk[:-1] + b"#", 99), (k, b"lab")] + ([(vk, 5)] if i % 2 else [])), i))
    return k, vk, recs

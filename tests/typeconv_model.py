"""CPU model of filter_type_converter (plugins/filter_type_converter/type_converter.c), restated on the msgpack walker of
tests/modify_model.py: the config map, config_rule and configure() (:57-140, :366-388), the type words and the conversions of
src/flb_typecast.c, the accessor as flb_ra_create cuts it (src/flb_record_accessor.c:74-230) and one call with its return codes
(:182-353).  The numbers come from glibc through ctypes (strtoimax, strtoumax, strtod, snprintf), as the reference takes them; the
model is the yardstick of tests/test_typeconv_*.py and does not use the product."""
import ctypes
import re
import struct

import modify_model as mm
import recmod_model as rmm

MAX_RULES, MAX_TABLE_BYTES, MAX_KEY, MAX_SUBKEYS, MAX_SUB_BYTES = 64, 32768, 128, 8, 256
STR, INT, UINT, FLOAT = 0, 1, 2, 3
TYPES = ["int", "uint", "float", "hex", "string", "bool"]             # the order flb_typecast_str_to_type_t tries them in
T_INT, T_UINT, T_FLOAT, T_HEX, T_STR, T_BOOL = range(6)
SRC = ["str", "int", "uint", "float"]
PROPS = ["str_key", "int_key", "uint_key", "float_key"]                # configure()'s order
M64 = (1 << 64) - 1

_c = ctypes.CDLL(None)
_c.strtoimax.restype = ctypes.c_longlong
_c.strtoimax.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
_c.strtoumax.restype = ctypes.c_ulonglong
_c.strtoumax.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
_c.strtod.restype = ctypes.c_double
_c.strtod.argtypes = [ctypes.c_char_p, ctypes.c_void_p]


def c_fmt(fmt, v):
    buf = ctypes.create_string_buffer(512)
    n = _c.snprintf(buf, 511, fmt, ctypes.c_double(v))
    return buf.raw[:n]


# ---------------------------------------------------------------- configuration
def split_tokens(val, maxn):
    """flb_slist_split_tokens(list, val, maxn) (src/flb_slist.c:182-217)"""
    s = val.encode() if isinstance(val, str) else val
    s = s.split(b"\0")[0]
    out, pos, count = [], 0, 0
    while True:
        tok, pos = rmm._token(s, pos)
        if tok is None:
            break
        out.append(tok)
        if pos is None:
            break
        count += 1
        if count >= maxn:
            rest = s[pos:].lstrip(b" ")
            if rest:
                out.append(rest)
            break
    return out


def type_of_word(w):
    """strncasecmp(word, name, strlen(word)) == 0: the word is a prefix of the name (src/flb_typecast.c:27-49)"""
    w = w.lower()
    for i, name in enumerate(TYPES):
        if name.encode().startswith(w):
            return i
    return None


class Skip(ValueError):
    """flb_ra_create answers NULL.  config_rule then frees the rule with delete_conv_entry, which unlinks an entry that was never
    linked (:52, :95-100): the reference dies, and so it does at an unknown type word.  Create refuses both."""


def meta_part(t):
    """one `$name['a'][1]` part; Skip where the grammar refuses it, ValueError where create has a limit"""
    m = re.match(rb"\$([A-Za-z_][A-Za-z0-9_.\-/]*)", t)
    if not m:
        raise ValueError("record accessor %r" % t)
    if len(m.group(1)) >= MAX_KEY:
        raise ValueError("key too long")
    key, p, subs, nbytes = m.group(1), m.end(), [], 0
    while t[p:p + 1] == b"[":
        if len(subs) >= MAX_SUBKEYS:
            raise ValueError("too many subkeys")
        p += 1
        if t[p:p + 1] == b"'":
            p += 1
            s = bytearray()
            while True:
                if p >= len(t):
                    raise Skip()
                if t[p:p + 1] == b"'":
                    if t[p + 1:p + 2] == b"'":
                        s.append(0x27)
                        p += 2
                        continue
                    p += 1
                    break
                s.append(t[p])
                p += 1
                if nbytes + len(s) > MAX_SUB_BYTES:
                    raise ValueError("subkeys too long")
            nbytes += len(s)
            subs.append(("s", bytes(s)))
        elif t[p:p + 1].isdigit():
            m2 = re.match(rb"[0-9]+", t[p:])
            subs.append(("i", int(m2.group(0))))
            p += m2.end()
        else:
            raise Skip()
        if t[p:p + 1] != b"]":
            raise Skip()
        p += 1
    if p != len(t):
        raise Skip()
    return (key, subs)


def accessor(a):
    """ra_parse_buffer's parts, then get_ra_parser: the FIRST part decides.  (key, subs), or None for a rule that never finds a key"""
    n = len(a)
    first = []                                    # [] none yet, [None] a part without a key, [(key, subs)]

    def string_part(lo, hi):
        if not first:
            if hi - lo >= MAX_KEY:
                raise ValueError("key too long")
            first.append((a[lo:hi], []))

    def no_key():
        if not first:
            first.append(None)
    pre = end = i = 0
    while i < n:
        if a[i] != 0x24:
            i += 1
            continue
        if i > pre:
            string_part(pre, i)
        pre = i
        nx = i + 1
        if nx >= n:
            break
        if a[nx:nx + 1].isdigit():
            no_key()
            i += 1
            pre = i + 1
            i += 1
            continue
        if nx + 2 < n and a[nx:nx + 3] == b"TAG":
            no_key()
            if nx + 4 < n and a[nx + 3] == 0x5b:
                t = nx + 3
                e = a.find(b"]", t)
                e = e - t if e >= 0 else -1
                if e == 0:
                    e = -1
                i = t + e + 1
                pre = i
                i += 1
                continue
            i = nx + 3
            pre = nx + 3
            i += 1
            continue
        quotes, end = 0, i + 1
        while end < n:
            c = a[end]
            if c == 0x27:
                quotes += 1
            elif c == 0x2e and quotes & 1:
                pass
            elif c in (0x2e, 0x20, 0x2c, 0x22):
                break
            end += 1
        part = meta_part(a[i:end])
        if not first:
            first.append(part)
        pre = end
        i = end + 1
    if ((i - 1 > end and pre < i) or i == 1) and pre < n:
        string_part(pre, n)
    return first[0] if first else None


class Rule:
    def __init__(self, src, to, ra, to_key):
        self.src, self.to, self.ra, self.to_key = src, to, ra, to_key


def table_bytes(rules):
    def pad4(x):
        return (x + 3) // 4 * 4
    n = 0
    for r in rules:
        key, subs = r.ra if r.ra else (b"", [])
        n += 24 + 8 * len(subs) + sum(pad4(len(x)) for k, x in subs if k == "s") + pad4(len(key))
        n += pad4(len(mm.pack_str_hdr(len(r.to_key))) + len(r.to_key))
    return n


def parse(props):
    """the rules in configure()'s order; ValueError where the filter does not start or create refuses"""
    groups = [[] for _ in PROPS]
    for name, val in props:
        name = (name.decode() if isinstance(name, bytes) else name).lower()
        if name not in PROPS:
            raise ValueError("unknown property %s" % name)
        tok = split_tokens(val, 3)
        if len(tok) < 3:                          # SLIST_3: the config map's size check
            raise ValueError("%s needs three entries" % name)
        groups[PROPS.index(name)].append(tok)
    rules = []
    for src, g in enumerate(groups):
        for tok in g:
            if len(tok) != 3:                     # config_rule's -1, ignored by configure()
                continue
            to = type_of_word(tok[2])
            if to is None:
                raise Skip("unknown type word %r" % tok[2])
            ra = accessor(tok[0])
            rules.append(Rule(src, to, ra, tok[1]))
    if not rules:
        raise ValueError("no rules")
    if len(rules) > MAX_RULES:
        raise ValueError("too many rules")
    if table_bytes(rules) > MAX_TABLE_BYTES:
        raise ValueError("rule table too large")
    return rules


def describe(rules):
    """the text flbgpu_type_converter_parse_check writes"""
    out = []
    for r in rules:
        if r.ra is None:
            k = "-"
        else:
            k = "K" + r.ra[0].hex() + "".join("[%d]" % x if kind == "i" else "." + x.hex() for kind, x in r.ra[1])
        out.append("%s>%s,%s,T%s" % (SRC[r.src], TYPES[r.to], k, r.to_key.hex()))
    return ";".join(out)


# ---------------------------------------------------------------- conversions
def pack_i64(v):
    """msgpack_pack_int64: a value >= 0 goes out in the unsigned formats"""
    return mm.canon(mm.Obj("uint" if v >= 0 else "int", v, None, None))


def pack_u64(v):
    return mm.canon(mm.Obj("uint", v, None, None))


def pack_f64(v):
    return b"\xcb" + struct.pack(">d", v)


def pack_str(b):
    return mm.pack_str_hdr(len(b)) + b


def cvttsd2si(v):
    """x86-64's double -> int64: NaN and what does not fit answer INT64_MIN"""
    if v != v or v >= 2.0 ** 63 or v < -2.0 ** 63:
        return -(1 << 63)
    return int(v)


def float_to_int(v):
    """(int64_t) v as x86-64 answers, and whether C leaves it undefined (NaN, |v| >= 2^63; -2^63 is counted with them)"""
    return cvttsd2si(v), (v != v or abs(v) >= 2.0 ** 63)


def float_to_uint(v):
    """(uint64_t) v as gcc compiles it for x86-64: below 2^63 cvttsd2si(v), else cvttsd2si(v - 2^63) with the top bit flipped"""
    undef = v != v or v <= -1.0 or v >= 2.0 ** 64
    if v >= 2.0 ** 63:
        return (cvttsd2si(v - 2.0 ** 63) & M64) ^ (1 << 63), undef
    return cvttsd2si(v) & M64, undef


def float_to_str(v):
    """flb_typecast_conv_float (:309-315): "%.1f" when v == (double)(long long) v, else "%.16g" """
    if v == float(cvttsd2si(v)):
        return c_fmt(b"%.1f", v)
    return c_fmt(b"%.16g", v)


def convert(rule, o):
    """flb_typecast_pack: (packed bytes | None when it fails, undefined)"""
    src, to = rule.src, rule.to
    if src == STR:
        if o.t != "str":
            return None, False
        s = o.v
        if to == T_INT:
            x = _c.strtoimax(s, None, 10)
            return (pack_i64(x) if x else None), False
        if to in (T_UINT, T_HEX):
            x = _c.strtoumax(s, None, 16 if to == T_HEX else 10)
            return (pack_u64(x) if x else None), False
        if to == T_FLOAT:
            return pack_f64(_c.strtod(s, None)), False
        if to == T_BOOL:
            z = s.split(b"\0")[0].lower()
            if len(s) >= 4 and z[:4] == b"true":
                return b"\xc3", False
            if len(s) >= 5 and z[:5] == b"false":
                return b"\xc2", False
        return None, False
    if src in (INT, UINT):
        if o.t not in ("uint", "int"):
            return None, False
        i64 = o.v - (1 << 64) if o.v >= 1 << 63 else o.v
        u64 = o.v & M64
        if src == INT:
            if to == T_STR:
                return pack_str(b"%d" % i64), False
            if to == T_FLOAT:
                return pack_f64(float(i64)), False
            if to == T_UINT:
                return pack_u64(u64), False
            return None, False
        if to == T_STR:
            return pack_str(b"%d" % u64), False
        if to == T_FLOAT:
            return pack_f64(float(u64)), False
        if to == T_INT:
            return pack_i64(i64), False
        return None, False
    if o.t not in ("f32", "f64"):
        return None, False
    v = struct.unpack(">f" if o.t == "f32" else ">d", o.v)[0]
    if to == T_STR:
        return pack_str(float_to_str(v)), False
    if to == T_INT:
        x, undef = float_to_int(v)
        return pack_i64(x), undef
    if to == T_UINT:
        x, undef = float_to_uint(v)
        return pack_u64(x), undef
    return None, False


def record(rules, raw, stats, pairs=None):
    """one record of the loop (:240-318): its output bytes"""
    end, skip, sec, nsec, meta, body = mm.decode_event(raw, 0)
    if not (0 <= sec <= 0xffffffff and 0 <= nsec < 1000000000):
        sec = nsec = 0                            # set_timestamp's refusal is overwritten (:252-257)
    out = [mm.canon(k) + mm.canon(v) for k, v in body.v]
    for r in rules:
        v = mm.ra_get(r.ra, body)
        if v is None:
            continue
        got, undef = convert(r, v)
        if pairs is not None:
            pairs.setdefault((r.src, r.to), [0, 0])[0 if got is not None else 1] += 1
        if got is None:
            stats[1] += 1
            got = mm.canon(v)
        else:
            stats[0] += 1
            stats[2] += undef
        out.append(pack_str(r.to_key) + got)
    head = b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + (mm.canon(meta) if meta is not None else b"\x80")
    return head + b"\xdf" + struct.pack(">I", len(out)) + b"".join(out)


class Model:
    """cb_type_converter_filter over a chunk: filter(data) -> (MODIFIED|NOTOUCH, bytes|None), counts() as flbgpu_filter_last_counts,
    counters() as flbgpu_type_converter_counters (since the model was created); pairs: per (source, target) [done, failed]"""
    MODIFIED, NOTOUCH = 1, 2

    def __init__(self, props):
        self.rules = parse(props)
        self.stats = [0, 0, 0, 0]                 # done, failed, undefined, size/emit mismatches (the model has none)
        self.pairs = {}
        self.n_in = 0

    def filter(self, data):
        p, out, n, bad = 0, [], 0, False
        done0 = self.stats[0]
        while p < len(data):
            try:
                end, skip, *_ = mm.decode_event(data, p)
            except mm.Bad:
                bad = not mm.clean_cut(data, p)   # INSUFFICIENT_DATA with the offset at the end is a clean end (:328-331)
                break
            if not skip:
                n += 1
                out.append(record(self.rules, bytes(data[p:end]), self.stats, self.pairs))
            p = end
        self.n_in = n
        if self.stats[0] == done0 or bad:         # is_record_modified stayed false (:321-326) / "encoder error" (:341-346)
            return self.NOTOUCH, None
        return self.MODIFIED, b"".join(out)

    def counts(self):
        return self.n_in, self.n_in

    def counters(self):
        return tuple(self.stats)

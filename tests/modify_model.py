"""CPU model of filter_modify (plugins/filter_modify/modify.c), restated line by line on a msgpack walker that keeps the raw
spans: the program setup() builds (:141-519), the conditions (:523-953), the rules (:955-1337), one record (:1341-1457) and one
call (:1486-1578).  Regex comes from the oracle's flb_regex restatement (oracle/oflb.c).  The model is the yardstick of
tests/test_modify_*.py; it does not use the product."""
import ctypes
import os
import re
import struct

# ---------------------------------------------------------------- configuration
RULES1 = {"remove": 4, "remove_wildcard": 5, "remove_regex": 6, "move_to_start": 9, "move_to_end": 10}
# (setup() also knows "add_if_not_present", :447-452, but the config map, :1589-1655, does not: the filter refuses it before setup() runs)
RULES2 = {"rename": 0, "hard_rename": 1, "add": 2, "set": 3, "copy": 7, "hard_copy": 8}
RENAME, HARD_RENAME, ADD, SET, REMOVE, REMOVE_WILDCARD, REMOVE_REGEX, COPY, HARD_COPY, MOVE_TO_START, MOVE_TO_END = range(11)
CONDS = ["key_exists", "key_does_not_exist", "a_key_matches", "no_key_matches", "key_value_equals", "key_value_does_not_equal",
         "key_value_matches", "key_value_does_not_match", "matching_keys_have_matching_values",
         "matching_keys_do_not_have_matching_values"]
MAX_RULES, MAX_CONDS, MAX_KEY = 64, 32, 128


def a_rx(t):
    return t in (2, 3, 8, 9)


def b_rx(t):
    return t in (6, 7, 8, 9)


def split_quoted(line):
    """flb_utils_split_quoted(line, ' ', 3) (src/flb_utils.c:278-462); None on an unterminated quote"""
    s = line.encode() if isinstance(line, str) else line
    s = s.split(b"\0")[0]
    n, i, out = len(s), 0, []
    while i < n:
        j = i
        while j < n and s[j:j + 1] == b" ":
            j += 1
        if j >= n or s[j:j + 1] not in (b'"', b"'"):
            rest = s[j:]
            k = rest.find(b" ")
            tl = k if k > 0 else len(rest)
            out.append(rest[:tl])
            i = j + tl
        else:
            quote = s[j]
            q, ql, qs = j + 1, 0, quote
            while qs:
                if q >= n:
                    return None
                c = s[q]
                q += 1
                if c == 0x5c:
                    if q < n and (s[q] == quote or s[q] == 0x5c):
                        q += 1
                elif c in (0x22, 0x27) and c == qs:
                    qs = 0
                ql += 1
            ql -= 1
            p, tok = j + 1, bytearray()
            for _ in range(ql):
                if s[p] == 0x5c and p + 1 < n and s[p + 1] in (quote, 0x5c):
                    p += 1
                tok.append(s[p])
                p += 1
            out.append(bytes(tok))
            i = p
        i += 1
        if len(out) >= 3 and i < n:
            out.append(s[i:])
            break
    return out


_NONREGULAR = re.compile(rb"\(\?<?[=!]|\(\?>|\\[1-9]|\\k<|\(\?~|[*+?}]\+")


_REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libflbregex_ref.so")
_ref_lib = []


def _ref():
    """the real src/flb_regex.c over the real Onigmo (oracle/_ref), None where it is not built"""
    if not _ref_lib:
        L = None
        if os.path.exists(_REF):
            L = ctypes.CDLL(_REF)
            L.flb_regex_create.restype = ctypes.c_void_p
            L.flb_regex_create.argtypes = [ctypes.c_char_p]
            L.flb_regex_destroy.argtypes = [ctypes.c_void_p]
        _ref_lib.append(L)
    return _ref_lib[0]


class Regex:
    """flb_regex_create / flb_regex_match: the compile verdict from the real Onigmo where oracle/_ref is built, the searches (and the
    verdict elsewhere) from the oracle's restatement (oracle/oflb.c)"""
    _cache = {}

    def __init__(self, pat):
        import oracle_binding as ob
        self.L = ob.lib()
        self.pat = pat
        self.h = self.L.oflb_regex_create(pat)
        self.ok = bool(self.h)
        ref = _ref()
        if ref is not None:
            r = ref.flb_regex_create(pat)
            self.ok = bool(r)
            if r:
                ref.flb_regex_destroy(r)
        self.nonregular = bool(_NONREGULAR.search(pat))

    def search(self, s):
        assert self.h, "the oracle's engine does not take %r" % self.pat
        return self.L.oflb_regex_match(self.h, s, len(s)) > 0

    @classmethod
    def get(cls, pat):
        r = cls._cache.get(pat)
        if r is None:
            r = cls._cache[pat] = Regex(pat)
        return r


def accessor(a):
    """flb_ra_create(a) then get_ra_parser: None (never finds a value) or (key, [("s", bytes) | ("i", n), ...]); raises on a bad one"""
    d = a.find(b"$")
    if d != 0:
        name = a if d < 0 else a[:d]
        if not name:
            return None
        if len(name) >= MAX_KEY:
            raise ValueError("condition key too long")
        return (name, [])
    if len(a) == 1 or a[1:2].isdigit() or (len(a) >= 4 and a[1:4] == b"TAG"):
        return None
    end, quotes = 1, 0
    while end < len(a):
        c = a[end:end + 1]
        if c == b"'":
            quotes += 1
        elif c == b"." and quotes & 1:
            pass
        elif c in (b".", b" ", b",", b'"'):
            break
        end += 1
    t = a[1:end]
    m = re.match(rb"[A-Za-z_][A-Za-z0-9_.\-/]*", t)
    if not m or len(m.group(0)) >= MAX_KEY or m.group(0) == b"TAG":
        raise ValueError("record accessor")
    key, p, subs = m.group(0), m.end(), []
    while p < len(t) and t[p:p + 1] == b"[":
        p += 1
        if t[p:p + 1] == b"'":
            p += 1
            s = bytearray()
            while True:
                if p >= len(t):
                    raise ValueError("record accessor")
                if t[p:p + 1] == b"'":
                    if t[p + 1:p + 2] == b"'":
                        s.append(0x27)
                        p += 2
                        continue
                    p += 1
                    break
                s.append(t[p])
                p += 1
            subs.append(("s", bytes(s)))
        elif t[p:p + 1].isdigit():
            m2 = re.match(rb"[0-9]+", t[p:])
            subs.append(("i", int(m2.group(0))))
            p += m2.end()
        else:
            raise ValueError("record accessor")
        if t[p:p + 1] != b"]":
            raise ValueError("record accessor")
        p += 1
        if len(subs) > 8:
            raise ValueError("record accessor")
    if p != len(t):
        raise ValueError("record accessor")
    return (key, subs)


def check_rx(pat, executed):
    r = Regex.get(pat)
    if not r.ok:
        raise ValueError("Unable to create regex from %r" % pat)
    if executed and r.nonregular:
        raise ValueError("pattern %r is not a regular expression" % pat)


def parse(props):
    """setup() (:141-519): [("R", type, key, val) | ("C", type, a, b|None, accessor)], or ValueError where cb_init refuses"""
    items, nr, nc = [], 0, 0
    for name, val in props:
        name = name.decode() if isinstance(name, bytes) else name
        tok = split_quoted(val)
        if tok is None or len(tok) == 0 or len(tok) > 3:
            raise ValueError("Invalid config for %s" % name)
        if name.lower() == "condition":
            t = tok[0].decode("latin-1").lower()
            if t not in CONDS or len(tok) < 2:
                raise ValueError("Invalid config for %s" % name)
            ty = CONDS.index(t)
            a, b = tok[1], (tok[2] if len(tok) == 3 else None)
            if a_rx(ty):
                if not a:
                    raise ValueError("Unable to create regex")
                check_rx(a, True)
            if b_rx(ty):
                if not b:
                    raise ValueError("Unable to create regex")
                check_rx(b, True)
            ra = None if a_rx(ty) else accessor(a)
            nc += 1
            if nc > MAX_CONDS:
                raise ValueError("too many conditions")
            items.append(("C", ty, a, b, ra))
        else:
            ln = name.lower()
            known = ln in RULES1 or ln in RULES2
            ty = None
            if len(tok) == 1 and ln in RULES1:
                ty = RULES1[ln]
            elif len(tok) == 2 and ln in RULES2:
                ty = RULES2[ln]
            elif len(tok) == 3 and known:
                ty = RENAME
            if ty is None:
                raise ValueError("Invalid operation %s" % name)
            k, v = tok[0], tok[-1]
            if ty == REMOVE_REGEX and not k:
                raise ValueError("Unable to create regex")
            check_rx(k, ty == REMOVE_REGEX)
            check_rx(v, False)
            if ty == HARD_COPY and k == v:
                raise ValueError("Hard_copy onto itself")
            nr += 1
            if nr > MAX_RULES:
                raise ValueError("too many rules")
            items.append(("R", ty, k, v))
    return items


def describe(items):
    """the text flbgpu_modify_parse_check writes"""
    out = []
    for it in items:
        if it[0] == "R":
            out.append("R%d,%s,%s" % (it[1], it[2].hex(), it[3].hex()))
            continue
        _, ty, a, b, ra = it
        d = "C%d,%s,%s" % (ty, a.hex(), "-" if b is None else b.hex())
        if not a_rx(ty):
            if ra is None:
                d += ",N"
            else:
                d += ",K" + ra[0].hex() + "".join("/i%d" % x if k == "i" else "/s" + x.hex() for k, x in ra[1])
        out.append(d)
    return ";".join(out)


# ---------------------------------------------------------------- msgpack with spans
class Obj:
    __slots__ = ("t", "v", "start", "end", "pay")     # pay: payload start of STR / BIN

    def __init__(self, t, v, start, end, pay=None):
        self.t, self.v, self.start, self.end, self.pay = t, v, start, end, pay


class Bad(Exception):
    pass


def _need(buf, p, n):
    if p + n > len(buf):
        raise Bad()


def unpack(buf, p, depth=0):
    """one object at p -> Obj; Bad when truncated / malformed / nested past msgpack-c's 32 open containers"""
    _need(buf, p, 1)
    c, s = buf[p], p
    p += 1

    def be(n):
        _need(buf, p, n)
        return int.from_bytes(buf[p:p + n], "big")
    if c <= 0x7f:
        return Obj("uint", c, s, p)
    if c >= 0xe0:
        return Obj("int", c - 256, s, p)
    if 0xa0 <= c <= 0xbf or c in (0xd9, 0xda, 0xdb, 0xc4, 0xc5, 0xc6):
        if 0xa0 <= c <= 0xbf:
            n, h = c & 31, 0
        else:
            h = {0xd9: 1, 0xda: 2, 0xdb: 4, 0xc4: 1, 0xc5: 2, 0xc6: 4}[c]
            n = be(h)
        _need(buf, p + h, n)
        return Obj("bin" if c in (0xc4, 0xc5, 0xc6) else "str", bytes(buf[p + h:p + h + n]), s, p + h + n, p + h)
    if 0x90 <= c <= 0x9f or c in (0xdc, 0xdd) or 0x80 <= c <= 0x8f or c in (0xde, 0xdf):
        is_map = 0x80 <= c <= 0x8f or c in (0xde, 0xdf)
        if c <= 0x9f:
            n = c & 15
        else:
            h = 2 if c in (0xdc, 0xde) else 4
            n = be(h)
            p += h
        if depth >= 32:
            raise Bad()
        items = []
        for _ in range(n * (2 if is_map else 1)):
            o = unpack(buf, p, depth + 1)
            items.append(o)
            p = o.end
        if is_map:
            return Obj("map", [(items[2 * i], items[2 * i + 1]) for i in range(n)], s, p)
        return Obj("array", items, s, p)
    if c == 0xc0:
        return Obj("nil", None, s, p)
    if c in (0xc2, 0xc3):
        return Obj("bool", c == 0xc3, s, p)
    if c in (0xcc, 0xcd, 0xce, 0xcf):
        n = 1 << (c - 0xcc)
        return Obj("uint", be(n), s, p + n)
    if c in (0xd0, 0xd1, 0xd2, 0xd3):
        n = 1 << (c - 0xd0)
        v = be(n)
        if v >= 1 << (8 * n - 1):
            v -= 1 << (8 * n)
        return Obj("uint" if v >= 0 else "int", v, s, p + n)
    if c == 0xca:
        _need(buf, p, 4)
        return Obj("f32", bytes(buf[p:p + 4]), s, p + 4)
    if c == 0xcb:
        _need(buf, p, 8)
        return Obj("f64", bytes(buf[p:p + 8]), s, p + 8)
    if 0xd4 <= c <= 0xd8 or c in (0xc7, 0xc8, 0xc9):
        if c >= 0xd4:
            n, h = 1 << (c - 0xd4), 0
        else:
            h = {0xc7: 1, 0xc8: 2, 0xc9: 4}[c]
            n = be(h)
        _need(buf, p + h, 1 + n)
        return Obj("ext", (buf[p + h], bytes(buf[p + h + 1:p + h + 1 + n])), s, p + h + 1 + n)
    raise Bad()


def pack_str_hdr(n, bin_=False):
    if bin_:
        return bytes([0xc4, n]) if n < 256 else (b"\xc5" + struct.pack(">H", n) if n < 65536 else b"\xc6" + struct.pack(">I", n))
    if n < 32:
        return bytes([0xa0 | n])
    return bytes([0xd9, n]) if n < 256 else (b"\xda" + struct.pack(">H", n) if n < 65536 else b"\xdb" + struct.pack(">I", n))


def pack_hdr(n, base, b16, b32):
    return bytes([base | n]) if n < 16 else (bytes([b16]) + struct.pack(">H", n) if n < 65536 else bytes([b32]) + struct.pack(">I", n))


def canon(o):
    """msgpack_pack_object (lib/msgpack-c/src/objectc.c:39-126)"""
    t, v = o.t, o.v
    if t == "nil":
        return b"\xc0"
    if t == "bool":
        return b"\xc3" if v else b"\xc2"
    if t == "uint":
        if v < 128:
            return bytes([v])
        for c, n in ((0xcc, 1), (0xcd, 2), (0xce, 4), (0xcf, 8)):
            if v < 1 << (8 * n):
                return bytes([c]) + v.to_bytes(n, "big")
    if t == "int":
        if v >= -32:
            return bytes([v & 0xff])
        for c, n in ((0xd0, 1), (0xd1, 2), (0xd2, 4), (0xd3, 8)):
            if v >= -(1 << (8 * n - 1)):
                return bytes([c]) + (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")
    if t == "f32":
        return b"\xca" + v
    if t == "f64":
        return b"\xcb" + v
    if t in ("str", "bin"):
        return pack_str_hdr(len(v), t == "bin") + v
    if t == "ext":
        et, d = v
        n = len(d)
        fx = {1: 0xd4, 2: 0xd5, 4: 0xd6, 8: 0xd7, 16: 0xd8}
        if n in fx:
            h = bytes([fx[n]])
        elif n < 256:
            h = bytes([0xc7, n])
        elif n < 65536:
            h = b"\xc8" + struct.pack(">H", n)
        else:
            h = b"\xc9" + struct.pack(">I", n)
        return h + bytes([et]) + d
    if t == "array":
        return pack_hdr(len(v), 0x90, 0xdc, 0xdd) + b"".join(canon(x) for x in v)
    if t == "map":
        return pack_hdr(len(v), 0x80, 0xde, 0xdf) + b"".join(canon(k) + canon(x) for k, x in v)
    raise AssertionError(t)


def S(b):
    return Obj("str", b, None, None)


# ---------------------------------------------------------------- one record
class Ctx:
    def __init__(self, buf):
        self.buf = buf            # the CURRENT buffer: the record, then each re-pack
        self.overread = False


def m_str(o, s):
    return o.t in ("str", "bin") and o.v == s


def m_rx(o, rx):
    if o.t == "bool":
        return rx.search(b"true" if o.v else b"false")
    return o.t == "str" and rx.search(o.v)


def m_prefix(ctx, o, s):
    """strncmp(s, key, len(s)) on the current buffer (:599-616)"""
    if o.t not in ("str", "bin"):
        return False
    L = len(s)
    if len(o.v) >= L:
        return o.v[:L] == s
    if o.v != s[:len(o.v)]:
        return False
    p = o.pay + len(o.v)
    for i in range(L - len(o.v)):
        if p + i >= len(ctx.buf):
            ctx.overread = True
            return False
        if ctx.buf[p + i] != s[len(o.v) + i]:
            return False
    return True


def ra_get(ra, m):
    """flb_ra_get_kv_pair: the value, or None when a key / value / key object is missing"""
    if ra is None:
        return None
    key, subs = ra
    val = None
    for k, v in m.v:
        if k.t == "str" and k.v == key:
            val = v
    if val is None:
        return None
    if val.t in ("map", "array") and subs:
        cur, matched, last_is_index = val, 0, False
        for kind, x in subs:
            if kind == "i":
                if cur.t != "array" or x >= len(cur.v):
                    return None
                cur = cur.v[x]
                matched += 1
                last_is_index = True
                if matched == len(subs):
                    break
                continue
            if cur.t != "map":
                break
            hit = None
            for k, v in cur.v:
                if k.t == "str" and k.v == x:
                    hit = v
            if hit is None:
                continue
            cur = hit
            matched += 1
            last_is_index = False
            if matched == len(subs):
                break
        if matched == 0 or matched != len(subs) or last_is_index:
            return None
        return cur
    return val


def cond(m, c):
    _, ty, a, b, ra = c
    if ty in (2, 3):
        rx = Regex.get(a)
        any_ = any(m_rx(k, rx) for k, _ in m.v)
        return any_ if ty == 2 else not any_
    if ty in (8, 9):
        ra_, rb_ = Regex.get(a), Regex.get(b)
        ok = True
        for k, v in m.v:
            if m_rx(k, ra_) and not m_rx(v, rb_):
                ok = False
                break
        return ok if ty == 8 else not ok
    v = ra_get(ra, m)
    if ty == 0:
        return v is not None
    if ty == 1:
        return v is None
    if v is None:
        return False
    if ty in (4, 5):
        eq = v.t in ("str", "bin") and v.v == (b or b"")
        return eq if ty == 4 else not eq
    mt = m_rx(v, Regex.get(b))
    return mt if ty == 6 else not mt


def rule(ctx, m, r):
    """apply_modifying_rule: the new map's entries, or None (NOTOUCH)"""
    _, ty, k, v = r
    E = m.v
    nk = sum(1 for kk, _ in E if m_str(kk, k))
    nv = sum(1 for kk, _ in E if m_str(kk, v))
    if ty == RENAME:
        if nk == 0 or nv > 0:
            return None
        return [(S(v) if m_str(kk, k) else kk, vv) for kk, vv in E]
    if ty == HARD_RENAME:
        if nk == 0:
            return None
        if nv == 0:
            return [(S(v) if m_str(kk, k) else kk, vv) for kk, vv in E]
        return [(S(v) if m_str(kk, k) else kk, vv) for kk, vv in E if not m_str(kk, v)]
    if ty in (COPY, HARD_COPY):
        if nk != 1 or (ty == COPY and nv > 0) or nv > 1:
            return None
        out = []
        for kk, vv in E:
            if ty == HARD_COPY and nv == 1 and m_str(kk, v):
                continue
            out.append((kk, vv))
            if m_str(kk, k):
                out.append((S(v), vv))
        return out
    if ty == ADD:
        return None if nk else E + [(S(k), S(v))]
    if ty == SET:
        return [(kk, vv) for kk, vv in E if not m_str(kk, k)] + [(S(k), S(v))]
    if ty == REMOVE:
        return [(kk, vv) for kk, vv in E if not m_str(kk, k)] if nk else None
    if ty in (REMOVE_WILDCARD, MOVE_TO_START, MOVE_TO_END, REMOVE_REGEX):
        if ty == REMOVE_REGEX:
            rx = Regex.get(k)
            hit = [m_rx(kk, rx) for kk, _ in E]
        else:
            hit = [m_prefix(ctx, kk, k) for kk, _ in E]
        if not any(hit):
            return None
        keep = [e for e, h in zip(E, hit) if not h]
        moved = [e for e, h in zip(E, hit) if h]
        if ty == REMOVE_WILDCARD or ty == REMOVE_REGEX:
            return keep
        return moved + keep if ty == MOVE_TO_START else keep + moved
    raise AssertionError(ty)


def decode_event(buf, p):
    """flb_log_event_decoder_next on buf[p:]: (end, skip, sec, nsec, meta|None, body) or raises Bad"""
    root = unpack(buf, p)
    if root.t != "array" or len(root.v) != 2:
        raise Bad()
    h, body = root.v
    meta = None
    if h.t == "array":
        if len(h.v) != 2 or h.v[1].t != "map":
            raise Bad()
        ts, meta = h.v
    else:
        ts = h
    if body.t != "map":
        raise Bad()
    if ts.t == "uint":
        sec, nsec = ts.v if ts.v < 1 << 63 else ts.v - (1 << 64), 0
    elif ts.t == "f64":
        f = struct.unpack(">d", ts.v)[0]
        sec = int(f)
        nsec = int((f - sec) * 1000000000)
    elif ts.t == "ext":
        et, d = ts.v
        if et != 0 or len(d) != 8:
            raise Bad()
        s, ns = struct.unpack(">II", d)
        if s in (0xffffffff, 0xfffffffe):
            if ns:
                raise Bad()
            sec, nsec = (-1 if s == 0xffffffff else -2), 0
        else:
            if ns >= 1000000000:
                raise Bad()
            sec, nsec = s, ns
    else:
        raise Bad()
    return root.end, sec < 0, sec, nsec, meta, body


def record(raw, conds, rules, stats):
    """apply_modifying_rules on one record's bytes: the output bytes and whether it was rebuilt"""
    end, skip, sec, nsec, meta, body = decode_event(raw, 0)
    assert end == len(raw)
    ctx = Ctx(raw)
    m = body
    verdicts = [cond(body, c) for c in conds]
    for c, v in zip(conds, verdicts):
        key = "cond_true" if v else "cond_false"
        stats.setdefault(key, {})[c[1]] = stats.setdefault(key, {}).get(c[1], 0) + 1
    if not all(verdicts):
        return raw, False
    applied = False
    for r in rules:
        e = rule(ctx, m, r)
        if e is None:
            continue
        applied = True
        stats.setdefault("rule_applied", {})[r[1]] = stats.setdefault("rule_applied", {}).get(r[1], 0) + 1
        ctx.buf = canon(Obj("map", e, None, None))
        m = unpack(ctx.buf, 0)
    if ctx.overread:
        stats["overread"] = stats.get("overread", 0) + 1
    if not applied or sec > 0xffffffff or nsec < 0 or nsec >= 1000000000:
        return raw, False
    return b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + (canon(meta) if meta is not None else b"\x80") + canon(m), True


def clean_cut(buf, p):
    """whether the bytes from p on, which hold no whole object, end where msgpack-c's executor has consumed all it was given: it takes
    whole fields (a type byte, a length field, a payload) and stops in front of the first one that is cut short
    (lib/msgpack-c/include/msgpack/unpack_template.h:242-247,439-447).  The decoder's offset then stands at the end of the buffer and
    cb_modify_filter reads its INSUFFICIENT_DATA as a clean end (:1550-1553)"""
    n, count = len(buf), []
    while True:
        if p >= n:
            return True
        c, q = buf[p], p + 1
        k, lb, items = 0, 0, None
        if c <= 0x7f or c >= 0xe0 or c in (0xc0, 0xc2, 0xc3):
            pass
        elif c == 0xc1:
            return False
        elif 0xa0 <= c <= 0xbf:
            k = c & 31
        elif 0x90 <= c <= 0x9f:
            items = c & 15
        elif 0x80 <= c <= 0x8f:
            items = 2 * (c & 15)
        elif c in (0xcc, 0xd0):
            k = 1
        elif c in (0xcd, 0xd1, 0xd4):
            k = 2
        elif c in (0xce, 0xd2, 0xca):
            k = 4
        elif c in (0xcf, 0xd3, 0xcb):
            k = 8
        elif c in (0xd5, 0xd6, 0xd7, 0xd8):
            k = {0xd5: 3, 0xd6: 5, 0xd7: 9, 0xd8: 17}[c]
        else:
            lb = 1 if c in (0xc4, 0xc7, 0xd9) else (2 if c in (0xc5, 0xc8, 0xda, 0xdc, 0xde) else 4)
            if n - q < lb:
                return q == n
            v = int.from_bytes(buf[q:q + lb], "big")
            q += lb
            if c in (0xdc, 0xdd):
                items = v
            elif c in (0xde, 0xdf):
                items = 2 * v
            else:
                k = v + (1 if c in (0xc7, 0xc8, 0xc9) else 0)
        if items is None and n - q < k:
            return q == n
        p = q + k
        if items is not None:
            if len(count) >= 32:
                return False
            if items > 0:
                count.append(items)
                continue
        while True:
            if not count:
                return False                   # a whole object after all: it is malformed, not cut
            count[-1] -= 1
            if count[-1] > 0:
                break
            count.pop()


def processor_output(buf):
    """what the reference's processor hands on of the buffer a filter unit left (flb_mp_normalize_log_buffer_groups_msgpack,
    src/flb_mp.c:80-230, called at src/flb_processor.c:1811-1825): the records its decoder takes up to the first error, without a
    group start that is never closed, a group end that has no start and a group that holds no record.  tools/gen_modify_golden.py
    records behind it, so a rebuilt record whose time is 0xffffffff s -- a group start to this decoder -- is not in the recording."""
    ent, p = [], 0
    while p < len(buf):
        try:
            end, skip, sec, *_ = decode_event(buf, p)
        except Bad:
            break
        ent.append([p, end, (sec if skip else 0), True])
        p = end
    stack = []
    for e in ent:
        if e[2] == -1:
            stack.append([e, False])
        elif e[2] == -2:
            if not stack:
                e[3] = False
                continue
            start, content = stack.pop()
            if not content:
                start[3] = e[3] = False
            elif stack:
                stack[-1][1] = True
        elif stack:
            stack[-1][1] = True
    for start, _ in stack:
        start[3] = False
    return b"".join(buf[a:b] for a, b, _, keep in ent if keep)


class Model:
    """cb_modify_filter over a chunk: filter(data) -> (MODIFIED|NOTOUCH, bytes|None), counts() as flbgpu_filter_last_counts"""
    MODIFIED, NOTOUCH = 1, 2                  # FLB_FILTER_MODIFIED, FLB_FILTER_NOTOUCH

    def __init__(self, props):
        items = parse(props)
        self.conds = [x for x in items if x[0] == "C"]
        self.rules = [x for x in items if x[0] == "R"]
        self.stats = {}
        self.n_in = 0

    def filter(self, data):
        p, out, mod, bad, n = 0, [], 0, False, 0
        while p < len(data):
            try:
                end, skip, *_ = decode_event(data, p)
            except Bad:
                bad = not clean_cut(data, p)
                break
            if skip:
                p = end
                continue
            n += 1
            o, m = record(bytes(data[p:end]), self.conds, self.rules, self.stats)
            out.append(o)
            mod += m
            self.stats["rebuilt" if m else "raw"] = self.stats.get("rebuilt" if m else "raw", 0) + 1
            p = end
        self.n_in = n
        if mod == 0 or bad:
            return self.NOTOUCH, None
        return self.MODIFIED, b"".join(out)

    def counts(self):
        return self.n_in, self.n_in

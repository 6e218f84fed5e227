"""CPU model of filter_checklist (plugins/filter_checklist/checklist.c), restated on the msgpack walker of tests/modify_model.py: the
config map and init_config (:198-267, :601-640), the list loader as fgets(buf, 2047) cuts the file (:130-196), both lookups -- byte
equality for mode exact, SQLite's LIKE (patternCompare with its own UTF-8 reader, case_sensitive_like on) for mode partial --, the
record writer (set_record :291-409) and one call with its raw spans (:411-582).  The model is the yardstick of
tests/test_checklist_*.py and does not use the product."""
import struct

import modify_model as mm
import typeconv_model as tcm

MAX_RECORDS, MAX_TABLE_BYTES, MAX_KEY, LINE = 64, 32768, 128, 2048
EXACT, PARTIAL = 0, 1
OK, NO_FILE, CANNOT_OPEN, STOPPED = range(4)


def fold_bytes(b):
    """tolower in the C locale: A-Z only"""
    return bytes(c + 32 if 0x41 <= c <= 0x5a else c for c in b)


def bool_of(v):
    v = v.lower()
    if v in (b"true", b"on", b"yes"):
        return 1
    if v in (b"false", b"off", b"no"):
        return 0
    raise ValueError("invalid boolean %r" % v)


def load_list(data, fold):
    """load_file_patterns over the file's bytes: (entries, status, line the load stopped at).  ValueError: a piece that begins with a
    NUL byte, where the reference reads buf[-1]"""
    entries, pos, line = [], 0, 0
    while pos < len(data):
        piece = data[pos:pos + LINE - 2]                      # fgets(buf, 2047): at most 2046 bytes, up to and with a '\n'
        nl = piece.find(b"\n")
        if nl >= 0:
            piece = piece[:nl + 1]
        eof = nl < 0 and len(piece) < LINE - 2                # the end-of-file mark: only a read that ran out of bytes sets it
        pos += len(piece)
        buf = piece.split(b"\0")[0]                           # strlen
        if not buf:
            raise ValueError("NUL at the start of a line")
        if buf.endswith(b"\n"):
            buf = buf[:-1]
            if buf.endswith(b"\r"):
                buf = buf[:-1]
        elif not eof:
            return entries, STOPPED, line
        if not buf or buf[:1] == b"#":
            line += 1
            continue
        entries.append(fold_bytes(buf) if fold else buf)
        line += 1
    return entries, OK, 0


class Config:
    pass


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def value_kind(v):
    return {b"true": "t", b"false": "f", b"null": "n"}.get(v.lower(), "s")


def parse(props, files=None):
    """the configuration and the loaded list; ValueError where the filter does not start or create refuses.  files: {path: bytes}
    stands in for the file system (a path it does not hold cannot be opened); None: the real one"""
    c = Config()
    c.fold, c.records, lookup, mode, file_ = 0, [], b"log", None, None
    seen = set()
    for name, val in props:
        name, val = _b(name).lower().decode(), _b(val).split(b"\0")[0]
        if name != "record":                                  # no FLB_CONFIG_MAP_MULT: set twice fails the check of the properties
            if name in seen:
                raise ValueError("%s is set more than once" % name)
            seen.add(name)
        if name == "file":
            file_ = val
        elif name == "lookup_key":
            lookup = val
        elif name == "mode":
            mode = val
        elif name in ("ignore_case", "print_query_time"):
            b = bool_of(val)
            if name == "ignore_case":
                c.fold = b
        elif name == "record":
            tok = tcm.split_tokens(val, 2)
            if len(tok) < 2:                                  # SLIST_2: the config map's size check
                raise ValueError("record needs two entries")
            c.records.append((tok[0], tok[-1]))               # the first entry and the LAST one (:339-340)
        else:
            raise ValueError("unknown property %s" % name)
    if len(c.records) > MAX_RECORDS:
        raise ValueError("too many record entries")
    c.mode = PARTIAL if mode is not None and mode.lower() == b"partial" else EXACT
    if b"${" in lookup:
        raise ValueError("environment variables are not translated")
    try:
        c.ra = tcm.accessor(lookup)
    except tcm.Skip:
        raise ValueError("the record accessor refuses the lookup_key")
    if table_bytes(c) > MAX_TABLE_BYTES:
        raise ValueError("table too large")
    c.entries, c.status, c.stop_line = [], OK, 0
    if file_ is None:
        c.status = NO_FILE
        return c
    if files is not None:
        data = files.get(file_)
    else:
        try:
            with open(file_, "rb") as f:
                data = f.read()
        except OSError:
            data = None
    if data is None:
        c.status = CANNOT_OPEN
        return c
    c.entries, c.status, c.stop_line = load_list(data, c.fold)
    return c


def pack_str(b):
    return mm.pack_str_hdr(len(b)) + b


def record_bytes(k, v):
    kind = value_kind(v)
    return pack_str(k) + {"t": b"\xc3", "f": b"\xc2", "n": b"\xc0"}.get(kind, pack_str(v) if kind == "s" else b"")


def table_bytes(c):
    def pad4(x):
        return (x + 3) // 4 * 4
    key, subs = c.ra if c.ra else (b"", [])
    n = 16 + 16 * len(c.records) + 8 * len(subs) + sum(pad4(len(x)) for k, x in subs if k == "s") + pad4(len(key))
    return n + sum(pad4(len(k)) + pad4(len(record_bytes(k, v))) for k, v in c.records)


def digest(entries):
    h = 0xcbf29ce484222325
    for e in entries:
        for b in struct.pack("<I", len(e)) + e:
            h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def slot_count(c, dense=False):
    """mode exact: a power of two of slots, load factor <= 1/2 -- or, under FLBGPU_CHECKLIST_DENSE=1, the smallest above the entry count"""
    if c.mode != EXACT:
        return 0
    want, n = (len(c.entries) + 1 if dense else 2 * len(c.entries)), 1
    while n < want:
        n *= 2
    return n


def describe(c, dense=False):
    """the text flbgpu_checklist_parse_check writes"""
    if c.ra is None:
        k = "-"
    else:
        k = "K" + c.ra[0].hex() + "".join("[%d]" % x if kind == "i" else "." + x.hex() for kind, x in c.ra[1])
    recs = ",".join("K%s:%s%s" % (rk.hex(), value_kind(rv), rv.hex() if value_kind(rv) == "s" else "") for rk, rv in c.records)
    load = {OK: "ok", NO_FILE: "no file", CANNOT_OPEN: "cannot open", STOPPED: "stopped at line %d" % c.stop_line}[c.status]
    return "mode=%s;fold=%d;key=%s;records=%s;entries=%d;slots=%d;load=%s;digest=%016x" % (
        "partial" if c.mode == PARTIAL else "exact", c.fold, k, recs, len(c.entries), slot_count(c, dense), load, digest(c.entries))


# ---------------------------------------------------------------- SQLite's LIKE
def u8read(z, i):
    """sqlite3Utf8Read on the NUL-terminated z at i: (character, next index)"""
    c = z[i]
    i += 1
    if c >= 0xc0:
        c = c & 0x1f if c < 0xe0 else c & 0x0f if c < 0xf0 else c & 0x07 if c < 0xf8 else c & 0x03 if c < 0xfc else c & 0x01 if c < 0xfe else 0
        while z[i] & 0xc0 == 0x80:
            c = ((c << 6) + (z[i] & 0x3f)) & 0xFFFFFFFF
            i += 1
        if c < 0x80 or c & 0xFFFFF800 == 0xD800 or c & 0xFFFFFFFE == 0xFFFE:
            c = 0xFFFD
    return c, i


MATCH, NOMATCH, NOWILDCARDMATCH = 0, 1, 2


def pattern_compare(pat, pi, s, si):
    """patternCompare with matchAll '%', matchOne '_', no escape, noCase off; pat and s end with a NUL"""
    while True:
        c, pi = u8read(pat, pi)
        if c == 0:
            break
        if c == 0x25:
            while True:
                c, pi = u8read(pat, pi)
                if c == 0x25:
                    continue
                if c == 0x5f:
                    c2, si = u8read(s, si)
                    if c2 == 0:
                        return NOWILDCARDMATCH
                    continue
                break
            if c == 0:
                return MATCH
            if c <= 0x80:
                while True:                                   # strcspn: the raw byte
                    while s[si] != 0 and s[si] != c:
                        si += 1
                    if s[si] == 0:
                        break
                    si += 1
                    r = pattern_compare(pat, pi, s, si)
                    if r != NOMATCH:
                        return r
            else:
                while True:
                    c2, si = u8read(s, si)
                    if c2 == 0:
                        break
                    if c2 != c:
                        continue
                    r = pattern_compare(pat, pi, s, si)
                    if r != NOMATCH:
                        return r
            return NOWILDCARDMATCH
        c2, si = u8read(s, si)
        if c == c2:
            continue
        if c == 0x5f and c2 != 0:
            continue
        return NOMATCH
    return MATCH if s[si] == 0 else NOMATCH


def like(value, entry):
    """value LIKE (entry || '%') with case_sensitive_like on; the value ends at its first NUL"""
    return pattern_compare(bytes(entry) + b"%\0\0", 0, bytes(value).split(b"\0")[0] + b"\0\0", 0) == MATCH


# ---------------------------------------------------------------- one call
def ra_value(ra, m):
    """flb_ra_get_value_object: the last top-level entry whose key is a STR equal to the name, then the sub-keys through maps and
    arrays; a path may end on an array index"""
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
        cur, matched = val, 0
        for kind, x in subs:
            if kind == "i":
                if cur.t != "array" or x >= len(cur.v):
                    return None
                cur = cur.v[x]
                matched += 1
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
            if matched == len(subs):
                break
        if matched != len(subs):
            return None
        return cur
    return val


class Model:
    """cb_checklist_filter over a chunk: filter(data) -> (MODIFIED|NOTOUCH, bytes|None), counts() as flbgpu_filter_last_counts,
    counters() as flbgpu_checklist_counters (since the model was created)"""
    MODIFIED, NOTOUCH = 1, 2

    def __init__(self, props, files=None):
        self.cfg = parse(props, files)
        self.set = set(self.cfg.entries)
        self.stats = [0, 0, 0, 0]                 # matched, rolled back, non-STR values, size/emit mismatches (the model has none)
        self.n_in = self.n_out = 0

    def found(self, body):
        v = ra_value(self.cfg.ra, body)
        if v is None:
            return False
        if v.t != "str":
            self.stats[2] += 1
            return False
        val = fold_bytes(v.v) if self.cfg.fold else v.v
        if self.cfg.mode == EXACT:
            return len(val) > 0 and val in self.set           # flb_hash_table_get refuses key_len <= 0
        return any(like(val, e) for e in self.cfg.entries)

    def set_record(self, sec, nsec, meta, body):
        """the record as the encoder writes it, or None where it refuses (the time: set_record's -2)"""
        if not (0 <= sec <= 0xffffffff and 0 <= nsec < 1000000000):
            return None
        keys = [k for k, _ in self.cfg.records]
        out = [mm.canon(k) + mm.canon(v) for k, v in body.v if k.t == "str" and k.v not in keys]
        out += [record_bytes(k, v) for k, v in self.cfg.records]
        head = b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + (mm.canon(meta) if meta is not None else b"\x80")
        return head + b"\xdf" + struct.pack(">I", len(out)) + b"".join(out)

    def filter(self, data):
        data = bytes(data)
        p = pre = 0
        out = bytearray()
        n = n_out = matches = 0
        while p < len(data):
            try:
                end, skip, sec, nsec, meta, body = mm.decode_event(data, p)
            except mm.Bad:
                break
            p = end
            if skip:                                          # the decoder steps over it: its bytes stay in front of `pre`'s successor
                continue
            n += 1
            if self.found(body):
                if not out and pre > 0:
                    out += data[:pre]
                    n_out += n - 1
                rec = self.set_record(sec, nsec, meta, body)
                if rec is None:
                    self.stats[1] += 1
                else:
                    out += rec
                    n_out += 1
                matches += 1
            elif out:
                out += data[pre:end]
                n_out += 1
            pre = end
        self.stats[0] += matches
        self.n_in = n
        if out and matches:
            self.n_out = n_out
            return self.MODIFIED, bytes(out)
        self.n_out = n
        return self.NOTOUCH, None

    def counts(self):
        return self.n_in, self.n_out

    def counters(self):
        return tuple(self.stats)

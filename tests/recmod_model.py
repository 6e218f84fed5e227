"""CPU model of filter_record_modifier (plugins/filter_record_modifier/filter_modifier.c), restated on the msgpack walker of
tests/modify_model.py: the config map and configure() (:69-155, :499-529), make_bool_map (:213-279) and one call with its drops and
return codes (:298-486).  The model is the yardstick of tests/test_recmod_*.py; it does not use the product."""
import struct

import modify_model as mm

MAX_RECORDS, MAX_KEYS, MAX_KEY_BYTES = 64, 64, 32768
NONE, REMOVE, ALLOW = 0, 1, 2
BOOL_MAP_LIMIT = 65535


# ---------------------------------------------------------------- configuration
def _token(s, pos):
    """token_retrieve (src/flb_slist.c:107-180): (token | None, next position | None when the line has ended)"""
    n = len(s)
    p = pos
    while p < n and s[p] == 0x20:
        p += 1
    start, quoted = p, False
    if p < n and s[p] == 0x22:
        quoted = True
        p += 1
        start = p
        while True:
            while p < n and s[p] != 0x22:
                p += 1
            if p >= n:
                break
            if s[p - 1] == 0x5c:
                p += 1
                continue
            break
    else:
        while p < n and s[p] != 0x20:
            p += 1
    if p < n:
        tok = s[start:p]
        if quoted:
            tok = tok.replace(b'\\"', b'"')
        p += 1
        while p < n and s[p] == 0x20:
            p += 1
        return tok, p
    return (s[start:] if p > start else None), None


def split_tokens2(val):
    """flb_slist_split_tokens(list, val, 2) (src/flb_slist.c:182-217)"""
    s = val.encode() if isinstance(val, str) else val
    s = s.split(b"\0")[0]
    out, pos, count = [], 0, 0
    while True:
        tok, pos = _token(s, pos)
        if tok is None:
            break
        out.append(tok)
        if pos is None:
            break
        count += 1
        if count >= 2:
            rest = s[pos:].lstrip(b" ")
            if rest:
                out.append(rest)
            break
    return out


def parse(props):
    """(list kind, [(key, is_prefix), ...], [(key, value), ...]); ValueError where the filter does not start or create refuses"""
    remove, allow, white, records = [], [], [], []
    for name, val in props:
        name = (name.decode() if isinstance(name, bytes) else name).lower()
        v = val.encode() if isinstance(val, str) else val
        v = v.split(b"\0")[0]
        if name == "record":
            tok = split_tokens2(v)
            if len(tok) < 2:                  # the config map's size check for SLIST_2 (src/flb_config_map.c:32-59)
                raise ValueError("Record needs KEY VALUE")
            if len(tok) > 2:                  # configure() skips it with a message (:96-101)
                continue
            records.append((tok[0], tok[1]))
            if len(records) > MAX_RECORDS:
                raise ValueError("too many Record entries")
            continue
        if name == "uuid_key":
            raise ValueError("Uuid_key is refused")
        dst = {"remove_key": remove, "allowlist_key": allow, "whitelist_key": white}.get(name)
        if dst is None:
            raise ValueError("unknown property %s" % name)
        if not v:
            raise ValueError("empty key")
        dst.append((v[:-1], True) if v.endswith(b"*") else (v, False))
    allow = allow + white
    if remove and allow:
        raise ValueError("remove_keys and allowlist_keys are exclusive")
    keys = remove or allow
    if len(keys) > MAX_KEYS:
        raise ValueError("too many key entries")
    if sum((len(k) + 3) // 4 * 4 for k, _ in keys) > MAX_KEY_BYTES:
        raise ValueError("key entries too long")
    return (REMOVE if remove else ALLOW if allow else NONE), keys, records


def describe(prog):
    """the text flbgpu_record_modifier_parse_check writes"""
    kind, keys, records = prog
    out = [("none", "remove", "allow")[kind]]
    out += ["K%s,%s" % ("p" if pre else "e", k.hex()) for k, pre in keys]
    out += ["R%s,%s" % (k.hex(), v.hex()) for k, v in records]
    return ";".join(out)


# ---------------------------------------------------------------- one call
def _lower(b):
    """tolower in the C locale: ASCII only"""
    return bytes(c | 0x20 if 0x41 <= c <= 0x5a else c for c in b)


def _strncasecmp_eq(key, entry, n):
    for i in range(n):
        a, b = _lower(key[i:i + 1]), _lower(entry[i:i + 1])
        if a != b:
            return False
        if a == b"\0":
            return True
    return True


def matches(key, keys):
    """make_bool_map's inner loop (:248-270) for one key object"""
    if key.t not in ("str", "bin"):
        return False
    for k, pre in keys:
        if not pre and len(key.v) != len(k):
            continue
        if pre and len(key.v) < len(k):
            continue
        if _strncasecmp_eq(key.v, k, len(k)):
            return True
    return False


class Model:
    """cb_modifier_filter over a chunk: filter(data) -> (MODIFIED|NOTOUCH|-1, bytes|None), counts() as flbgpu_filter_last_counts"""
    MODIFIED, NOTOUCH = 1, 2

    def __init__(self, props):
        self.kind, self.keys, self.records = parse(props)
        self.tail = b"".join(mm.pack_str_hdr(len(k)) + k + mm.pack_str_hdr(len(v)) + v for k, v in self.records)
        self.n_in = self.n_out = 0

    def filter(self, data):
        p, out, is_modified, n_in = 0, [], False, 0
        self.n_in = self.n_out = 0
        while p < len(data):
            try:
                end, skip, sec, nsec, meta, body = mm.decode_event(data, p)
            except mm.Bad:
                break                                     # the loop ends; what was encoded in front stays (:351-353)
            p = end
            if skip:
                continue
            n_in += 1
            if len(body.v) > BOOL_MAP_LIMIT:
                return -1, None
            if self.kind == NONE:
                kept = body.v
            else:
                kept = [(k, v) for k, v in body.v if matches(k, self.keys) != (self.kind == REMOVE)]
            if len(kept) != len(body.v):
                is_modified = True
            total = len(kept) + len(self.records)
            if total <= 0:
                continue
            if self.records:
                is_modified = True
            # the body is a dynamic field of the encoder: its map header is always map32 (flb_mp_map_header_init, src/flb_mp.c:591-603)
            # set_timestamp refuses a time outside the EventTime range and its answer is dropped: the zero time goes out
            if not (0 <= sec <= 0xffffffff and 0 <= nsec < 1000000000):
                sec, nsec = 0, 0
            out.append(b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + (mm.canon(meta) if meta is not None else b"\x80") +
                       b"\xdf" + struct.pack(">I", total) + b"".join(mm.canon(k) + mm.canon(v) for k, v in kept) + self.tail)
        self.n_in = n_in
        if is_modified and out:
            self.n_out = len(out)
            return self.MODIFIED, b"".join(out)
        self.n_out = n_in
        return self.NOTOUCH, None

    def counts(self):
        return self.n_in, self.n_out

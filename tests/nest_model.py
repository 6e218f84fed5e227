"""CPU model of filter_nest (plugins/filter_nest/nest.c), restated on the msgpack walker of tests/modify_model.py: the config map and
configure() (:57-175, :729-761), is_kv_to_nest (:298-345), is_kv_to_lift (:353-397), the two rules (:473-606) and one call with its
raw rows, lost rows and return codes (:631-717).  The model is the yardstick of tests/test_nest_*.py; it does not use the product."""
import struct

import modify_model as mm

MAX_WILDCARDS, MAX_KEY_BYTES = 64, 32768
NEST, LIFT = 1, 2
ADD, REMOVE = 1, 2


# ---------------------------------------------------------------- configuration
class Program:
    def __init__(self):
        self.op, self.wild, self.key, self.pfx, self.prefix = 0, [], None, 0, b""


def parse(props):
    """Program; ValueError where the filter does not start or create refuses"""
    pg = Program()
    add = remove = False
    once = set()
    for name, val in props:
        name = (name.decode() if isinstance(name, bytes) else name).lower()
        if name != "wildcard":                # the config map lets only Wildcard repeat (FLB_CONFIG_MAP_MULT, :735-739)
            if name in once:
                raise ValueError("%s is set 2 times" % name)
            once.add(name)
        v = val.encode() if isinstance(val, str) else val
        v = v.split(b"\0")[0]
        if name == "operation":
            if v[:4] == b"nest":              # strncmp(val, "nest", 4), with its case (:85-96)
                pg.op = NEST
            elif v[:4] == b"lift":
                pg.op = LIFT
            else:
                raise ValueError("Operation %r" % v)
        elif name == "wildcard":
            if not v:                         # the reference reads key[-1] (:115)
                raise ValueError("empty Wildcard")
            pg.wild.append((v[:-1], True) if v.endswith(b"*") else (v, False))
            if len(pg.wild) > MAX_WILDCARDS:
                raise ValueError("too many Wildcard entries")
        elif name in ("nest_under", "nested_under"):
            pg.key = v
        elif name == "add_prefix":
            pg.prefix, add = v, True
        elif name == "remove_prefix":
            pg.prefix, remove = v, True
        else:                                 # Prefix_with too: the config map does not know it
            raise ValueError("unknown property %s" % name)
    if add and remove:
        raise ValueError("Add_prefix and Remove_prefix are exclusive")
    if not pg.op:                             # the reference reads an uninitialised field (:161-165)
        raise ValueError("Operation is missing")
    pg.pfx = ADD if add else REMOVE if remove else 0

    def pad4(n):
        return (n + 3) // 4 * 4
    if sum(pad4(len(k)) for k, _ in pg.wild) + pad4(len(pg.key or b"")) + pad4(len(pg.prefix)) > MAX_KEY_BYTES:
        raise ValueError("wildcards, key and prefix too long")
    return pg


def describe(pg):
    """the text flbgpu_nest_parse_check writes"""
    out = ["nest" if pg.op == NEST else "lift", "K-" if pg.key is None else "K" + pg.key.hex(),
           "P%s,%s" % ("nar"[pg.pfx], pg.prefix.hex())]
    out += ["W%s,%s" % ("p" if pre else "e", k.hex()) for k, pre in pg.wild]
    return ";".join(out)


# ---------------------------------------------------------------- one record
class Rec:
    """one record's bytes and what the compares on it counted"""

    def __init__(self, buf):
        self.buf, self.overread, self.undef = buf, 0, False

    def cmp(self, key, entry):
        """strncmp(key, entry, len(entry)) == 0 on the record: the bytes behind a shorter key take part, a compare that would need
        bytes past the record fails and is counted (the convention of modify_model.m_prefix)"""
        L = len(entry)
        got = self.buf[key.pay:key.pay + L]
        if got != entry[:len(got)]:
            return False
        if len(got) < L:
            self.overread += 1
            return False
        return True


def to_nest(rc, pg, k):
    if k.t not in ("str", "bin"):
        return False
    for w, pre in pg.wild:
        if not pre and len(k.v) != len(w):
            continue
        if rc.cmp(k, w):
            return True
    return False


def to_lift(pg, k, v):
    return k.t in ("str", "bin") and k.v == (pg.key or b"") and v.t == "map"


def out_key(rc, pg, k):
    """the key of a nested or lifted entry (:177-216, :243-279, :421-453); b"" and rc.undef where the reference is undefined"""
    if not pg.pfx:
        return mm.canon(k)
    if k.t not in ("str", "bin"):
        rc.undef = True
        return b""
    if pg.pfx == ADD:
        s = pg.prefix + k.v
    elif rc.cmp(k, pg.prefix):
        if len(k.v) < len(pg.prefix):
            rc.undef = True
            return b""
        s = k.v[len(pg.prefix):]
    else:
        s = k.v
    return mm.pack_str_hdr(len(s)) + s


def map32(n):
    return b"\xdf" + struct.pack(">I", n)


def record(pg, raw, stats):
    """one record of the loop (:671-691): its output bytes (b"" when it is lost) and whether it was built again"""
    end, skip, sec, nsec, meta, body = mm.decode_event(raw, 0)
    rc = Rec(raw)
    lost = not (0 <= sec <= 0xffffffff and 0 <= nsec < 1000000000) or (pg.op == NEST and pg.key is None)
    stay, moved, nmatch, nmoved = [], [], 0, 0
    for k, v in body.v:
        if pg.op == NEST:
            if to_nest(rc, pg, k):
                nmatch += 1
                if not lost:
                    moved.append(out_key(rc, pg, k) + mm.canon(v))
            else:
                stay.append(mm.canon(k) + mm.canon(v))
        elif to_lift(pg, k, v):
            nmatch += 1
            if not lost:
                nmoved += len(v.v)
                moved += [out_key(rc, pg, ik) + mm.canon(iv) for ik, iv in v.v]
        else:
            stay.append(mm.canon(k) + mm.canon(v))
    stats[1] += rc.overread
    if nmatch == 0:
        return raw, False                     # emit_raw_record (:685-690): the bytes as they came
    if lost:
        return b"", False                     # begin_record, then -2 / -4: neither committed nor sent raw
    if rc.undef:
        stats[2] += 1
        return raw, False
    head = b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + (mm.canon(meta) if meta is not None else b"\x80")
    if pg.op == NEST:
        key = mm.pack_str_hdr(len(pg.key)) + pg.key
        return head + map32(len(stay) + 1) + b"".join(stay) + key + map32(nmatch) + b"".join(moved), True
    return head + map32(len(stay) + nmoved) + b"".join(stay) + b"".join(moved), True


class Model:
    """cb_nest_filter over a chunk: filter(data) -> (MODIFIED|NOTOUCH, bytes|None), counts() as flbgpu_filter_last_counts, counters() as
    flbgpu_nest_counters (since the model was created)"""
    MODIFIED, NOTOUCH = 1, 2

    def __init__(self, props):
        self.pg = parse(props)
        self.stats = [0, 0, 0, 0]             # built again, overread compares, undefined, rows over 4 GB
        self.n_in = self.n_out = 0
        self.rows = []

    def filter(self, data):
        p, out, n_in = 0, [], 0
        stats = [0, 0, 0, 0]
        self.rows = []                        # per decoded record: "raw" / "built" / "lost"
        while p < len(data):
            try:
                end, skip, *_ = mm.decode_event(data, p)
            except mm.Bad:
                break                         # the loop ends; what was encoded in front stays (:671-696)
            raw = bytes(data[p:end])
            p = end
            if skip:
                continue
            n_in += 1
            o, built = record(self.pg, raw, stats)
            stats[0] += built
            self.rows.append("built" if built else "raw" if o else "lost")
            if o:
                out.append(o)
        for i in range(4):
            self.stats[i] += stats[i]
        self.n_in = n_in
        if out:                               # MODIFIED exactly when a byte came out (:698-711)
            self.n_out = len(out)
            return self.MODIFIED, b"".join(out)
        self.n_out = n_in
        return self.NOTOUCH, None

    def counts(self):
        return self.n_in, self.n_out

    def counters(self):
        return tuple(self.stats)

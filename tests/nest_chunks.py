"""The chunks of tests/test_nest_gpu.py, kept apart from it so that they can be built and looked at without a device: records whose
rows alternate between raw and built, the seeded structural fuzz of both operations (its generator produces no compare past a
record's end and no record the reference leaves undefined), wide maps."""
import struct

import nest_model as nm
import synth

N1 = [("Operation", "nest"), ("Wildcard", "host"), ("Wildcard", "k8s_*"), ("Nest_under", "kubernetes")]
L1 = [("Operation", "lift"), ("Nested_under", "kubernetes"), ("Add_prefix", "k8s_")]


def rec(body, sec=1, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def mixed_records(n):
    """matching and non-matching rows in turn: raw and rebuilt rows alternate inside a wave"""
    out = []
    for i in range(n):
        if i % 3 == 0:
            body = {"log": "line %d" % i, "stream": "stdout"}
        elif i % 3 == 1:
            body = synth.KV([(b"host", b"h%d" % i), (b"log", b"x" * (i % 37)), (b"k8s_pod", b"p"), (b"kubernetes", {b"ns": b"d", b"pod": i})])
        else:
            body = synth.KV([(b"kubernetes", {b"a": 1}), (b"n", i), (b"kubernetes", synth.Raw(b"\xde\x00\x01\xd9\x01b\xd0\x05"))])
        out.append(rec(body, 1700000000 + i, i))
    return b"".join(out)


# ---- seeded structural fuzz: no compare runs past a record's end and no record is undefined
KEYS = [b"", b"a", b"ab", b"abc", b"abcd", b"abcde", b"abcdefg", b"abcdefgh", b"abcdefghi", b"host", b"hostname", b"k8s_pod", b"k8s_", b"k8",
        b"m", b"mm", b"log", b"x" * 40, b"pre_a", b"pre_", b"pre_pre_b", b"a\0b", "é".encode()]
WILD = ["a", "ab*", "abc", "abcd*", "abcde", "abcdefgh*", "abcdefghi", "host", "k8s_*", "m", "*", "x" * 40, "x" * 8 + "*", "pre_*", "zz", "é"]
PREFIXES = ["", "p", "pre_", "abcd", "k8s_", "x" * 9]


def hdr(b, forms, r):
    h, n = r.choice(forms)
    return h + len(b).to_bytes(n, "big") + b


def rnd_key(r, scalar_ok=True, avoid=None):
    c = r.random()
    k = r.choice([x for x in KEYS if x != avoid])
    if c < 0.55:
        return k
    if c < 0.7:
        return synth.Raw(hdr(k, [(b"\xd9", 1), (b"\xda", 2), (b"\xdb", 4)], r))
    if c < 0.88 or not scalar_ok:
        return synth.Raw(hdr(k, [(b"\xc4", 1), (b"\xc5", 2), (b"\xc6", 4)], r))
    return r.choice([0, 7, 300, -1, True, None, 1.5, [1, b"a"]])


def rnd_val(r, depth=0):
    c = r.randrange(11 if depth < 2 else 8)
    if c == 0:
        return r.choice([b"", b"sample", "café".encode(), b"x" * r.randrange(70), b"y" * 300])
    if c == 1:
        return synth.Raw(b"\xc4\x03abc")
    if c == 2:
        return r.choice([0, 1, 127, 128, 255, 256, 65535, 65536, 2 ** 32, 2 ** 63, -1, -32, -33, -129, -32769, -2 ** 31 - 1])
    if c == 3:
        return synth.Raw(r.choice([b"\xd0\x05", b"\xd1\x01\x00", b"\xd2\x00\x01\x00\x00", b"\xd3" + bytes(7) + b"\x09", b"\xcd\x00\x07",
                                   b"\xce\x00\x00\x01\x00", b"\xcf" + bytes(7) + b"\x01", b"\xd1\xff\xff"]))
    if c == 4:
        return r.choice([1.5, True, False, None, synth.Raw(b"\xca" + struct.pack(">f", 1.5))])
    if c == 5:
        return synth.Raw(r.choice([b"\xda\x00\x03abc", b"\xdb\x00\x00\x00\x01z", b"\xc5\x00\x02hi", b"\xc7\x03\x05abc", b"\xd5\x01ab"]))
    if c == 6:
        return synth.Raw(r.choice([b"\xdc\x00\x02\x01\x02", b"\xdd\x00\x00\x00\x01\xa1q", b"\xde\x00\x01\xa1q\x01", b"\xdf\x00\x00\x00\x00"]))
    if c == 7:
        return [rnd_val(r, depth + 1) for _ in range(r.randrange(4))]
    return rnd_map(r, depth + 1, True)


def rnd_map(r, depth, scalar_ok):
    items = [(rnd_key(r, scalar_ok), rnd_val(r, depth)) for _ in range(r.choice([0, 1, 2, 3, 6, 17]))]
    b = synth.mp(synth.KV(items))
    if r.random() < 0.2 and len(items) < 16:
        b = b"\xde" + struct.pack(">H", len(items)) + b[1:]                              # map16 where a fixmap would do
    elif r.random() < 0.1:
        b = b"\xdf" + struct.pack(">I", len(items)) + (b[1:] if len(items) < 16 else b[3:])
    return synth.Raw(b)


def rnd_record(r, op, key, prefixed):
    items = []
    for _ in range(r.choice([0, 1, 2, 3, 5, 8, 16, 17])):
        if op == nm.LIFT and r.random() < 0.25:
            # an entry under the key: a map (inner keys STR / BIN only when a prefix is configured), sometimes not a map
            k = r.choice([key, synth.Raw(b"\xc4" + bytes([len(key)]) + key), synth.Raw(b"\xda" + struct.pack(">H", len(key)) + key)])
            items.append((k, rnd_map(r, 1, not prefixed) if r.random() < 0.85 else rnd_val(r, 2)))
        else:
            items.append((rnd_key(r, avoid=key if op == nm.LIFT else None), rnd_val(r)))      # (the key's entries are the ones above)
    # every STR / BIN key is followed by a value and a closing entry long enough that no compare leaves the record
    items.append((b"tail", b"t" * 48))
    body = rnd_map_of(items, r)
    kind = r.randrange(8)
    if kind == 0:
        return synth.mp([r.choice([0, 5, 1700000000, 2 ** 32 - 1, 2 ** 32, 2 ** 40]), body])      # legacy; the last two: refused times
    if kind == 1:
        return synth.mp([1700000000.25, body])
    if kind == 2:
        return synth.mp([[synth.ext_ts(5, 6), synth.KV([(b"m", 1), (b"z", [1, synth.Raw(b"\xd0\x05")])])], body])
    if kind == 3 and r.random() < 0.3:
        return synth.mp([[synth.Raw(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), {}], {}])      # group marker
    return synth.mp([[synth.ext_ts(r.randrange(2 ** 32 - 2), r.randrange(10 ** 9)), {}], body])


def rnd_map_of(items, r):
    b = synth.mp(synth.KV(items))
    if r.random() < 0.2 and len(items) < 16:
        b = b"\xde" + struct.pack(">H", len(items)) + b[1:]
    return synth.Raw(b)


def rnd_program(r, op):
    key = r.choice([b"m", b"kubernetes", b"abcd", b"abcde", b""])
    props = [("Operation", "nest" if op == nm.NEST else "lift"), (r.choice(["Nest_under", "Nested_under"]), key.decode())]
    if op == nm.NEST:
        props += [("Wildcard", x) for x in r.sample(WILD, r.randrange(1, 5))]
    c = r.random()
    if c < 0.35:
        props.append(("Add_prefix", r.choice(PREFIXES)))
    elif c < 0.7:
        # a removed prefix is never longer than the 48 bytes that close every record, and a key shorter than it that continues it
        # does not occur: the keys that are proper prefixes of a prefix ("pre_" of nothing, "k8" of "k8s_", "abc" of "abcd") are
        # followed by a type byte >= 0x80, never by the prefix's next letter
        props.append(("Remove_prefix", r.choice(PREFIXES)))
    r.shuffle(props)
    return props, key, c < 0.7


def wide_body(n):
    items = b"".join(synth.mp(b"k%d" % j) + synth.mp(b"v%d" % (j % 7)) for j in range(n))
    return synth.Raw((b"\xde" + struct.pack(">H", n) if n < 65536 else b"\xdf" + struct.pack(">I", n)) + items)

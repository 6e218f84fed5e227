"""The record builders of the filter_expect tests and of tools/gen_expect_golden.py, kept apart so that the chunks can be built and
looked at without a device: hand-built events, one record per msgpack value type, the chunk of n records with chosen failing rows,
and the seeded random rules and records of the fuzz rounds."""
import random
import struct

import synth
from checklist_chunks import GROUP_END, GROUP_START, R, f32, kv, rec, sv  # noqa: F401

RULES = ("key_exists", "key_not_exists", "key_val_is_null", "key_val_is_not_null", "key_val_eq")
BIG_T = R(b"\xcf" + struct.pack(">Q", 2 ** 33))          # a time the EventTime cannot hold

# one value of every msgpack type, in the order the failure lists of the tests read
TYPE_VALUES = [("nil", None), ("true", True), ("false", False), ("pint", 7), ("nint", -7), ("f32", f32(1.5)), ("f64", 2.5), ("str", "val"),
               ("bin", R(b"\xc4\x03val")), ("array", ["val"]), ("map", kv(("val", 1))), ("ext", R(b"\xc7\x03\x05val"))]


def type_records():
    return b"".join(rec(kv(("t", name), ("k", v)), 10 + i) for i, (name, v) in enumerate(TYPE_VALUES))


def map_n(n, first=None):
    """a body of n entries with the smallest header that holds them"""
    items = b"".join(synth.mp("k%d" % i) + synth.mp(i & 0x7f) for i in range(n - (1 if first else 0)))
    if first:
        items = synth.mp(first[0]) + synth.mp(first[1]) + items
    hdr = bytes([0x80 | n]) if n < 16 else (b"\xde" + struct.pack(">H", n) if n < 65536 else b"\xdf" + struct.pack(">I", n))
    return R(hdr + items)


def rows(n, failing=(), key="a"):
    """n records that all carry `key`, except the rows of `failing`, which carry `b` in its place"""
    failing = set(failing)
    out = []
    for i in range(n):
        k = "b" if i in failing else key
        s = i % 3
        if s == 0:
            body = kv((k, "v%d" % (i % 11)), ("n", i))
        elif s == 1:
            body = kv(("pad", "x" * (i % 37)), (k, None), ("f", 1.5))
        else:
            body = kv((7, "int key"), (k, kv(("s", [1, "two"]))), ("u", R(b"\xcd\x00\x05")))
        out.append(rec(body, 1700000000 + i, i % 1000, kv(("m", i)) if i % 5 == 0 else None))
    return b"".join(out)


# rules that pass on the record fuzz_round() builds before it damages it
FUZZ_RULES = [("key_exists", "$a"), ("key_exists", "log"), ("key_exists", "$m['a']['b']"), ("key_exists", "$m['l'][1]"), ("key_not_exists", "$zz"),
              ("key_not_exists", "$TAG"), ("key_not_exists", "$m['zz']"), ("key_not_exists", "$m['l'][3]"), ("key_val_is_null", "$nul"),
              ("key_val_is_not_null", "$a"), ("key_val_is_not_null", "$m['a']"), ("key_val_eq", "$a v"), ("key_val_eq", "$m['a']['b'] val"),
              ("key_val_eq", "log a b  c"), ("key_val_eq", "$m['l'][0] anything"), ("key_val_eq", "b$x bee")]


def fuzz_round(seed):
    """(props, chunk): random rules, every one of which a whole record passes, over at most 2000 records of which a share -- none,
    few, a fifth or all, by the seed -- is damaged in one place: a key gone, a value of another type, another text, a duplicate key"""
    rnd = random.Random(seed)
    action = ("warn", "exit", "result_key")[seed % 3]
    props = [rnd.choice(FUZZ_RULES) for _ in range(rnd.choice([0, 1, 2, 3, 5, 8, 13]))]
    props.insert(rnd.randint(0, len(props)), ("action", action))
    if rnd.random() < 0.5:
        props.insert(rnd.randint(0, len(props)), ("result_key", rnd.choice(["matched", "a", "r" * 40])))
    share = (0.0, 0.02, 0.2, 1.0)[(seed // 3) % 4]
    odd = [None, True, 5, -5, 2.5, f32(0.5), R(b"\xc4\x01v"), R(b"\xd4\x01v"), ["v"], kv(("b", "val")), sv(b""), sv(b"v\0"), sv(b"va"), sv(b"val"), sv(b"a b  c ")]
    recs = []
    n = rnd.choice([1, 63, 64, 65, 300, 1000, 2000])
    for i in range(n):
        items = {"a": "v", "b": "bee", "log": "a b  c", "nul": None, "m": None}
        inner = {"a": kv(("b", "val")), "l": ["anything", sv(b"x"), 2]}
        extra = []
        if rnd.random() < share:
            what = rnd.randrange(6)
            k = rnd.choice(["a", "b", "log", "nul"])
            if what == 0:
                del items[k]
            elif what == 1:
                items[k] = rnd.choice(odd)
            elif what == 2:
                extra.append((k, rnd.choice(odd)))                       # a duplicate key: the last one wins
            elif what == 3:
                inner[rnd.choice(["a", "l"])] = rnd.choice(odd)
            elif what == 4:
                extra.append((rnd.choice(["zz", "b$x"]), rnd.choice(odd)))
            else:
                inner["zz"] = rnd.choice(odd)
        pairs = [(k, kv(*inner.items()) if k == "m" else v) for k, v in items.items()] + extra
        if rnd.random() < 0.1:
            pairs.append((R(b"\xc4\x01a"), 1))                            # a key that is no STR
        if not extra:
            rnd.shuffle(pairs)
        if rnd.random() < 0.02:
            recs.append(GROUP_START if rnd.random() < 0.5 else GROUP_END)
        recs.append(rec(kv(*pairs), 1700000000 + i, i, kv(("m", i)) if rnd.random() < 0.1 else None))
    return props, b"".join(recs)

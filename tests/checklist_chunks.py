"""The record builders of the filter_checklist tests and of tools/gen_checklist_golden.py, kept apart so that the chunks can be built
and looked at without a device: hand-built events, the recorded cases' inputs, the chunk of n records of which every third matches,
and the seeded random lists, records and accessor paths of the fuzz rounds."""
import random
import struct

import synth

R = synth.Raw
GROUP_START = synth.mp([[R(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), synth.KV([("g", 1)])], synth.KV([("r", 1)])])
GROUP_END = synth.mp([[R(b"\xd7\x00\xff\xff\xff\xfe\x00\x00\x00\x00"), {}], {}])
LIST, MISSING = "@LIST@", "@MISSING@"          # stand for the list file's path and for a path that does not exist


def rec(body, sec=1, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def kv(*items):
    return synth.KV(list(items))


def sv(b):
    """a STR of any bytes"""
    b = bytes(b)
    n = len(b)
    if n < 32:
        h = bytes([0xa0 | n])
    elif n < 256:
        h = bytes([0xd9, n])
    elif n < 65536:
        h = b"\xda" + struct.pack(">H", n)
    else:
        h = b"\xdb" + struct.pack(">I", n)
    return R(h + b)


def f32(v):
    return R(b"\xca" + struct.pack(">f", v))


# the LIKE edge list of the issue: (value, entry, answer)
LIKE_EDGES = [
    (b"a\xc3\xa9\xa9\xa9b", b"a_b", True),
    (b"a\xa9b", b"a_b", True),
    (b"a\xc0\x80b", b"a\xc1\x81b", True),
    (b"ab\0cd", b"ab", True),
    (b"ab\0cd", b"ab%d", False),
    (b"", b"%", True),
    # and what the walker's own paths add
    (b"xx\xe2\x80\xa2y", b"%\xe2\x80", True),                 # U+0080 behind '%' is searched as a raw byte
    (b"abcabd", b"%ab_%d", True),
    (b"abcabc", b"a%c%d", False),
    (b"", b"_", False),
    (b"a", b"a__", False),
    (b"mississippi", b"m%iss%ip_i", True),
    (b"\xef\xbf\xbe", b"\xed\xa0\x80", True),                 # U+FFFE and a surrogate both read as U+FFFD
    (b"a%b", b"a%b", True),
    (b"ab", b"abc", False),
    (b"Ab", b"ab", False),
]


def third_records(n, hit=b"hit-%d", miss=b"miss-%d"):
    """n records of several shapes; every third one carries a value of the list third_list() builds"""
    out = []
    for i in range(n):
        val = (hit if i % 3 == 0 else miss) % (i % 7)
        s = i % 4
        if s == 0:
            body = kv(("log", sv(val)), ("n", i))
        elif s == 1:
            body = kv(("a", "x" * (i % 41)), ("log", sv(val)), ("flag", "old"))
        elif s == 2:
            body = kv(("log", 5), ("m", kv(("k", [1, 2.5, None]))), ("log", sv(val)))
        else:
            body = kv((R(b"\xc4\x01b"), 1), ("log", sv(val)), (7, "int key"), ("s8", R(b"\xd9\x02ab")))
        out.append(rec(body, 1700000000 + i, i % 1000, kv(("m", i)) if i % 5 == 0 else None))
    return b"".join(out)


def third_list(partial):
    if partial:
        return b"hit-0\nhit-_%\n# comment\n%never\n"
    return b"".join(b"hit-%d\n" % i for i in range(7))


def fuzz_round(seed, partial):
    """(props without file, list bytes, chunk): random list, records and accessor path; half the values are drawn from the list"""
    rnd = random.Random(seed)
    alpha = b"abAB%_-\xc3\xa9\x80 " if partial else b"abcABC-_ \xc3\xa9"
    def word(lo=1, hi=9):
        return bytes(rnd.choice(alpha) for _ in range(rnd.randint(lo, hi)))
    entries = []
    for _ in range(rnd.randint(1, 40)):
        w = word()
        if not any(c in b"abAB-" for c in w):                 # every entry asks for a literal the unmatched values do not have
            w += b"a"
        entries.append(w)
    lines = b"".join(e + (b"\r\n" if rnd.random() < 0.2 else b"\n") for e in entries)
    fold = rnd.random() < 0.5
    path = ["log", "$log", "$m['a']", "$m['l'][1]", "$m['a']['b']"][seed % 5]
    props = [("lookup_key", path), ("mode", "partial" if partial else "exact"), ("ignore_case", "on" if fold else "off"),
             ("record", "hit true"), ("record", "log replaced") if rnd.random() < 0.5 else ("record", "why listed")]
    recs = []
    for i in range(rnd.randint(100, 400)):
        if rnd.random() < 0.5:
            v = rnd.choice(entries)
            if partial:
                v = v.replace(b"%", b"").replace(b"_", b"q") + word(0, 3)
            if fold and rnd.random() < 0.5:
                v = v.upper()
        else:
            v = bytes(rnd.choice(b"zZyY") for _ in range(rnd.randint(1, 9)))
        val = sv(v) if rnd.random() < 0.9 else rnd.choice([5, None, [sv(v)], R(b"\xc4\x01a")])
        if path in ("log", "$log"):
            body = kv(("k", i), ("log", val))
        elif path == "$m['a']":
            body = kv(("m", kv(("a", val), ("z", 1))))
        elif path == "$m['l'][1]":
            body = kv(("m", kv(("l", [0, val, 2]))), ("log", "x"))
        else:
            body = kv(("m", kv(("a", kv(("b", val))))))
        recs.append(rec(body, 1700000000 + i, i))
    return props, lines, b"".join(recs)

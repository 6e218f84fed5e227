"""The chunks of tests/test_typeconv_gpu.py, kept apart from it so that they can be built and looked at without a device: records
that hold one key of every source class, the seeded fuzz (random programs, and records that place next to each rule's key values of
every msgpack type; its float sources stay inside the ranges in which C defines float -> int / uint), value strings of given lengths."""
import struct

import synth

# one rule of each source class
P4 = [("str_key", "status status_i int"), ("int_key", "size size_s string"), ("uint_key", "id id_f float"), ("float_key", "lat lat_s string")]
# 64 rules: the table spans many LDS words (names of every length from 1 to 16, four kinds of accessor)
P64 = ([("str_key", "status t%d %s" % (i, ["int", "uint", "hex", "float", "bool", "string"][i % 6])) for i in range(12)] +
       [("int_key", "%s n%d %s" % ("size" if i % 2 else "$m['n']", i, ["string", "float", "uint", "int"][i % 4])) for i in range(16)] +
       [("uint_key", "%s u%d %s" % ("id" if i % 3 else "$m['l'][1]", i, ["string", "float", "int", "hex"][i % 4])) for i in range(16)] +
       [("float_key", "%s f%s %s" % ("lat" if i % 2 else "k" * (i // 2 + 1), "x" * i, ["string", "int", "uint", "float"][i % 4])) for i in range(20)])


def rec(body, sec=1, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def mixed_records(n):
    """three shapes in turn, so that the lanes of a wave take different paths: every key present; some keys, a failing conversion and
    a non-canonical entry; none of the keys"""
    out = []
    for i in range(n):
        if i % 3 == 0:
            body = synth.KV([(b"status", b"%d" % (200 + i % 300)), (b"size", i * 37 - 500), (b"id", 2 ** 40 + i), (b"lat", i / 8.0),
                             (b"m", {b"n": -i, b"l": [0, i, 2]}), (b"log", b"x" * (i % 41))])
        elif i % 3 == 1:
            body = synth.KV([(b"status", b"abc"), (b"size", synth.Raw(b"\xd3" + struct.pack(">q", i))), (b"lat", b"text"), (b"kk", 0.5 + i),
                             (b"status", b" %d tail" % i)])
        else:
            body = {"log": "line %d" % i, "stream": "stdout"}
        out.append(rec(body, 1700000000 + i, i))
    return b"".join(out)


# ---- seeded fuzz
KEYS = [b"a", b"ab", b"abc", b"abcd", b"abcde", b"abcdefgh", b"abcdefghi", b"status", b"k" * 40]
TO_KEYS = ["t", "out", "a", "abcd", "x" * 33, "é"]
WORDS = {0: ["int", "i", "uint", "u", "hex", "h", "float", "f", "bool", "b", "string"],
         1: ["string", "s", "str", "float", "uint", "u", "int", "hex"],
         2: ["string", "s", "float", "f", "int", "i", "uint", "bool"],
         3: ["string", "st", "int", "in", "uint", "ui", "float", "hex"]}
PROPS = ["str_key", "int_key", "uint_key", "float_key"]
STRINGS = [b"", b"0", b"12", b"-12", b"+7", b"  42", b"\t-9x", b"abc", b"0x1f", b"0X", b"ff", b"1.5", b"-2.5e3", b"1e400", b"nan", b"nan(0x7)", b"inf", b"-0",
           b"true", b"FALSE", b"TRUEish", b"fals", b"18446744073709551616", b"9223372036854775808", b"-9223372036854775809", b"1\x002", b"7" * 25,
           b"0x" + b"f" * 17, b" \r\n12.75rest", b"0.1", b"123456789.123456789e-5"]
INTS = [0, 1, -1, 127, 128, 255, 256, -32, -33, -128, -129, 65535, 65536, 2 ** 31, 2 ** 32, 2 ** 53 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, -2 ** 31 - 1, -2 ** 63,
          synth.Raw(b"\xd0\x05"), synth.Raw(b"\xd1\x00\x07"), synth.Raw(b"\xd3" + bytes(7) + b"\x09"), synth.Raw(b"\xcf" + bytes(7) + b"\x01")]
# float sources: inside (-1, 2^63), where C defines both float -> int and float -> uint
FLOATS = [0.0, -0.0, 0.5, -0.5, 1.0, 1.5, 123.456, 1e15, 1e16, 2.0 ** 53 + 2, 2.0 ** 62, 2.0 ** 63 - 1024, 1e-7, 5e-324, 0.1,
          synth.Raw(b"\xca" + struct.pack(">f", 1.5)), synth.Raw(b"\xca" + struct.pack(">f", 0.1)), synth.Raw(b"\xca" + struct.pack(">f", 16777216.0))]
OTHERS = [None, True, False, synth.Raw(b"\xc4\x0212"), synth.Raw(b"\xd5\x01ab"), [1, b"2"], {b"a": b"1"}, synth.Raw(b"\xda\x00\x0212"),
          synth.Raw(b"\xdb\x00\x00\x00\x03-45"), synth.Raw(b"\xdc\x00\x01\x05")]


def rnd_value(r, src):
    """a value for a key a rule of source class src reads: mostly of the class, often not"""
    c = r.random()
    if c < 0.6:
        return r.choice([STRINGS, INTS, INTS, FLOATS][src])
    if c < 0.9:
        return r.choice(r.choice([STRINGS, INTS, FLOATS]))
    return r.choice(OTHERS)


# the fourteen pairs a conversion exists for: program i's first rule is pair i, so a seed's programs go through all of them
PAIR_WORDS = [(0, "int"), (0, "uint"), (0, "hex"), (0, "float"), (0, "bool"), (1, "string"), (1, "float"), (1, "uint"),
              (2, "string"), (2, "float"), (2, "int"), (3, "string"), (3, "int"), (3, "uint")]


def rnd_program(r, i):
    """(props, [(key, source class, accessor form)])"""
    props, keys = [], []
    for j in range(r.choice([1, 1, 2, 3, 5, 8])):
        src = r.randrange(4)
        word = r.choice(WORDS[src])
        if j == 0:
            src, word = PAIR_WORDS[i % len(PAIR_WORDS)]
        key = r.choice(KEYS)
        form = r.randrange(5)
        name = key.decode()
        acc = [name, "$" + name, "$m['%s']" % name, "$m['l'][1]", "$" + name + "['sub']"][form]
        props.append((PROPS[src], "%s %s %s" % (acc, r.choice(TO_KEYS), word)))
        keys.append((key, src, form))
    r.shuffle(props)
    return props, keys


def rnd_record(r, keys):
    items = []
    for key, src, form in keys:
        if r.random() < 0.2:
            continue
        if form in (0, 1):
            items.append((key, rnd_value(r, src)))
        elif form == 2:
            items.append((b"m", synth.KV([(b"z", 1), (key, rnd_value(r, src)), (key, rnd_value(r, src))])))
        elif form == 3:
            items.append((b"m", {b"l": [rnd_value(r, src) for _ in range(r.randrange(4))]}))
        else:
            items.append((key, r.choice([rnd_value(r, src), {b"sub": rnd_value(r, src)}, {b"other": 1}])))
    for _ in range(r.choice([0, 1, 3, 17])):
        items.append((r.choice(KEYS + [b"other", 5, None]), rnd_value(r, r.randrange(4))))
    r.shuffle(items)
    b = synth.mp(synth.KV(items))
    if r.random() < 0.2 and len(items) < 16:
        b = b"\xde" + struct.pack(">H", len(items)) + b[1:]                              # map16 where a fixmap would do
    body = synth.Raw(b)
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


def number_then_garbage(number, n):
    """n bytes: the number's text, cut to fit, then bytes no number continues with"""
    return (number + b"z" * n)[:n]

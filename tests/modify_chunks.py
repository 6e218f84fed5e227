"""The chunks of tests/test_modify_gpu.py, kept apart from it so that they can be built and looked at without a device: the seeded
fuzz of programs and records (its generator produces no prefix compare past a record's end: tests/test_modify_ref.py holds it to that
on the model), rows that alternate between rebuilt and raw inside a wave, bodies around the LDS list's size, rows of 64 entries for
the arena."""
import struct

import modify_model as mm
from nest_chunks import hdr, rnd_val
import synth

# the names of the first generator, longer ones over the same letters, a key with a NUL, a 40-byte key
KEYS = [b"a", b"ab", b"abc", b"abcd", b"k", b"k1", b"k2", b"log", b"re", b"ref", b"referer", b"x", b"", b"true", b"A3", b"a\0b", b"x" * 40]
NAMES = [k.decode() for k in KEYS if k and b"\0" not in k]
# prefix rules: none is longer than the 48 bytes that close every record.  A key that is a proper prefix of one of them ("a" of "ab",
# "re" of "ref", "x" of "xxxxxxxx", "" of all) is followed by its value: the compare then runs into the value and the entries behind
# it, at most 48 bytes, and every record ends in ("tail", 48 bytes) -- and so does every re-pack, unless a rule moved or removed the
# tail: the programs below never name it.
PREFIXES = NAMES + ["r", "refe", "abx", "x" * 8, "k"]
TAIL = (b"tail", b"t" * 48)
FUZZ_SEEDS = [1234, 20271, 20272, 20273]


def rec(body, sec=1, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def rnd_key(r):
    c = r.random()
    k = r.choice(KEYS)
    if c < 0.55:
        return k
    if c < 0.72:
        return synth.Raw(hdr(k, [(b"\xd9", 1), (b"\xda", 2), (b"\xdb", 4)], r))
    if c < 0.88:
        return synth.Raw(hdr(k, [(b"\xc4", 1), (b"\xc5", 2), (b"\xc6", 4)], r))
    return r.choice([0, 7, 300, -1, True, False, None, 1.5, [1, b"a"]])


def rnd_value(r):
    c = r.random()
    if c < 0.4:
        return r.choice([b"sample", b"sample", b"abc", b"abc", b"500", b"true", b"", b"s0"])    # what the drawn conditions look for
    if c < 0.46:
        return r.choice([True, False, synth.Raw(b"\xc4\x06sample"), synth.Raw(b"\xc4\x03abc")])
    if c < 0.52:
        return {b"ab": r.choice([1, b"sample", [1]]), b"k": [r.choice([1, b"abc"])]}
    return rnd_val(r)


def rnd_body(r):
    items = [(rnd_key(r), rnd_value(r)) for _ in range(r.choice([0, 1, 2, 3, 4, 5, 6, 7, 9, 14]))]
    if r.random() < 0.6:
        # the entry most of the drawn conditions ask for
        items.insert(r.randrange(len(items) + 1), (b"k", b"sample" if r.random() < 0.7 else r.choice([b"abc", b"s0", b"500"])))
    items.append(TAIL)
    b = synth.mp(synth.KV(items))
    c = r.random()
    if c < 0.15 and len(items) < 16:
        b = b"\xde" + struct.pack(">H", len(items)) + b[1:]                               # map16 where a fixmap would do
    elif c < 0.25 and len(items) < 16:
        b = b"\xdf" + struct.pack(">I", len(items)) + b[1:]
    return synth.Raw(b)


def rnd_record(r):
    body = rnd_body(r)
    kind = r.randrange(10)
    if kind == 0:
        return synth.mp([r.choice([0, 5, 1700000000, 2 ** 32 - 1, 2 ** 32, 2 ** 40, r.randrange(2 ** 33)]), body])   # legacy, integer time
    if kind == 1:
        return synth.mp([1700000000.25, body])                                            # legacy, float time
    if kind == 2:
        return synth.mp([[synth.ext_ts(5, 6), {"m": 1, "z": [1, 2]}], body])               # metadata
    if kind == 3 and r.random() < 0.3:
        return synth.mp([[synth.Raw(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), {}], {}])   # group marker
    if kind == 4:
        # metadata that is not canonical: map16, a str8 key, a positive value in the signed family
        return synth.mp([[synth.ext_ts(7, 8), synth.Raw(b"\xde\x00\x02\xd9\x01m\xd0\x05\xa1z\x92\x01\xd1\x00\x02")], body])
    return synth.mp([[synth.ext_ts(r.randrange(2 ** 32), r.randrange(10 ** 9)), {}], body])


def rnd_word(r):
    return r.choice(NAMES + ["^a", "b$", "^k[0-9]$", "/^A/i", "x|y", "^true$", "^false$"])


def rnd_program(r):
    props = []
    for _ in range(r.choice([0, 0, 1, 1, 1, 2])):
        t = r.choice(mm.CONDS)
        ty = mm.CONDS.index(t)
        if mm.a_rx(ty):
            props.append(("Condition", "%s %s %s" % (t, r.choice(["^a", "^k", "^re", "true", ".", "^zz"]), r.choice(["^s", "0", "t", "."]))))
        else:
            props.append(("Condition", "%s %s %s" % (t, r.choice(["k", "k", "k", "k", "a", "$a", "k1", "$a['k'][0]", "$a['ab']", "$TAG", "log", "tail"]),
                                                    r.choice(["^s", "abc", "^t", "0"] if mm.b_rx(ty) else ["sample", "sample", "sample", "abc", "''", "true"]))))
    for _ in range(r.randrange(1, 9)):
        name = r.choice(list(mm.RULES1) + list(mm.RULES2))
        if name in mm.RULES1:
            props.append((name, rnd_word(r) if name == "remove_regex" else r.choice(PREFIXES if name != "remove" else NAMES)))
        else:
            a, b = r.choice(NAMES), r.choice(NAMES + ["new", "other"])
            if name == "hard_copy" and a == b:
                b = b + "_2"
            props.append((name, "%s %s" % (a, b)))
    r.shuffle(props)
    return props


def noncanonical_key_headers(data):
    """the body keys of a chunk whose header is not the one msgpack_pack_object writes"""
    n, p = 0, 0
    while p < len(data):
        end, skip, _, _, _, body = mm.decode_event(data, p)
        p = end
        for k, _ in body.v:
            n += data[k.start:k.end] != mm.canon(k)
    return n


# ---- rows that alternate inside a wave: rebuilt, raw because the condition is false, raw because the encoder refuses the time
W_COND = [("Condition", "Key_exists go"), ("Set", "k x"), ("Move_to_start", "n"), ("Copy", "n m")]
W_PLAIN = [("Remove", "go"), ("Rename", "n0 first"), ("Move_to_end", "k")]


def wave_rows(n):
    out = []
    for i in range(n):
        items = [(b"n%d" % j, j) for j in range(i % 7)] + [(b"k", b"v%d" % i)]
        if i % 3 != 1:
            items.insert(i % (len(items) + 1), (b"go", 1))
        items.append(TAIL)
        if i % 3 == 2:
            out.append(synth.mp([2 ** 32 + i, synth.KV(items)]))
        else:
            out.append(rec(synth.KV(items), 1700000000 + i, i))
    return b"".join(out)


# ---- bodies around the LDS list's size
def list_rows(n, sizes):
    """rows of sizes[i % len] entries e0..: "src" first where there is room for it, an empty map every seventh row"""
    out = []
    for i in range(n):
        m = sizes[i % len(sizes)]
        if i % 7 == 6:
            out.append(rec({}, 2, i))
            continue
        items = [(b"src", b"s%d" % i)] + [(b"e%d" % j, j) for j in range(m - 1)]
        out.append(rec(synth.KV(items), 2, i))
    return b"".join(out)


def rows_of_64(n, bad_at=None):
    body = synth.mp(synth.KV([(b"k%d" % j, j) for j in range(64)]))
    out = [synth.mp([[synth.ext_ts(4, i), {}], synth.Raw(body)]) for i in range(n)]
    if bad_at is not None:
        out[bad_at] = synth.mp([[synth.ext_ts(4, bad_at), {}], "not a map"])
    return b"".join(out)

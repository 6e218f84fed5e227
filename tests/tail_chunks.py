"""The named texts of the in_tail tests, kept apart so that they can be built and looked at without a device.  Every text is
deterministic and built from lengths; each group aims at one family of edges of csrc/tail_kernels.inc, and tests/test_tail_lines.py
asserts (with tail_model.emit_paths or plain arithmetic) that each still reaches the edge it was written for.

group(name) -> [(label, text, [config, ...])]; a config is the keyword set of tail_model.records / oracle_binding.tail_process."""
import functools

D = dict()
NOSKIP = dict(skip_empty_lines=False)
OFFS = dict(offset_key="offset", stream_offset=123456789012)
PATHS = dict(key="message", path_key="file", path="/var/log/app/a.log")
GROUPS = ("staging", "many_lines", "edges", "neighbours", "nuls", "encodings")
MANY_LINES_OFFSET = dict(offset_key="offset", stream_offset=2 ** 32 - 1_000_000)       # 5-byte / 9-byte offsets meet at byte 1 000 000
CRLF_RULE = ("regex", "log ^ab$")                                                      # keeps the CR LF lines of the many-lines text


def default_size(ll):
    """bytes of the default config's record of a line of ll bytes (after the CR rule): 22 + a4 "log" + str header + line"""
    return 26 + (1 if ll < 32 else 2 if ll < 256 else 3 if ll < 65536 else 5) + ll


class _Lines:
    """lines appended by length, tracking where the default config's record of the next line starts"""

    def __init__(self):
        self.parts, self.o, self.rows = [], 0, 0

    def line(self, ll, fill=b"s"):
        self.parts.append(fill * ll + b"\n")
        self.o += default_size(ll)
        self.rows += 1

    def skipped(self):
        self.parts.append(b"\r\n" if self.rows & 1 else b"\n")
        self.rows += 1

    def align_to(self, a):
        """one short record after which the next one starts at a & 15"""
        self.line(1 + ((a - self.o - 28) & 15), b"p")
        assert self.o & 15 == a

    def small_until(self, lane):
        while self.rows & 63 != lane:
            self.line(3 + (self.rows & 7), b"f")

    def text(self):
        return b"".join(self.parts)


def staging_text():
    """k_tl_emit's staging area (TL_STG = 18944 bytes per wave), default config: a record of 26 + hdr + ll bytes.
    tile 0: a batch that fits exactly at align 0 (line of 18915 bytes) with a skipped row inside it, one that fits exactly at
    align 1 (record of 18943 bytes), a record one byte over at align 0 (line of 18916 bytes: direct path), then 16 times a short
    record growing by one byte from align 0 and a record of 18916 bytes that it pushes out of its batch, so that batches start at
    every align; lane 63 direct.  tile 1: direct at lanes 0 and 31, the rest short rows and skipped ones.  tile 2 (partial): a direct record."""
    b = _Lines()
    b.line(18915)                       # lane 0: record of 18944 bytes at offset 0
    b.skipped()                         # lane 1: inside that batch, adds nothing
    b.align_to(1)                       # lane 2
    b.line(18914)                       # lane 3: record of 18943 bytes at align 1
    b.skipped()
    b.align_to(0)                       # lane 5
    b.line(18916)                       # lane 6: record of 18945 bytes at align 0: one byte over
    for k in range(16):                 # lanes 7 .. 54
        b.align_to(0)
        b.line(2 + k, b"a")             # a record of 29 + k bytes from align 0 ...
        b.line(18887, b"b")             # ... pushes this one (18916 bytes: fits alone at any align) to a batch at align (29 + k) & 15
    b.small_until(63)
    b.line(40000, b"c")                 # (0, 63)
    b.line(18916 + 15, b"d")            # (1, 0)
    b.small_until(20)
    for _ in range(6):
        b.skipped()
    b.small_until(31)
    b.line(66000, b"e")                 # (1, 31): a 5-byte str header on the direct path
    b.small_until(0)
    for k in range(5):
        b.line(100 + k, b"g")
    b.line(19000, b"h")                 # (2, 5): the last tile is partial
    b.line(7, b"i")
    return b.text()


MANY_UNIT = b"a\n" b"ab\r\n" b"\n" b"\r\n" b"a\n" b"b\n"           # 6 lines in 13 bytes: no phase repeats within a 64-byte mask word


def many_lines_text(lines=1_100_004):
    return MANY_UNIT * (lines // 6)


def _fill(n, final_newline):
    body = (b"line of seven\n" * (n // 14 + 1))[:n - 1]
    return body + (b"\n" if final_newline else b"x")


def edge_texts():
    out = []
    for p in (62, 63, 64, 65, 16382, 16383, 16384, 16385, 32767, 32768):
        out.append(("newline at byte %d" % p, b"x" * p + b"\nyz\n"))
    for n in (63, 64, 65, 16383, 16384, 16385):
        out.append(("%d bytes, final newline" % n, _fill(n, True)))
        out.append(("%d bytes, no final newline" % n, _fill(n, False)))
    out.append(("64 newlines in one mask word", b"a" * 64 + b"\n" * 64 + b"b\n"))
    out.append(("64 newlines across two mask words", b"a" * 31 + b"\n" * 65 + b"b\n"))
    out.append(("a tile without a newline", b"l\n" * 8192 + b"z" * 16384 + b"\n" + b"m\n" * 100))
    out.append(("CR LF across a 64-byte edge", b"x" * 63 + b"\r\nnext\n"))
    out.append(("CR LF across a 16 KB edge", b"x" * 16383 + b"\r\nnext\n"))
    out.append(("a lone CR across a 64-byte edge", b"x" * 62 + b"\n\r\nnext\n"))
    out.append(("a lone CR across a 16 KB edge", b"x" * 16382 + b"\n\r\nnext\n"))
    return [(n, t, [D, NOSKIP]) for n, t in out]


def neighbours_text():
    """for every byte value v: `v \\n v` four times (3-byte period: the newline in each byte lane of a dword) and `\\n v v v v` four
    times (5-byte period, likewise), 32 bytes per value; the whole laid twice, 32 bytes apart, so that each value meets both halves
    of a thread's 64 bytes"""
    body = b"".join(bytes([v, 10, v]) * 4 + bytes([10, v, v, v, v]) * 4 for v in range(256))
    return b"byte neighbours".ljust(31, b".") + b"\n" + body + b"second lay".ljust(31, b".") + b"\n" + body


def noise_text(n=65536, seed=0x2545F491):
    """all 256 byte values from a fixed linear congruential generator, NULs inside but not leading"""
    out, x = bytearray(), seed
    for _ in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        out.append(x >> 56)
    out[0] = 0x41
    return bytes(out)


def nul_texts():
    out = []
    for z in (0, 1, 63, 64, 65, 127, 128, 16384):
        out.append(("%d NULs, abc" % z, b"\0" * z + b"abc\n"))
        out.append(("%d NULs, newline" % z, b"\0" * z + b"\nabc\n"))
        out.append(("%d NULs, no newline" % z, b"\0" * z + b"abc"))
    for z in (1, 64, 100, 16384):
        out.append(("all NUL, %d bytes" % z, b"\0" * z))
    out.append(("NULs inside", b"\0\0a\0b\n\0\n\0\0c\n"))
    return [(n, t, [D, NOSKIP]) for n, t in out]


LENGTHS = (0, 1, 31, 32, 33, 255, 256, 257, 65535, 65536, 65537)
BOUNDS = (128, 256, 65536, 2 ** 32)
OFFSET_WALK = b"x\n" * 10 + b"\n" * 40 + b"ab\n" * 20        # lines start at 0, 2 .. 18, 20, 21 .. 59, 60, 63 ..
K1 = dict(key="k" * 31, path_key="p" * 32, path="/" * 255, offset_key="o" * 31, stream_offset=5)
K2 = dict(key="k" * 32, path_key="p" * 255, path="/" * 31, offset_key="o" * 32, stream_offset=70000)
K3 = dict(key="k" * 255, path_key="p" * 31, path="/" * 32, offset_key="o" * 255, stream_offset=2 ** 40)
EMPTY_PATH = dict(path_key="pk", path="")


def encoding_texts():
    lengths = b"".join(b"e" * n + b"\n" + b"e" * n + b"\r\n" for n in LENGTHS)
    out = [("str headers", lengths, [D, NOSKIP, OFFS])]
    walk = []
    for bound in BOUNDS:
        # a kept line at bound - 2 and at bound (skipping or not); an empty line at bound - 1 and at bound (not skipping)
        for back, skip in ((8, True), (8, False), (40, False)):
            walk.append(dict(offset_key="o", stream_offset=bound - back, skip_empty_lines=skip))
    out.append(("offsets across 128, 256, 65536, 2^32", OFFSET_WALK, walk))
    out.append(("long keys", b"hello\nworld\r\n\n\r\nlast\n", [K1, K2, K3, EMPTY_PATH, dict(K3, skip_empty_lines=False)]))
    return out


@functools.lru_cache(maxsize=None)
def group(name):
    if name == "staging":
        return [("staging", staging_text(), [D, OFFS, PATHS])]
    if name == "many_lines":
        return [("many lines", many_lines_text(), [D, MANY_LINES_OFFSET])]
    if name == "edges":
        return edge_texts()
    if name == "neighbours":
        return [("byte neighbours", neighbours_text(), [D, NOSKIP]), ("noise", noise_text(), [D, NOSKIP])]
    if name == "nuls":
        return nul_texts()
    if name == "encodings":
        return encoding_texts()
    raise KeyError(name)


def cases(names=GROUPS):
    """every (group, label, text, config) of the named groups"""
    return [(g, label, text, c) for g in names for label, text, cfgs in group(g) for c in cfgs]

"""The corpus of csrc/numconv.hpp: every entry point of the header at the inputs where such arithmetic goes wrong, with references that
are exact and -- where that is possible -- independent of glibc and of the code under test.  tests/test_numconv_cases.py runs it through
the host instantiation (flbgpu_nc_*, csrc/numconv_host.cpp); tests/test_numconv.py and tests/test_numconv_int.py draw their generators and
hand-written lists from here.

scan_double     bits: the accepted prefix as a fractions.Fraction, rounded to binary64 by Python's integer true division (correctly
                rounded, subnormals included), the sign put on by hand; status, consumed and NaN payloads: glibc strtod / sscanf("%lf%n")
fmt_f6          decimal.Decimal(v) (exact) quantised to 10^-6, ROUND_HALF_EVEN, cut at cap
fmt_json_double fmt_chunks.py_float_rule
fmt_ld, fmt_lu  str(int)
scan_intmax     ref_intmax below (a restatement of strtoimax / strtoumax), cross-checked against libc by the CPU half
casts           float(int), int(float) inside the defined ranges; x86-64's answers outside them (CAST_X86_*)"""
import ctypes
import functools
import os
import random
import re
import struct
from decimal import Decimal, ROUND_HALF_EVEN, localcontext
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "fluent-bit_amd", "csrc")

NC_FAIL, NC_OK, NC_NEED_EXACT = 0, 1, 2
MODE_STRTOD, MODE_SSCANF, NAN_PAYLOAD = 0, 1, 0x100             # numconv.hpp
MODES = (MODE_STRTOD, MODE_SSCANF, MODE_STRTOD | NAN_PAYLOAD, MODE_SSCANF | NAN_PAYLOAD)
M64 = (1 << 64) - 1
INF_BITS, NAN_BITS, SIGN = 0x7FF0000000000000, 0x7FF8000000000000, 1 << 63
L2M_LABEL_MAX = int(re.search(r"constexpr int L2M_LABEL_MAX = (\d+)", open(os.path.join(CSRC, "dev.hpp")).read()).group(1))
MAX_SIG_DIGITS = int(re.search(r"constexpr int MAX_SIG_DIGITS = (\d+)", open(os.path.join(CSRC, "numconv.hpp")).read()).group(1))
# the entry points, as the runners and checkers below name them
OP_SCAN_DOUBLE, OP_SCAN_INTMAX, OP_FMT_F6, OP_FMT_JSON, OP_FMT_LD, OP_FMT_LU, OP_I2D, OP_U2D, OP_D2I, OP_D2U = range(10)


def f2b(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def b2f(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


# ------------------------------------------------------------------------------------------ moved here from test_numconv.py
def gen_cases(rng, n):
    out = []
    for _ in range(n):
        t = rng.randrange(8)
        if t == 0: out.append(repr(struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]))
        elif t == 1: out.append("%.*e" % (rng.randrange(0, 30), rng.uniform(-1, 1) * 10.0 ** rng.randrange(-320, 308)))
        elif t == 2: out.append("%d.%de%d" % (rng.randrange(10 ** 9), rng.getrandbits(rng.randrange(1, 120)), rng.randrange(-340, 310)))
        elif t == 3:
            # exact decimal expansion of a midpoint between two doubles (the hard rounding cases)
            b = rng.getrandbits(63) % 0x7FE0000000000000
            lo = struct.unpack("<d", struct.pack("<Q", b))[0]; hi = struct.unpack("<d", struct.pack("<Q", b + 1))[0]
            mid = (Fraction(lo) + Fraction(hi)) / 2
            if rng.random() < 0.5 and mid.denominator.bit_length() < 1200 and mid.numerator.bit_length() < 1200:
                # scale to an integer numerator over a power of ten
                k = max(mid.denominator.bit_length() - 1, 0)
                num = mid.numerator * 5 ** k
                s = str(num)
                s = (s[:-k] or "0") + "." + s[-k:].rjust(k, "0") if k else s
                out.append(s + rng.choice(["", "0", "1", "0000000000000000000001"]))
            else:
                out.append(repr(lo))
        elif t == 4: out.append("0x%x.%xp%d" % (rng.getrandbits(rng.randrange(1, 80)), rng.getrandbits(rng.randrange(1, 80)), rng.randrange(-1200, 1100)))
        elif t == 5: out.append("%d%s" % (rng.getrandbits(rng.randrange(1, 200)), rng.choice(["", "e-30", "e5", ".5"])))
        elif t == 6: out.append("0." + "0" * rng.randrange(0, 330) + str(rng.getrandbits(64)))
        else: out.append("".join(rng.choice("0123456789.eE+-xXpPinfatyINFANb \t()") for _ in range(rng.randrange(1, 10))))
    return out


# the hand-written list of test_sscanf_lf_against_glibc
SSCANF_CASES = ["1e", "1e+", "0x", "0x1p", "0x.8", "0x.", "0xg", "1.", ".5", ".", "+.e1", "inf", "infinity", "infinit", "infx", "in",
                "nan", "nan(abc)", "nan(", "  12", "1_000", "", "-", "+", "-0", "1e400", "0x1P+", "-inf", "+nan", "1..2", "1e1e1",
                "1d5", "infinityx", "1e-", ".e5", "0.e", "5e 3", "0x.p1", "- 1", "i", "n", "na", "INF", "iNfInItY", "0X.", "12\x0034"]

# ------------------------------------------------------------------------------------------ moved here from test_numconv_int.py
EDGES = [b"", b" ", b"0", b"-0", b"+0", b"  -0", b"7", b" 7", b"\t7", b"\n7", b"\v7", b"\f7", b"\r7", b"\x0b\x0c \t\r\n-7", b"\x1c7", b"\xa07",
         b"-", b"+", b"-+1", b"+-1", b"--1", b"- 1", b"1 2", b"12abc", b"abc", b"1.5", b"1e3", b"0x", b"0X", b"0xg", b"0x g", b"0x1f", b"0X1F", b"-0x1f",
         b"+0x", b"0x-1", b"x1f", b"00x1f", b"0b1", b"1f", b"ff", b"g", b"9223372036854775806", b"9223372036854775807",
         b"9223372036854775808", b"-9223372036854775807", b"-9223372036854775808", b"-9223372036854775809", b"18446744073709551614",
         b"18446744073709551615", b"18446744073709551616", b"18446744073709551617", b"-18446744073709551615", b"-18446744073709551616",
         b"-1", b"7fffffffffffffff", b"8000000000000000", b"-8000000000000000", b"-8000000000000001", b"ffffffffffffffff",
         b"0xffffffffffffffff", b"10000000000000000", b"0x10000000000000001", b"123456789012345678901234567890",
         b"-123456789012345678901234567890", b"abcdefabcdefabcdefabcdefabcdef", b"1\x002", b"\x001", b" \x00 1", b"0x\x001", b"12\x00",
         b"0" * 40 + b"5", b"-" + b"0" * 40 + b"5", b"0x" + b"0" * 40 + b"f"]

NANS = [b"nan", b"-nan", b"nan()", b"nan(0)", b"nan(1)", b"-nan(1)", b"nan(0x12)", b"NAN(0X7ffffffffffff)", b"nan(0xfffffffffffff)", b"nan(0x8000000000000)",
        b"nan(0xffffffffffffffff)", b"nan(0x1ffffffffffffffff)", b"nan(123)", b"nan(0123)", b"nan(08)", b"nan(abc)", b"nan(12ab)", b"nan(0x)", b"nan(0xg)",
        b"nan(_)", b"nan(1_)", b"nan(0b1)", b"nan(18446744073709551615)", b"nan(99999999999999999999)", b"nan(2251799813685248)", b"nan(2251799813685247)",
        b"nan(12", b"nan(1 )", b"nan(-1)", b"nan(+1)", b"nan( 1)", b"nan(1)x", b"  +nan(7)rest", b"nan(0x12", b"nan(\x00)"]


def gen_int_strings(r, n):
    """the strings of test_200000_random_strings, in its order of draws"""
    alphabet = b"0123456789" * 3 + b"abcdefABCDEFxX" + b"+- \t\n\v\f\r" + b"gz.\x00\xff"
    heads = [b"", b"", b"", b" ", b"-", b"+", b"0x", b"-0x", b" 0X", b"\t-", b"1844674407370955161", b"922337203685477580", b"-922337203685477580",
             b"ffffffffffffffff", b"7fffffffffffffff"]
    for _ in range(n):
        k = r.choice((0, 1, 2, 3, 5, 8, 17, 19, 20, 21, 33))
        yield r.choice(heads) + bytes(r.choice(alphabet) for _ in range(k))


# the hand-written lists of test_casts
CAST_I64 = [0, 1, -1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 63 - 1, -2 ** 63, 2 ** 63 - 513, 2 ** 63 - 512, 9007199254740993]
CAST_U64 = [0, 1, 2 ** 63, 2 ** 64 - 1, 2 ** 64 - 1024, 2 ** 64 - 1025, 2 ** 63 + 1025]
CAST_D2U_IN_RANGE = (0.9, -0.9, 1.5, 2.0 ** 63 - 1024, 2.0 ** 63, 2.0 ** 64 - 2048, 123.456)
_MIN = 1 << 63
# outside the targets' ranges: x86-64's answers
CAST_X86_I64 = ((float("nan"), _MIN), (float("inf"), _MIN), (float("-inf"), _MIN), (2.0 ** 63, _MIN), (-(2.0 ** 63), _MIN), (1e300, _MIN), (-1e300, _MIN))
CAST_X86_U64 = ((float("nan"), _MIN), (float("inf"), 0), (float("-inf"), _MIN), (2.0 ** 64, 0), (1e300, 0), (-1.0, M64), (-1.5, M64), (-5.0, M64 - 4),
                (-(2.0 ** 63), _MIN), (-1e300, _MIN))


# ------------------------------------------------------------------------------------------ the power-of-five table and the product
@functools.lru_cache(None)
def pow5_table():
    words = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{16})ull", open(os.path.join(CSRC, "pow5_table.inc")).read())]
    assert len(words) == 2 * (308 + 342 + 1)
    return words


def el_product(w, q):
    """eisel_lemire's product for w * 10^q (-342 <= q <= 308) restated: (hi, lo, refined, doubt, p2)"""
    t = pow5_table()
    lz = 64 - w.bit_length()
    w <<= lz
    i = 2 * (q + 342)
    p = w * t[i]
    hi, lo = p >> 64, p & M64
    refined = (hi & 0x1FF) == 0x1FF
    if refined:
        hi2 = (w * t[i + 1]) >> 64
        lo = (lo + hi2) & M64
        if hi2 > lo: hi += 1
    doubt = lo == M64 and not -27 <= q <= 55
    p2 = ((217706 * q) >> 16) + 63 + (hi >> 63) - lz + 1023
    return hi, lo, refined, doubt, p2


def doubt_pairs():
    """(w, q): 19-digit significands whose product with the table's word for 5^q has a low word of all ones, outside the exponents
    whose power of five is exact -- eisel_lemire cannot decide them.  w = -T^-1 mod 2^64 for an odd table word T"""
    t = pow5_table()
    out = []
    for q in range(-342, 309):
        T = t[2 * (q + 342)]
        if -27 <= q <= 55 or not T & 1: continue
        w = (-pow(T, -1, 1 << 64)) & M64
        if (1 << 63) <= w < 10 ** 19:
            out.append((w, q))
    return out


def doubt_family():
    """the doubt pairs as texts: as they are, with a leading '-', with the '.' moved inside the digits, with a 20th digit.  NOT part of
    scan_corpus(): without the exact path they answer NC_NEED_EXACT at once, but with it dec_to_bits starts its search for the neighbouring
    doubles at the encoding 0 when eisel_lemire reports doubt and does not come back (tests/test_numconv.py)"""
    out = []
    for w, q in doubt_pairs():
        d = str(w)
        out += ["%se%d" % (d, q), "-%se%d" % (d, q), "%s.%se%d" % (d[:1], d[1:], q + 18), "%s.%se%d" % (d[:10], d[10:], q + 9)]
        out += ["%s%se%d" % (d, x, q - 1) for x in "059"]
    return [s.encode() for s in out]


# ------------------------------------------------------------------------------------------ references
_libc = ctypes.CDLL(None)
_strtod = _libc.strtod
_strtod.restype = ctypes.c_double
_strtod.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
_sscanf = _libc.sscanf
_strtoimax, _strtoumax = _libc.strtoimax, _libc.strtoumax
_strtoimax.restype = ctypes.c_longlong
_strtoimax.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
_strtoumax.restype = ctypes.c_ulonglong
_strtoumax.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]


def glibc_strtod(s):
    """(status, bits, consumed) of strtod over the C string s (an embedded NUL ends it)"""
    buf = ctypes.create_string_buffer(s)
    end = ctypes.c_void_p()
    v = ctypes.c_double(_strtod(ctypes.addressof(buf), ctypes.byref(end)))
    used = end.value - ctypes.addressof(buf)
    return (NC_OK if used else NC_FAIL), ctypes.c_uint64.from_buffer(v).value, used


def glibc_sscanf(s):
    """(status, bits, consumed) of sscanf(s, "%lf%n")"""
    v = ctypes.c_uint64(0)
    used = ctypes.c_int(0)
    r = _sscanf(ctypes.create_string_buffer(s), b"%lf%n", ctypes.byref(v), ctypes.byref(used))
    return (NC_OK if r == 1 else NC_FAIL), v.value, used.value


def glibc_scan(s, mode):
    """what scan_double has to answer in `mode`: glibc's status and consumed; its bits too, except that without MODE_NAN_PAYLOAD a NaN is
    the plain quiet one with its sign.  `consumed` is strtod's end pointer in both modes (numconv.hpp, ScanResult): where sscanf converts,
    the bytes it read beyond that ("0x." is read whole and converts as "0") are not part of the number"""
    st, bits, used = glibc_strtod(s)
    if mode & 0xff == MODE_SSCANF:
        st, sbits, _ = glibc_sscanf(s)
        if st != NC_OK: used = 0
        elif sbits & ~SIGN <= INF_BITS: bits = sbits       # (a NaN's payload is strtod's in both modes: vfscanf stops in front of the '(')
        else: assert bits & ~SIGN > INF_BITS and (bits ^ sbits) & SIGN == 0, s
    if st == NC_OK and bits & ~SIGN > INF_BITS and not mode & NAN_PAYLOAD:
        bits = (bits & SIGN) | NAN_BITS
    return st, bits, used


def round_fraction(f):
    """the binary64 encoding nearest to the Fraction f >= 0 (ties to even)"""
    try:
        return f2b(f.numerator / f.denominator)             # int / int: correctly rounded
    except OverflowError:
        return INF_BITS


def exact_bits(prefix):
    """the binary64 encoding of the accepted prefix of a scan (bytes: spaces, sign, a decimal or hexadecimal number), by exact rational
    arithmetic; None for inf and nan, which are not numbers.  Exponents too large for a Fraction are decided by the position of the leading
    digit: 10^310 and 2^1025 are past DBL_MAX, 10^-400 and 2^-1100 below half the smallest subnormal"""
    t = prefix.decode("latin1").lstrip(" \t\n\v\f\r").lower()
    sign = 0
    if t[:1] in ("-", "+"):
        sign = SIGN if t[0] == "-" else 0
        t = t[1:]
    if t[:1] in ("i", "n"): return None
    hexa = t.startswith("0x")
    if hexa: t = t[2:]
    dg = "[0-9a-f]" if hexa else "[0-9]"
    m = re.fullmatch(r"(%s*)(?:\.(%s*))?(?:%s([-+]?[0-9]+))?" % (dg, dg, "p" if hexa else "e"), t)
    assert m and (m.group(1) or m.group(2)), prefix
    ip, fp, ex = m.group(1), m.group(2) or "", int(m.group(3) or 0)
    base, ebase, per = (16, 2, 4) if hexa else (10, 10, 1)
    num = int(ip + fp, base)
    if num == 0: return sign
    ex -= per * len(fp)
    lead = ex + (num.bit_length() - 1 if hexa else len(str(num)) - 1)      # exponent of the leading bit / digit
    if lead > (1030 if hexa else 320): return sign | INF_BITS
    if lead < (-1100 if hexa else -400): return sign
    f = Fraction(num) * Fraction(ebase) ** ex
    return sign | round_fraction(f)


def ref_f6(bits, cap):
    """printf("%f") of the binary64 `bits`, cut at cap characters"""
    mag = bits & ~SIGN
    if mag >= INF_BITS:
        t = ("-" if bits & SIGN else "") + ("inf" if mag == INF_BITS else "nan")
    else:
        with localcontext() as c:
            c.prec = 400
            t = format(Decimal(b2f(bits)).quantize(Decimal("0.000001"), rounding=ROUND_HALF_EVEN), "f")
    return t.encode()[:max(cap, 0)]


def ref_intmax(s, base, signed):
    """strtoimax / strtoumax (base 10 or 16) over the bytes s, as the 64 bits of the answer: isspace bytes, one sign, with base 16 an
    optional 0x in front of a digit or not; no digit is 0; overflow saturates; the unsigned scan negates modulo 2^64; a NUL ends s"""
    s = s.split(b"\x00")[0]
    i = 0
    while i < len(s) and s[i] in b" \t\n\v\f\r": i += 1
    neg = False
    if i < len(s) and s[i] in b"+-":
        neg = s[i] == 0x2d
        i += 1
    if base == 16 and s[i:i + 2].lower() == b"0x": i += 2
    v, any_ = 0, False
    while i < len(s):
        d = "0123456789abcdef".find(chr(s[i]).lower())
        if d < 0 or d >= base: break
        v = v * base + d
        any_ = True
        i += 1
    if not any_: return 0
    if signed:
        lim = (1 << 63) if neg else (1 << 63) - 1
        return (-min(v, lim) if neg else min(v, lim)) & M64
    if v > M64: return M64
    return (-v if neg else v) & M64


def libc_intmax(s, base, signed):
    return (_strtoimax(s, None, base) & M64) if signed else _strtoumax(s, None, base)


def ref_d2i(v):
    """(int64_t) v: (bits, undef) -- the C cast inside the range, x86-64's INT64_MIN outside it (and for -2^63 itself, counted with them)"""
    if v != v or abs(v) >= 2.0 ** 63: return _MIN, 1
    return int(v) & M64, 0


def ref_d2u(v):
    """(uint64_t) v as gcc compiles it for x86-64: below 2^63 cvttsd2si of v, from there on cvttsd2si(v - 2^63) with the top bit flipped"""
    if v != v: return _MIN, 1
    if v >= 2.0 ** 64: return 0, 1
    if v <= -(2.0 ** 63): return _MIN, 1
    return int(v) & M64, 1 if v <= -1.0 else 0


# ------------------------------------------------------------------------------------------ the scan_double corpus
def dec_str(f):
    """the exact decimal expansion of a Fraction whose denominator is a power of two"""
    k = f.denominator.bit_length() - 1
    s = str(f.numerator * 5 ** k)
    return (s[:-k] or "0") + "." + s[-k:].rjust(k, "0") if k else s


def midpoint(b):
    """the exact decimal expansion of the midpoint between the doubles with encodings b and b + 1 (b + 1 = inf stands for 2^1024)"""
    hi = Fraction(2) ** 1024 if b + 1 == INF_BITS else Fraction(b2f(b + 1))
    return dec_str((Fraction(b2f(b)) + hi) / 2)


def sig_digits(s):
    return len(s.replace(".", "").lstrip("0"))


MIDPOINT_EDGES = [0, 1, 2, 0x000FFFFFFFFFFFFE, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x0010000000000001, 0x7FEFFFFFFFFFFFFE, 0x7FEFFFFFFFFFFFFF]


def midpoint_encodings():
    r = random.Random(767)
    bs = list(MIDPOINT_EDGES)
    for i in range(40):                                   # both parities, every magnitude; few of the long ones (they cost text)
        e = r.choice((1, 2, 3, 40, 300)) if i < 6 else (r.randrange(700, 1075) if i < 34 else r.randrange(1076, 2046))
        bs.append((e << 52 | r.getrandbits(52)) & ~1 | (i & 1))
    return bs


@functools.lru_cache(None)
def scan_corpus():
    """[(family, bytes)]: the texts of the scan_double tests.  A text is one case: its length is the `len` the scanner gets"""
    r = random.Random(20261020)
    out = []
    add = lambda fam, s: out.append((fam, s.encode("latin1") if isinstance(s, str) else s))
    # ---- decimal, exact path
    mids = midpoint_encodings()
    for b in mids:
        m = midpoint(b)
        fam = "midpoint/even" if b % 2 == 0 else "midpoint/odd"
        # as it is, with 0 or 1 appended (behind a '.' where the midpoint is a whole number), with its last digit lowered by one
        if "." in m:
            assert m[-1] == "5"
            variants = (m, m + "0", m + "1", m[:-1] + "4")
        else:
            variants = (m, m + ".0", m + ".1", str(int(m) - 1))
        for s in variants:
            add(fam, s)
    # (the longest expansion of a binary64 has 767 significant digits; a midpoint has one bit, and one digit, more)
    assert max(sig_digits(midpoint(b)) for b in mids) == 768 < MAX_SIG_DIGITS
    for b in (1, 2, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x3FF0000000000000, 0x3FF0000000000001, 0x7FEFFFFFFFFFFFFF):
        m = midpoint(b)
        for pos in (MAX_SIG_DIGITS, MAX_SIG_DIGITS + 1, 1200):
            add("midpoint/pad%d" % pos, (m if "." in m else m + ".") + "0" * (pos - 1 - sig_digits(m)) + "1")
    for w, q in [(9007199254740993000, -3), (1234567890123456789, 0), (9586467486297153594, -46), (9734559530549076844, -224), (9792353653691471312, 270)]:
        for d, qq in ((str(w), q), (str(w) + "5", q - 1)):
            for pos in range(len(d) + 1):
                add("sig19_20", "%s.%se%d" % (d[:pos], d[pos:], qq + len(d) - pos))
            add("sig19_20", "000%se%d" % (d, qq))
            add("sig19_20", "0.000%se%d" % (d, qq + len(d) + 3))
            add("sig19_20", "00.%se%d" % (d, qq + len(d)))
    for sci in (310, 311, 320, 326, 327, 400):
        d = "".join(r.choice("0123456789") for _ in range(399))
        add("early_exit", "%s%se%d" % (r.choice("123456789"), d, sci - 399))
        add("early_exit", "%s.%se%d" % (r.choice("123456789"), d, sci))
    for sci in (-324, -325, -326, -327, -328, -340, -345, -400):
        d = "".join(r.choice("0123456789") for _ in range(399))
        add("early_exit", "0.%s%s%s" % ("0" * (-sci - 1), r.choice("123456789"), d))
        add("early_exit", "%s.%se%d" % (r.choice("123456789"), d, sci))
    for s in ("1e100000000", "1e99999999", "1e-99999999", "1e-100000000", "1e1000000000000", "1e-1000000000000", "1e99999999999999999999",
              "1e-99999999999999999999", "0e99999999999999999999", "0." + "0" * 400 + "1e401", "1" + "0" * 400 + "e-400",
              "0." + "0" * 400 + "1e100000000", "1" + "0" * 400 + "e-100000000", "123456789012345678901234567890e-100000020"):
        add("exp_clamp", s)
    # ---- Eisel-Lemire
    n = 0
    while n < 64:
        w, q = r.randrange(10 ** 18, 10 ** 19), r.randrange(-342, 309)
        if el_product(w, q)[2]:
            add("el_refine", "%de%d" % (w, q)); n += 1
    for q in (-344, -343, -342, -341, 307, 308, 309, 310):
        for w in (1, 2, 7, 17, 10 ** 18 + 1, 2470328229206232721, 4940656458412465442, 9999999999999999999):
            add("q_edge", "%de%d" % (w, q))
    for shift in (62, 63, 64, 65):
        n = 0
        while n < 6:
            q = r.randrange(-342, -300)
            w = r.getrandbits(r.randrange(1, 64)) | 1
            if w < 10 ** 19 and 1 - el_product(w, q)[4] == shift:
                add("subnormal_shift/%d" % shift, "%de%d" % (w, q)); n += 1
    # ---- hexadecimal
    for s in ("0x1.0000000000000000001p0", "0x1234567890abcdef1p0", "0x1234567890abcdef0001p-20", "0x1.00000000000008000000000000001p0",
              "0x123456789abcdef.123456789abcdefp-30", "0xfffffffffffffffffp0", "0x.00000000000000000000fffffffffffffffffp80"):
        add("hex/sticky", s)
    for s in ("0x1.00000000000008p0", "0x1.00000000000018p0", "0x1.fffffffffffff8p0", "0x1.ffffffffffffe8p0", "0x20000000000001p0", "0x20000000000003p0",
              "0x1.00000000000008p-1022", "0x0.00000000000018p-1022", "0x0.00000000000008p-1022"):
        add("hex/tie", s)
    for s in ("0x1p-1074", "0x1p-1075", "0x1.8p-1075", "0x.8p-1073", "0x1.fffffffffffff8p1023", "0x1p1024", "0x1.fffffffffffff7p1023", "0x1.0000000000001p-1075",
              "-0x1p-1075", "0x1p-1076", "0x1p1023", "0X1P+3", "0x0p0", "-0x0.0p5"):
        add("hex/edge", s)
    for s in ("0x1p100000000", "0x1p-100000000", "0x1p99999999999", "0x1p-99999999999", "0x0p99999999999", "0x1p99999999", "0x1p-99999999",
              "0x" + "0" * 300 + "1p-1000", "0x1" + "0" * 300 + "p-1200", "0x." + "0" * 300 + "1p1200"):
        add("hex/clamp", s)
    for s in ("0x", "0x.", "0x.p1", "0xp1", "-0x", "0x.g", " 0X", "0x+1"):
        add("hex/empty", s)
    # ---- grammar
    for s in SSCANF_CASES:
        add("grammar", s)
    for s in NANS:
        add("nans", s)
    for s in (b"12\x0034", b"1.5\x00e5", b"\x001", b"0x1\x00p3", b"nan(\x00)", b"1e\x005", b"inf\x00inity", b"123456789012345678\x009e5"):
        add("nul", s)
    # a length that ends inside a number: the rest of the number is the next case's text
    for a, b_ in (("1e", "5"), ("123", "456"), ("1e+", "3"), ("0x1p", "4"), ("0x", "8"), ("1.", "5e3"), ("inf", "inity"), ("nan(", "1)"),
                  ("9007199254740992", "1"), ("12345678901234567890123", "e5"), ("-", "1"), ("", "7")):
        add("len_cut", a)
        add("len_cut/rest", b_)
    for s in gen_cases(r, 1200):
        add("fuzz", s)
    return out


SCAN_FAMILIES = ["midpoint/even", "midpoint/odd"] + ["midpoint/pad%d" % p for p in (MAX_SIG_DIGITS, MAX_SIG_DIGITS + 1, 1200)] + \
    ["sig19_20", "early_exit", "exp_clamp", "el_refine", "q_edge"] + ["subnormal_shift/%d" % s for s in (63, 64)] + \
    ["hex/sticky", "hex/tie", "hex/edge", "hex/clamp", "hex/empty", "grammar", "nans", "nul", "len_cut", "fuzz"]


def pack(texts):
    """the texts back to back, and their offsets"""
    off = [0]
    for t in texts:
        off.append(off[-1] + len(t))
    return b"".join(texts), off


def check_scan(texts, mode, exact, got, ref=None):
    """got = [(status, bits, consumed)] for texts in `mode`: glibc's status and consumed, the exact bits for numbers and glibc's for the
    rest; NC_NEED_EXACT only without `exact`, and never instead of a failure.  Returns the indices that answered NC_NEED_EXACT"""
    need = []
    for i, (s, (st, bits, used)) in enumerate(zip(texts, got)):
        wst, wbits, wused = ref[i] if ref else glibc_scan(s, mode)
        if st == NC_NEED_EXACT:
            assert not exact and wst == NC_OK and used == wused, (s, mode, st, used, wused)
            need.append(i)
            continue
        assert (st, used) == (wst, wused), (s, mode, exact, (st, used), (wst, wused))
        if st != NC_OK: continue
        assert bits == wbits, (s, mode, exact, hex(bits), hex(wbits))
        eb = exact_bits(s.split(b"\x00")[0][:used])
        assert eb is None or eb == bits, (s, mode, exact, hex(bits), hex(eb))
    return need


# ------------------------------------------------------------------------------------------ the formatting corpora
F6_STRIDE = 512
F6_CAP = 400


@functools.lru_cache(None)
def f6_corpus():
    """[(family, bits, cap)]"""
    r = random.Random(6)
    out = []
    def add(fam, v, cap=F6_CAP):
        out.append((fam, v if isinstance(v, int) else f2b(v), cap))
    for m in range(1, 128, 2):                               # m / 128 = 0.0078125 m: seven decimals, the seventh a 5
        for base in (0, 1, 7, 999999, 2 ** 20, 2 ** 40 + 1, 2 ** 45 - 1):
            add("tie", base + m / 128.0)
            add("tie", -(base + m / 128.0))
    for v in (0.9999995, 9.9999995, 999999.9999995, 0.0000005, 0.0000015, 0.5000005, 99.9999995, 0.99999949999999994, 1e15 + 0.5):
        for d in (-1, 0, 1):
            add("carry", f2b(v) + d)
    for e in range(1, 2047):                                 # every binade twice: 1075 - e is the divisor's exponent k
        for _ in range(2):
            add("binade", e << 52 | r.getrandbits(52) | r.getrandbits(1) << 63)
    for v in (1e-6, 5e-7, 4.9999999999999998e-7, 5.0000000000000004e-7, 2.0 ** -64, 2.0 ** -63, 2.0 ** -65, 2.0 ** -127, 2.0 ** -128, 2.0 ** -129,
              2.0 ** -20, 2.0 ** -21, 1.5 * 2.0 ** -20, 2.0 ** -11, 2.0 ** -12):
        for d in (-1, 0, 1):
            add("divisor", f2b(v) + d)
    for b in (1, 2, 0x000FFFFFFFFFFFFF, 0x0008000000000000, SIGN | 1, SIGN | 0x000FFFFFFFFFFFFF):
        add("subnormal", b)
    for b in (0, SIGN, INF_BITS, SIGN | INF_BITS, NAN_BITS, SIGN | NAN_BITS, NAN_BITS | 0x123, INF_BITS | 1, SIGN | INF_BITS | 1):
        add("special", b)
    for k in range(0, 1024, 31):
        add("integer", 2.0 ** k)
        add("integer", -(2.0 ** k) * 1.5)
    for v in (1.7976931348623157e308, -1.7976931348623157e308, 1e22, 1e23, 1e300, 2.0 ** 53 + 2, 2.0 ** 63, 2.0 ** 64, 999999999.0, 1000000000.0, 1e18):
        add("integer", v)
    for v in (1.5, -1.5, 0.0, -0.0, 123456789.987654321, 1.7976931348623157e308, -1.7976931348623157e308, 5e-324, 1e250, float("inf"), float("-inf"),
              b2f(SIGN | NAN_BITS), 999999.9999995, 2.0 ** 830):
        n = len(ref_f6(f2b(v), 10 ** 6))
        for cap in (0, 1, 2, 251, 400, L2M_LABEL_MAX, n - 1, n, n + 1):
            add("cap", v, cap)
    return out


F6_FAMILIES = ["tie", "carry", "binade", "divisor", "subnormal", "special", "integer", "cap"]


def f6_divisor_branch(bits):
    """which of fmt_f6's three divisor branches a finite value with a fraction takes (None: it prints as an integer)"""
    mag = bits & ~SIGN
    e = mag >> 52
    k = 1074 if e == 0 else 1075 - e
    if mag >= INF_BITS or k <= 0 or mag == 0: return None
    return "k<64" if k < 64 else ("64<=k<128" if k < 128 else "k>=128")


@functools.lru_cache(None)
def json_corpus():
    """[bits]: fmt_chunks' float list, 2 000 random bit patterns, and the float32-widened forms of both"""
    import fmt_chunks
    r = random.Random(16)
    vals = [f2b(v) for v in fmt_chunks.float_list()] + [r.getrandbits(64) for _ in range(2000)]
    wide = []
    for b in vals:
        v = b2f(b)
        try:
            f = struct.unpack("<f", struct.pack("<f", v))[0]
        except OverflowError:
            f = float("inf") if v > 0 else float("-inf")
        wide.append(f2b(f))
    return vals + wide


def ref_json(bits, nan_to_null):
    import fmt_chunks
    return fmt_chunks.py_float_rule(b2f(bits), nan_to_null).encode()


@functools.lru_cache(None)
def int_texts():
    return list(EDGES) + list(gen_int_strings(random.Random(20261018), 20000))


def ld_values():
    """fmt_ld's inputs as 64-bit patterns"""
    vals = [0, 1, -1, 2 ** 63 - 1, -2 ** 63]
    for k in range(0, 19):
        vals += [10 ** k - 1, 10 ** k, -(10 ** k - 1), -(10 ** k)]
    return [v & M64 for v in vals]


def lu_values():
    vals = [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]
    for k in range(0, 20):
        vals += [10 ** k - 1, 10 ** k]
    return vals


@functools.lru_cache(None)
def cast_corpus():
    """(i64 patterns, u64 values, double bit patterns)"""
    r = random.Random(11)
    i64 = [v & M64 for v in CAST_I64 + [r.randrange(-2 ** 63, 2 ** 63) for _ in range(2000)]]
    u64 = CAST_U64 + [r.getrandbits(64) for _ in range(2000)] + [(1 << k) + d for k in range(53, 64) for d in (-1, 0, 1, (1 << (k - 53)), (1 << (k - 53)) + 1)]
    dbl = [f2b(v) for v in CAST_D2U_IN_RANGE] + [f2b(v) for v, _ in CAST_X86_I64 + CAST_X86_U64] + [r.getrandbits(64) for _ in range(2000)]
    dbl += [f2b(float(r.randrange(-2 ** 64, 2 ** 64)) / r.choice((1, 3, 1024))) for _ in range(2000)]
    dbl += [f2b(v) + d for v in (2.0 ** 63, -(2.0 ** 63), 2.0 ** 64, -1.0, 1.0, 0.0, -0.0, 2.0 ** 53) for d in (-1, 0, 1) if f2b(v) + d >= 0]
    return i64, u64, dbl


# ------------------------------------------------------------------------------------------ the host instantiation
def host_lib():
    import flbamd_loader
    L = flbamd_loader.load().lib()
    L.flbgpu_nc_scan_double.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    L.flbgpu_nc_scan_intmax.restype = ctypes.c_ulonglong
    L.flbgpu_nc_scan_intmax.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.flbgpu_nc_fmt_f6.argtypes = [ctypes.c_double, ctypes.c_char_p, ctypes.c_int]
    L.flbgpu_nc_fmt_json_double.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_char_p]
    L.flbgpu_nc_fmt_ld.argtypes = [ctypes.c_longlong, ctypes.c_char_p]
    L.flbgpu_nc_fmt_lu.argtypes = [ctypes.c_ulonglong, ctypes.c_char_p]
    L.flbgpu_nc_int_to_double.restype = ctypes.c_double
    L.flbgpu_nc_int_to_double.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
    L.flbgpu_nc_double_to_int.restype = ctypes.c_ulonglong
    L.flbgpu_nc_double_to_int.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return L


def host_scan(L, texts, mode, exact):
    """[(status, bits, consumed)]"""
    out, used, res = ctypes.c_double(), ctypes.c_int(), []
    view = ctypes.c_uint64.from_buffer(out)
    for s in texts:
        st = L.flbgpu_nc_scan_double(s, len(s), mode, exact, ctypes.byref(out), ctypes.byref(used))
        res.append((st, view.value, used.value))
    return res


def host_intmax(L, texts, base, signed):
    return [L.flbgpu_nc_scan_intmax(s, len(s), base, signed) for s in texts]


def _dbl(bits):
    return ctypes.c_double.from_buffer(ctypes.c_uint64(bits))


def host_text(L, op, vals, caps=None, p0=0):
    """[(count, text)] of a formatting operation over 64-bit patterns"""
    buf, res = ctypes.create_string_buffer(F6_STRIDE), []
    for i, v in enumerate(vals):
        if op == OP_FMT_F6: n = L.flbgpu_nc_fmt_f6(_dbl(v), buf, caps[i])
        elif op == OP_FMT_JSON: n = L.flbgpu_nc_fmt_json_double(_dbl(v), p0, buf)
        elif op == OP_FMT_LD: n = L.flbgpu_nc_fmt_ld(v - (1 << 64) if v >> 63 else v, buf)
        else: n = L.flbgpu_nc_fmt_lu(v, buf)
        res.append((n, buf.raw[:n]))
    return res


def host_cast(L, op, vals):
    """[(out, undef)]"""
    res, u = [], ctypes.c_int()
    for v in vals:
        if op in (OP_I2D, OP_U2D):
            d = ctypes.c_double(L.flbgpu_nc_int_to_double(v, 1 if op == OP_I2D else 0))
            res.append((ctypes.c_uint64.from_buffer(d).value, 0))
        else:
            r = L.flbgpu_nc_double_to_int(_dbl(v), 1 if op == OP_D2I else 0, ctypes.byref(u))
            res.append((r, u.value))
    return res


def check_intmax(texts, base, signed, got):
    for s, v in zip(texts, got):
        assert v == ref_intmax(s, base, signed), (s, base, signed, v)


def check_text(op, vals, got, caps=None, p0=0):
    for i, (v, (n, text)) in enumerate(zip(vals, got)):
        if op == OP_FMT_F6: want = ref_f6(v, caps[i])
        elif op == OP_FMT_JSON: want = ref_json(v, p0)
        elif op == OP_FMT_LD: want = str(v - (1 << 64) if v >> 63 else v).encode()
        else: want = str(v).encode()
        assert (n, text) == (len(want), want), (op, hex(v), caps[i] if caps else None, p0, text, want)


def check_cast(op, vals, got):
    for v, (out, undef) in zip(vals, got):
        if op == OP_I2D: want = (f2b(float(v - (1 << 64) if v >> 63 else v)), 0)
        elif op == OP_U2D: want = (f2b(float(v)), 0)
        elif op == OP_D2I: want = ref_d2i(b2f(v))
        else: want = ref_d2u(b2f(v))
        assert (out, undef) == want, (op, hex(v), out, undef, want)

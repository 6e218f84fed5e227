"""The host instantiations of numconv.hpp's integer scanners and of what filter_type_converter's float paths add (flbgpu_nc_*,
csrc/numconv_host.cpp) against glibc: strtoimax / strtoumax in base 10 and 16, "%lu", the float rule without the NaN-to-null
option against snprintf, scan_double's nan(n-char-sequence) payload mode against strtod, and the casts between 64-bit integers and
doubles against the machine's own."""
import ctypes
import random
import struct

import flbamd_loader
from numconv_cases import (CAST_D2U_IN_RANGE, CAST_I64, CAST_U64, CAST_X86_I64, CAST_X86_U64, EDGES, NANS, gen_int_strings)

g = flbamd_loader.load()
L = g.lib()
L.flbgpu_nc_scan_intmax.restype = ctypes.c_ulonglong
L.flbgpu_nc_scan_intmax.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
L.flbgpu_nc_fmt_lu.argtypes = [ctypes.c_ulonglong, ctypes.c_char_p]
L.flbgpu_nc_int_to_double.restype = ctypes.c_double
L.flbgpu_nc_int_to_double.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
L.flbgpu_nc_double_to_int.restype = ctypes.c_ulonglong
L.flbgpu_nc_double_to_int.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
L.flbgpu_nc_fmt_json_double.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_char_p]
L.flbgpu_nc_scan_double.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(ctypes.c_int)]
C = ctypes.CDLL(None)
C.strtoimax.restype = ctypes.c_longlong
C.strtoimax.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
C.strtoumax.restype = ctypes.c_ulonglong
C.strtoumax.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
C.strtod.restype = ctypes.c_double
C.strtod.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
M64 = (1 << 64) - 1
NAN_PAYLOAD = 0x100                                 # numconv.hpp MODE_NAN_PAYLOAD


def ours(s, base, signed):
    return L.flbgpu_nc_scan_intmax(s, len(s), base, signed)


def libc(s, base, signed):
    # (the reference scans a NUL-terminated copy: ctypes hands the bytes over the same way, an embedded NUL ends them)
    return (C.strtoimax(s, None, base) & M64) if signed else C.strtoumax(s, None, base)


def check(s):
    for base in (10, 16):
        for signed in (1, 0):
            assert ours(s, base, signed) == libc(s, base, signed), (s, base, signed)


def test_hand_picked_edges():
    for s in EDGES:
        check(s)
    # what the filter reads as a failure
    for s in (b"0", b"", b"  -0", b"0x", b"0xg", b"xyz"):
        assert ours(s, 10, 1) == ours(s, 10, 0) == ours(s, 16, 0) == 0
    assert ours(b"abc", 10, 1) == ours(b"abc", 10, 0) == 0 and ours(b"abc", 16, 0) == 0xabc       # (to hex, "abc" is a number)
    assert ours(b"-1", 10, 0) == M64 and ours(b"99999999999999999999", 10, 1) == (1 << 63) - 1
    assert ours(b"-99999999999999999999", 10, 1) == 1 << 63 and ours(b"-99999999999999999999", 10, 0) == M64
    # the length ends the text as a NUL does
    assert L.flbgpu_nc_scan_intmax(b"123456", 3, 10, 1) == 123


def test_200000_random_strings():
    r = random.Random(20261018)
    for s in gen_int_strings(r, 200000):
        check(s)


def test_fmt_lu():
    buf = ctypes.create_string_buffer(32)
    for v in (0, 1, 9, 10, 2 ** 32, 2 ** 63 - 1, 2 ** 63, M64, 10 ** 19, 10 ** 19 - 1):
        n = L.flbgpu_nc_fmt_lu(v, buf)
        assert buf.raw[:n] == b"%d" % v


def ref_float_text(v):
    """flb_typecast_conv_float's rule (src/flb_typecast.c:309-315) with the machine's own (long long) cast"""
    as_ll = L.flbgpu_nc_double_to_int(v, 1, None)
    as_ll = as_ll - (1 << 64) if as_ll >> 63 else as_ll
    buf = ctypes.create_string_buffer(512)
    n = C.snprintf(buf, 511, b"%.1f" if v == float(as_ll) else b"%.16g", ctypes.c_double(v))
    return buf.raw[:n]


def bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def test_float_to_string_against_snprintf():
    vals = [float("inf"), float("-inf"), bits(0x7ff8000000000000), bits(0xfff8000000000000), bits(0x7ff8000000000123), 0.0, -0.0, 2.0 ** 63,
            -(2.0 ** 63), 2.0 ** 63 - 1024, -(2.0 ** 63) + 1024, 1e22, 1e15, 1e16, 123.456, 0.1, -1.5, 5e-324, 1.7976931348623157e308, 2.0 ** 64, 1e-5]
    r = random.Random(7)
    vals += [bits(r.getrandbits(64)) for _ in range(20000)] + [float(r.randrange(-2 ** 62, 2 ** 62)) for _ in range(2000)]
    buf = ctypes.create_string_buffer(512)
    for v in vals:
        n = L.flbgpu_nc_fmt_json_double(v, 0, buf)
        assert buf.raw[:n] == ref_float_text(v), v
    assert ref_float_text(float("-inf")) == b"-inf" and ref_float_text(bits(0xfff8000000000000)) == b"-nan" and ref_float_text(-0.0) == b"-0.0"
    assert ref_float_text(2.0 ** 63) == b"9.223372036854776e+18" and ref_float_text(-(2.0 ** 63)) == b"-9223372036854775808.0"
    assert ref_float_text(1e22) == b"1e+22"


def scan(s, mode):
    d, used = ctypes.c_double(), ctypes.c_int()
    st = L.flbgpu_nc_scan_double(s, len(s), mode, 1, ctypes.byref(d), ctypes.byref(used))
    return st, struct.pack("<d", d.value), used.value


def test_nan_payload_mode_against_strtod():
    end = ctypes.c_char_p()
    for s in NANS:
        buf = ctypes.create_string_buffer(s)
        want = C.strtod(buf, ctypes.byref(end))
        used = ctypes.cast(end, ctypes.c_void_p).value - ctypes.addressof(buf)
        st, got, n = scan(s, NAN_PAYLOAD)
        assert (st, got, n) == (1, struct.pack("<d", want), used), s
        # the existing callers' mode: the plain quiet NaN with its sign, the same bytes consumed
        st0, got0, n0 = scan(s, 0)
        assert (st0, n0) == (1, used) and got0 in (struct.pack("<Q", 0x7ff8000000000000), struct.pack("<Q", 0xfff8000000000000))
    assert scan(b"nan(0x12)", NAN_PAYLOAD)[1] == struct.pack("<Q", 0x7ff8000000000012)
    # the flag changes nothing else
    r = random.Random(3)
    for _ in range(20000):
        s = ("%.17g" % bits(r.getrandbits(64))).encode()
        assert scan(s, NAN_PAYLOAD) == scan(s, 0)


def test_casts():
    r = random.Random(11)
    ints = CAST_I64 + [r.randrange(-2 ** 63, 2 ** 63) for _ in range(20000)]
    for v in ints:
        assert L.flbgpu_nc_int_to_double(v & M64, 1) == float(v)
    for v in CAST_U64 + [r.getrandbits(64) for _ in range(20000)]:
        assert L.flbgpu_nc_int_to_double(v, 0) == float(v)
    u = ctypes.c_int()
    # inside the targets' ranges: the C cast
    for _ in range(20000):
        v = bits(r.getrandbits(64))
        if v != v:
            continue
        if abs(v) < 2.0 ** 63:
            assert L.flbgpu_nc_double_to_int(v, 1, ctypes.byref(u)) == int(v) & M64 and u.value == 0
        if -1.0 < v < 2.0 ** 64:
            assert L.flbgpu_nc_double_to_int(v, 0, ctypes.byref(u)) == int(v) and u.value == 0
    for v in CAST_D2U_IN_RANGE:
        assert L.flbgpu_nc_double_to_int(v, 0, ctypes.byref(u)) == int(v) and u.value == 0
    # outside: x86-64's answers, counted
    for v, want in CAST_X86_I64:
        assert L.flbgpu_nc_double_to_int(v, 1, ctypes.byref(u)) == want and u.value == 1, v
    for v, want in CAST_X86_U64:
        assert L.flbgpu_nc_double_to_int(v, 0, ctypes.byref(u)) == want and u.value == 1, v

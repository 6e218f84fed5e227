"""filter_modify's regex compile verdicts (every rule key and value goes through flb_regex_create, plugins/filter_modify/modify.c:
478-507; condition patterns at :306-343) against the REAL src/flb_regex.c over the real Onigmo (oracle/_ref/libflbregex_ref.so):
the product, and the CPU model the other modify tests are held to, accept exactly the strings the reference accepts"""
import ctypes
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import modify_model as mm
import test_modify_frontend as fe

REF = os.path.join(HERE, "..", "oracle", "_ref", "libflbregex_ref.so")
pytestmark = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/libflbregex_ref.so not built (needs the reference tree)")

# the strings of the corpus: every token of the runtime cases and the front-end quirks, the fuzz words of test_modify_gpu.py, and
# patterns Onigmo refuses or that are not regular expressions
EXTRA = [b"*s3", b"[abc", b"(abc", b"a{2,1}", b"\\", b"(?=abc)x", b"(?<=a)b", b"^(?!a)", b"(a)\\1", b"(?>a+)", b"a++", b"/^A/i", b"/x/z",
         b"^k[0-9]$", b"x|y", b"[[:alpha:]]", b"\\p{Greek}", b"(?<n>a)\\k<n>", b"caf\xc3\xa9", b"\xe9", b"", b".*with spaces.*", b"true",
         b"ab\x01z", b"ref", b"[", b"]", b")", b"?", b"+a", b"a**", b"\\x{1F600}", b"(?i)abc", b"(?~abc)"]


def corpus():
    out = set(EXTRA)
    for c in fe.CASES:
        for _, v in c["props"]:
            out.update(mm.split_quoted(v) or [])
    for props in fe.QUIRKS:
        for _, v in props:
            out.update(mm.split_quoted(v) or [])
    return sorted(x for x in out if x and b" " not in x and b'"' not in x and b"'" not in x)


@pytest.fixture(scope="module")
def ref():
    L = ctypes.CDLL(REF)
    L.flb_regex_create.restype = ctypes.c_void_p
    L.flb_regex_create.argtypes = [ctypes.c_char_p]
    L.flb_regex_destroy.argtypes = [ctypes.c_void_p]
    return L


def test_compile_verdicts_match_onigmo(ref):
    g = flbamd_loader.load()
    checked = 0
    for s in corpus():
        r = ref.flb_regex_create(s)
        want = bool(r)
        if r:
            ref.flb_regex_destroy(r)
        # a Set value is only compiled, never run: the product takes what Onigmo takes
        try:
            g.modify_parse_check([("Set", b"k " + s)])
            got = True
        except ValueError:
            got = False
        assert mm.Regex.get(s).ok == want, s
        try:
            s.decode("utf-8")
        except UnicodeDecodeError:
            # the one documented difference: a string that is not UTF-8 is refused even where it is only compiled,
            # although Onigmo takes some of them
            assert not got, s
            continue
        assert got == want, s
        checked += 1
    assert checked >= 40

"""The C ABI of libflbgpu.so by name: the defined dynamic symbols that start with `flbgpu_` are the recorded list
(tests/golden/abi_symbols.txt: `nm -D --defined-only`, names only, sorted), and every function include/flb_gpu.h declares is among
them.  The host side is several translation units: an `extern "C"` definition that a move between them drops, or leaves behind
twice, has no caller inside the library that would notice."""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "fluent-bit_amd", "csrc", "libflbgpu.so")


def _defined():
    nm = shutil.which("nm")
    assert nm, "nm (binutils) is needed to read the library's dynamic symbols"
    out = subprocess.run([nm, "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    return [n for n in names if n.startswith("flbgpu_")]


def test_defined_symbols_are_the_recorded_list():
    got = _defined()
    assert len(got) == len(set(got)), sorted(n for n in set(got) if got.count(n) > 1)
    with open(os.path.join(HERE, "golden", "abi_symbols.txt")) as fh:
        want = fh.read().split()
    assert want == sorted(want)
    assert sorted(got) == want, {"missing": sorted(set(want) - set(got)), "new": sorted(set(got) - set(want))}


def test_every_declared_function_is_defined():
    with open(os.path.join(ROOT, "include", "flb_gpu.h")) as fh:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(flbgpu_\w+)\s*\(", text))
    assert len(declared) > 100                              # (the pattern still reads the header)
    assert not declared - set(_defined()), sorted(declared - set(_defined()))

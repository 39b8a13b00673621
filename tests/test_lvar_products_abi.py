"""The pair-keyed list variable's entry points at the C boundary, and its host walk, without a
GPU (include/laspj.h "pair-keyed list variables"; lasp_amd/csrc/laspj_host.cpp
list_walk_pairs)."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest

from lasp_amd import _lib, build
from oracle import etf as oetf
from oracle.terms import Atom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("laspj_lvar_create_pairs", "laspj_lvar_product", "laspj_lvar_product_recheck")
A = Atom


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (laspj_\w+)", out))
    for n in NAMES:
        assert n in exported and n in _lib.SIGNATURES and hasattr(lib, n)
    from lasp_amd import engine
    assert hasattr(engine.Context, "pair_list_var")
    assert hasattr(engine.NifListVar, "product") and hasattr(engine.NifListVar, "product_recheck")


def test_null_handles_answer_inval(lib):
    h = ctypes.c_void_p()
    st, verd, n, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.laspj_lvar_create_pairs(None, ctypes.byref(h)) == _lib.E_INVAL
    assert lib.laspj_lvar_create_pairs(None, None) == _lib.E_INVAL
    assert lib.laspj_lvar_product(None, None, None, ctypes.byref(st),
                                  ctypes.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_product_recheck(None, None, None, ctypes.byref(st), None, 0,
                                          ctypes.byref(n), ctypes.byref(w),
                                          ctypes.byref(verd)) == _lib.E_INVAL


def _raw_list(items: bytes, n: int, tail: bytes = b"\x6a") -> bytes:
    return b"\x6c" + n.to_bytes(4, "big") + items + tail


def _images():
    """(kind, image): V — taken and written back byte for byte; R — refused."""
    tb = oetf.term_to_binary
    t = lambda k: k.to_bytes(4, "big") + bytes(16)            # noqa: E731
    ok = [
        [],
        [((1, 2), [([t(1), t(2)], False)])],
        # a token of two small integers travels as STRING_EXT; an empty token list
        [((A("a"), b"bin"), [([1, 2], True), ([t(3), 7], False)]), (((0,), 2 ** 40), [])],
        # keys out of order and repeated, runs descending (what product/7 leaves)
        [((2, 0), [([t(9), t(8)], False), ([t(9), t(7)], True)]), ((1, 0), [([t(5), t(8)], False)]),
         ((2, 0), [([t(9), t(8)], True)])],
    ]
    out = [("V", tb(v)) for v in ok]
    body = tb([([t(1), t(2)], False)])[1:]                     # the token list of one entry
    pair = tb((1, 2))[1:]
    entry = lambda key, toks: b"\x68\x02" + key + toks         # noqa: E731
    refused = [
        tb([(1, [([t(1), t(2)], False)])]),                     # a key that is no tuple
        tb([((1, 2, 3), [([t(1), t(2)], False)])]),             # a 3-tuple key
        tb([((1, 2), [(t(1), False)])]),                        # a token that is a binary
        tb([((1, 2), [([t(1), t(2), t(3)], False)])]),          # a 3-element token list
        tb([((1, 2), [([t(1)], False)])]),                      # a 1-element token list
        tb([((1, 2), [([1, 2, 3], False)])]),                   # STRING_EXT of three
        tb([((1, 2), [([t(1), t(2)], A("maybe"))])]),           # a flag that is no boolean
        tb([((1, 2), [([t(1), t(2)], False)]), 7]),             # an entry that is no tuple
        tb([1, 2, 3]),                                          # a list of integers
        tb((1, 2)),                                             # not a list
        # improper lists: the value, the token list, the token itself ([Tx, Ty | Z])
        b"\x83" + _raw_list(entry(pair, body), 1, tail=tb(0)[1:]),
        b"\x83" + _raw_list(entry(pair, _raw_list(b"\x68\x02" + tb([t(1), t(2)])[1:] +
                                                  tb(False)[1:], 1, tail=tb(0)[1:])), 1),
        b"\x83" + _raw_list(entry(pair, _raw_list(
            b"\x68\x02" + _raw_list(tb(t(1))[1:] + tb(t(2))[1:], 2, tail=tb(t(3))[1:]) +
            tb(False)[1:], 1)), 1),
        # the second entry refused: the first one's registrations are undone
        tb([((A("new1"), A("new2")), [([t(40), t(41)], False)]), ((1, 2), [(t(1), False)])]),
        # `==`-equal terms under two images
        tb([((1, 2), [([t(1), t(2)], False)]), ((1.0, 2), [([t(1), t(2)], False)])]),
        # an element past 64 distinct tokens
        tb([((A("many"), 0), [([t(100 + k), t(1)], False) for k in range(65)])]),
        tb([((1, 2), [([t(1), t(2)], False)])])[:-3],           # truncated
    ]
    return out + [("R", r) for r in refused]


def test_pair_walk_under_host_sanitizers(tmp_path):
    """A stand-alone program over the host source, built with the address and undefined-
    behaviour sanitizers: valid pair images round-trip through list_walk_pairs and list_write,
    refused ones leave the dictionary as it was.  Nothing loaded into Python runs under a
    sanitizer."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    cands = [os.path.join(rocm, "llvm", "bin", "clang++"),
             os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("clang++")]
    cxx = next((c for c in cands if c and os.path.exists(c)), None)
    assert cxx is not None, "no host clang++ beside hipcc"
    images = _images()
    src = tmp_path / "images.txt"
    src.write_text("".join(f"{k} {img.hex()}\n" for k, img in images))
    exe = str(tmp_path / "pair_walk_check")
    # plain host C++ (the source holds no kernels): the HIP headers only declare
    cmd = [cxx, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "c", "pair_walk_check.cpp"),
           os.path.join(build.CSRC, "laspj_host.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert f"{len(images)} lines, 0 bad" in res.stdout

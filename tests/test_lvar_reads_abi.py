"""The list variables' lazy threads and one-pass reads at the C boundary (include/laspj.h
"list-valued resident variables": laspj_lvar_wait_needed / _read / _read_any / _lazy_count /
_lazy_at / _lazy_cancel): declared, exported, bound, and closed to null handles.  No GPU."""

import ctypes as C
import os

import pytest

from lasp_amd import _lib

NAMES = ["laspj_lvar_wait_needed", "laspj_lvar_read", "laspj_lvar_read_any",
         "laspj_lvar_lazy_count", "laspj_lvar_lazy_at", "laspj_lvar_lazy_cancel"]


@pytest.fixture(scope="module")
def lib():
    from lasp_amd import build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "laspj.h")).read()
    for name in NAMES:
        assert ("int %s(" % name) in hdr, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    assert "Lazy threads are not kept for it" not in hdr


def test_entry_points_reject_null_handles(lib):
    met, verd, found = C.c_int32(), C.c_int32(), C.c_int32()
    n32, still = C.c_uint32(), C.c_uint32()
    wid, ln, p = C.c_uint64(), C.c_uint64(), C.c_void_p()
    ids = (C.c_uint64 * 4)()
    nl = (C.c_uint32 * 1)()
    img = b"\x83j"
    assert lib.laspj_lvar_wait_needed(None, img, 2, 0, 7, C.byref(met),
                                      C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_read(None, img, 2, 0, 7, C.byref(met), ids, 4, C.byref(n32),
                               C.byref(still), C.byref(verd)) == _lib.E_INVAL
    lvs = (C.c_void_p * 1)(None)
    pv = (C.c_char_p * 1)(img)
    nv = (C.c_uint64 * 1)(2)
    st = (C.c_int32 * 1)(0)
    assert lib.laspj_lvar_read_any(None, 1, lvs, pv, nv, st, 7, C.byref(found), ids, 4, nl,
                                   C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_lazy_count(None, C.byref(n32)) == _lib.E_INVAL
    assert lib.laspj_lvar_lazy_at(None, 0, C.byref(wid), C.byref(p),
                                  C.byref(ln)) == _lib.E_INVAL
    assert lib.laspj_lvar_lazy_cancel(None, 7, C.byref(found)) == _lib.E_INVAL
    assert lib.laspj_abi_version() == 2           # additive: the version stands

"""List-valued resident variables at the C boundary (include/laspj.h "list-valued resident
variables"), without a GPU: the entry points are exported with the signatures _lib declares,
and each rejects a null handle before it touches a device."""

import ctypes as C

import pytest

from lasp_amd import _lib

NAMES = ("laspj_lvar_create", "laspj_lvar_destroy", "laspj_lvar_intersection",
         "laspj_lvar_etf_bind", "laspj_lvar_etf_write", "laspj_lvar_etf_read",
         "laspj_lvar_etf_value", "laspj_lvar_etf_threshold", "laspj_lvar_counts",
         "laspj_lvar_resident")


@pytest.fixture(scope="module")
def lib():
    from lasp_amd import build
    build.build()
    return _lib.load()


def test_entry_points_are_exported(lib):
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    assert _lib.BIND_REFUSED == 2 and _lib.TUNE_LVAR_PRODUCER == 16


def test_entry_points_reject_null_handles(lib):
    st, verd, res = C.c_int32(), C.c_int32(), C.c_int32()
    out, olen = C.c_void_p(), C.c_uint64()
    ne, nt = C.c_uint32(), C.c_uint32()
    h = C.c_void_p()
    img = b"\x83j"
    assert lib.laspj_lvar_create(None, C.byref(h)) == _lib.E_INVAL and not h
    assert lib.laspj_lvar_destroy(None) == _lib.E_INVAL
    assert lib.laspj_lvar_intersection(None, None, None, C.byref(st),
                                       C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_etf_bind(None, img, 2, C.byref(st), C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_etf_write(None, img, 2, C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_etf_read(None, C.byref(out), C.byref(olen),
                                   C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_etf_value(None, C.byref(out), C.byref(olen),
                                    C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_etf_threshold(None, img, 2, 0, C.byref(res),
                                        C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_counts(None, C.byref(ne), C.byref(nt)) == _lib.E_INVAL
    assert lib.laspj_lvar_resident(None, C.byref(res)) == _lib.E_INVAL
    assert lib.laspj_abi_version() == 2           # additive: the version stands

"""Resident map processes at the C boundary (include/laspj.h "resident map processes"),
without a GPU: the five entry points are exported with the signatures _lib declares, each
rejects a null handle before it touches a device, and the engine wraps them."""

import ctypes as C

import pytest

from lasp_amd import _lib

NAMES = ("laspj_map_create", "laspj_map_destroy", "laspj_map_run", "laspj_map_args",
         "laspj_map_results")


@pytest.fixture(scope="module")
def lib():
    from lasp_amd import build
    build.build()
    return _lib.load()


def test_entry_points_are_exported(lib):
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name


def test_entry_points_reject_null_handles(lib):
    st, verd, pend, cnt = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32()
    out, olen = C.c_void_p(), C.c_uint64()
    h = C.c_void_p()
    img = b"\x83j"
    assert lib.laspj_map_create(None, None, C.byref(h)) == _lib.E_INVAL and not h
    assert lib.laspj_map_destroy(None) == _lib.E_INVAL
    assert lib.laspj_map_run(None, C.byref(st), C.byref(pend), C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_map_args(None, C.byref(out), C.byref(olen), C.byref(cnt),
                              C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_map_results(None, img, 2, C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_abi_version() == 2           # additive: the version stands


def test_engine_wraps_the_process():
    from lasp_amd import engine
    for name in ("run", "args", "results", "step", "close"):
        assert callable(getattr(engine.NifMap, name)), name
    assert callable(engine.Context.map)

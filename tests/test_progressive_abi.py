"""Progressive rendering, the part of its C ABI that needs no GPU (include/rt.h
rt_render_rows_accumulate / rt_accum_resolve): the symbols are exported and bound, the null-context
argument checks answer before anything touches a device, and the ABI version did not move."""
import ctypes as C

import rtzig
from rtzig.abi import RtCamera
from rtzig.lib import EXPORTED

RT_ERR_INVALID = -1


def test_symbols_exported_and_bound():
    lib = rtzig.load()
    for name in ("rt_render_rows_accumulate", "rt_accum_resolve"):
        assert name in EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None
    assert len(lib.rt_render_rows_accumulate.argtypes) == 10
    assert len(lib.rt_accum_resolve.argtypes) == 7


def test_accumulate_null_context_is_invalid():
    lib = rtzig.load()
    cam = RtCamera()
    buf = (C.c_double * 3)()
    rc = lib.rt_render_rows_accumulate(None, C.byref(cam), 0, 1, 1, 0, 1, C.cast(buf, C.c_void_p), None, None)
    assert rc == RT_ERR_INVALID
    assert b"context" in lib.rt_last_error()


def test_resolve_null_context_is_invalid():
    lib = rtzig.load()
    a, o = (C.c_double * 3)(), (C.c_double * 3)()
    rc = lib.rt_accum_resolve(None, C.cast(a, C.c_void_p), 1, 1, 0, C.cast(o, C.c_void_p), None)
    assert rc == RT_ERR_INVALID
    assert b"context" in lib.rt_last_error()


def test_abi_version_unchanged():
    assert rtzig.load().rt_abi_version() == 3

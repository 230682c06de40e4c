"""Progressive rendering, the part of its C ABI that needs no GPU (include/rt.h
rt_render_rows_accumulate / rt_accum_resolve): the symbols are exported and bound, the null-context
argument checks answer before anything touches a device, and the ABI version did not move."""
import ctypes as C

import rtzig
from abi_support import assert_bound, assert_invalid, vp
from rtzig.abi import RtCamera


def test_symbols_exported_and_bound():
    assert_bound("rt_render_rows_accumulate", 10)
    assert_bound("rt_accum_resolve", 7)


def test_accumulate_null_context_is_invalid():
    lib = rtzig.load()
    cam = RtCamera()
    buf = (C.c_double * 3)()
    rc = lib.rt_render_rows_accumulate(None, C.byref(cam), 0, 1, 1, 0, 1, vp(buf), None, None)
    assert_invalid(rc, b"context")


def test_resolve_null_context_is_invalid():
    lib = rtzig.load()
    a, o = (C.c_double * 3)(), (C.c_double * 3)()
    rc = lib.rt_accum_resolve(None, vp(a), 1, 1, 0, vp(o), None)
    assert_invalid(rc, b"context")


def test_abi_version_unchanged():
    assert rtzig.load().rt_abi_version() == 3

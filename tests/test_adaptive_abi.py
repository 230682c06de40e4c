"""Adaptive sampling, the part that needs no GPU (include/rt.h rt_render_pixels_accumulate /
rt_accum_select / rt_accum_resolve_counts): the symbols are exported and bound, every
argument check that can answer without a device does, the ABI version did not move, the six gather
kernels exist within their register budget (checked at build time, as tests/test_kernel_resources.py
does for the kernels they are twins of), and render_adaptive validates its arguments on the host."""
import ctypes as C
import re

import pytest

import rtzig
from abi_support import assert_bound, assert_invalid, cam_of, resources, vp

NAN = float("nan")


def test_symbols_exported_and_bound():
    for name, n_args in (("rt_render_pixels_accumulate", 10), ("rt_accum_select", 13), ("rt_accum_resolve_counts", 7)):
        assert_bound(name, n_args)
    for name in ("render_adaptive",):
        assert name in rtzig.__all__ and callable(getattr(rtzig, name))
    for name in ("accumulate_pixels", "select", "resolve_counts"):
        assert callable(getattr(rtzig.DeviceRenderer, name))
    assert callable(rtzig.Camera.render_adaptive)


def test_abi_version_unchanged():
    assert rtzig.load().rt_abi_version() == 3


# ---- rt_render_pixels_accumulate -------------------------------------------------------------------
def pixels_call(ctx=None, cam="ok", pixels=None, n_pixels=12, count=1, accum="ok", counts="ok"):
    lib = rtzig.load()
    a = (C.c_double * 36)()
    c = (C.c_uint32 * 12)()
    camera = cam_of() if cam == "ok" else cam
    return lib.rt_render_pixels_accumulate(ctx, C.byref(camera) if camera is not None else None, pixels, n_pixels, count,
                                           vp(a) if accum == "ok" else None, None, vp(c) if counts == "ok" else None,
                                           None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(), b"context"),                                    # everything else valid: the null context answers
    (dict(cam=None), b"camera"),
    (dict(accum=None), b"accumulator"),
    (dict(counts=None), b"counts"),
    (dict(n_pixels=11), b"null pixel list"),                 # NULL list, n_pixels != W*H
    (dict(n_pixels=0), b"null pixel list"),
    (dict(pixels=C.c_void_p(64), n_pixels=13), b"exceeds"),  # n_pixels > W*H (the list is never read)
    (dict(cam=cam_of(0, 3)), b"image_width"),
], ids=["ctx", "cam", "accum", "counts", "null-list-short", "null-list-empty", "too-many", "empty-image"])
def test_pixels_accumulate_invalid_arguments(kw, word):
    assert_invalid(pixels_call(**kw), word)


# ---- rt_accum_select -------------------------------------------------------------------------------
def select_call(ctx=None, null=None, n=4, min_count=2, max_count=8, tolerance=0.1, floor=0.01):
    lib = rtzig.load()
    bufs = dict(accum=(C.c_double * 12)(), m2=(C.c_double * 4)(), counts=(C.c_uint32 * 4)(), lst=(C.c_uint32 * 4)(),
                n=(C.c_uint32 * 1)())
    p = {k: (None if k == null else vp(v)) for k, v in bufs.items()}
    return lib.rt_accum_select(ctx, p["accum"], p["m2"], p["counts"], n, min_count, max_count, tolerance, floor,
                               p["lst"], p["n"], None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(), b"context"),
    (dict(null="accum"), b"null"), (dict(null="m2"), b"null"), (dict(null="counts"), b"null"),
    (dict(null="lst"), b"null"), (dict(null="n"), b"null"),
    (dict(min_count=1), b"min_count"), (dict(min_count=0), b"min_count"),
    (dict(min_count=9), b"max_count"),
    (dict(n=2 ** 32), b"2^32"),
    (dict(floor=0.0), b"floor"), (dict(floor=-1.0), b"floor"), (dict(floor=NAN), b"floor"),
    (dict(tolerance=NAN), b"tolerance"),
], ids=["ctx", "accum", "m2", "counts", "list", "n", "min1", "min0", "max<min", "n>=2^32", "floor0", "floor<0",
        "floor-nan", "tol-nan"])
def test_select_invalid_arguments(kw, word):
    assert_invalid(select_call(**kw), word)


# ---- rt_accum_resolve_counts -----------------------------------------------------------------------
def test_resolve_counts_null_context_is_invalid():
    lib = rtzig.load()
    a, o, c = (C.c_double * 3)(), (C.c_double * 3)(), (C.c_uint32 * 1)()
    assert_invalid(lib.rt_accum_resolve_counts(None, vp(a), vp(c), 1, 0, vp(o), None), b"context")


# ---- render_adaptive's host-side argument checks ---------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(min_spp=1), dict(min_spp=0), dict(max_spp=7), dict(step=0), dict(step=-3), dict(tolerance=NAN),
    dict(tolerance=-0.1), dict(floor=0.0), dict(floor=NAN), dict(output="png"), dict(max_spp=2 ** 32),
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_render_adaptive_rejects_bad_arguments_before_any_device_work(kw):
    args = dict(min_spp=8, max_spp=64, step=8, tolerance=0.05)
    args.update(kw)
    with pytest.raises(ValueError):
        rtzig.render_adaptive(cam_of(), [], **args)  # an empty scene: never reached


# ---- the gather kernels' register budget (build time) ----------------------------------------------
def test_six_gather_kernels_no_scratch_lds_tree_ones_at_four_waves():
    rows = resources("rt_kernel.hip")
    gather = {k: v for k, v in rows.items() if re.search(r"gather_kernel(_bvh|_fast)?I", k)}
    # the list walk (lds, smem), the BVH walk and the fast walk (LDS tree, global-memory tree)
    assert len(gather) == 6, sorted(gather)
    assert len([k for k in gather if "gather_kernelI" in k]) == 2
    assert not any("sample_kernel" in k for k in gather)
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in gather.values()), gather
    lds_tree = {k: v for k, v in gather.items() if re.search(r"gather_kernel_(bvh|fast)ILb1E", k)}
    assert len(lds_tree) == 2
    assert all(v["Occupancy [waves/SIMD]"] == 4 and v["VGPRs"] <= 128 for v in lds_tree.values()), lds_tree

"""Feature buffers, the part that needs no GPU (include/rt.h rt_render_rows_features):
the symbol is exported and bound, the ABI version did not move, every argument check that can answer
without a device does, the Python entry points exist with their signatures, and the twelve feature
kernels exist, outside the sample kernels' count, without scratch memory (checked at build time, as
tests/test_kernel_resources.py does for the sample kernels)."""
import ctypes as C
import inspect
import os
import re

import pytest

import rtzig
from abi_support import ROOT, assert_bound, assert_invalid, cam_of, resources, vp


def test_symbol_exported_and_bound():
    assert_bound("rt_render_rows_features", 12)
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        assert re.search(r"\bint rt_render_rows_features\(", f.read())


def test_abi_version_unchanged():
    assert rtzig.load().rt_abi_version() == 3


def features_call(ctx=None, cam="ok", row0=0, row_step=1, n_rows=3, begin=0, count=1):
    lib = rtzig.load()
    a, n, d, h = (C.c_double * 36)(), (C.c_double * 36)(), (C.c_double * 12)(), (C.c_uint32 * 12)()
    camera = cam_of() if cam == "ok" else cam
    return lib.rt_render_rows_features(ctx, C.byref(camera) if camera is not None else None, row0, row_step, n_rows,
                                       begin, count, vp(a), vp(n), vp(d), vp(h), None)


@pytest.mark.parametrize("kw, word", [
    (dict(), b"context"),                                   # everything else valid: the null context answers
    (dict(count=0), b"context"),                            # an empty call still needs a context
    (dict(n_rows=0), b"context"),
    (dict(cam=None), b"camera"),
    (dict(n_rows=4), b"row range"),                         # rows 0..3 of a 3-row image
    (dict(row0=3, n_rows=1), b"row range"),
    (dict(row0=1, row_step=2, n_rows=2), b"row range"),     # rows 1, 3
    (dict(begin=2 ** 32 - 1, count=1), b"2^32"),
    (dict(begin=1, count=2 ** 32 - 1), b"2^32"),
    (dict(cam=cam_of(0, 3)), b"image_width"),
], ids=["ctx", "ctx-empty-samples", "ctx-empty-rows", "cam", "rows-past", "row0-past", "stride-past", "range-end",
        "range-count", "empty-image"])
def test_invalid_arguments_answer_without_a_device(kw, word):
    assert_invalid(features_call(**kw), word)


def test_largest_sample_range_passes_the_range_check():
    """sample_begin + sample_count == 2^32 - 1 is allowed: the null context answers instead."""
    assert_invalid(features_call(begin=2 ** 32 - 2, count=1), b"context")


def test_python_entry_points_and_signatures():
    assert "render_features" in rtzig.__all__ and callable(rtzig.render_features)
    assert list(inspect.signature(rtzig.render_features).parameters) == ["cam", "spheres", "spp", "device"]
    assert inspect.signature(rtzig.render_features).parameters["device"].default == 0
    assert list(inspect.signature(rtzig.Camera.render_features).parameters) == ["self", "spp", "device"]
    sig = inspect.signature(rtzig.DeviceRenderer.features)
    assert list(sig.parameters) == ["self", "cam", "sample_begin", "sample_count", "d_albedo_ptr", "d_normal_ptr",
                                    "d_depth_ptr", "d_hits_ptr", "row0", "row_step", "n_rows", "stream_ptr"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(d_albedo_ptr=None, d_normal_ptr=None, d_depth_ptr=None, d_hits_ptr=None, row0=0,
                            row_step=1, n_rows=None, stream_ptr=None)


@pytest.mark.parametrize("spp", [0, -1, 2 ** 32])
def test_render_features_rejects_bad_sample_counts_before_any_device_work(spp):
    with pytest.raises(ValueError):
        rtzig.render_features(cam_of(), [], spp)  # an empty scene: never reached


# ---- the feature kernels' register budget (build time) ---------------------------------------------
def test_twelve_feature_kernels_no_scratch_bvh_ones_fit_a_1024_thread_block():
    rows = resources("rt_kernel.hip")
    feat = {k: v for k, v in rows.items() if re.search(r"feature_kernel(_bvh)?I", k)}
    # the list walk (lds, smem) and the BVH walk (LDS tree, global-memory tree), each with 1, 4 and 16
    # lanes per pixel
    assert len(feat) == 12, sorted(feat)
    assert len([k for k in feat if "feature_kernelI" in k]) == 6
    assert not any("sample_kernel" in k for k in feat)
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in feat.values()), feat
    bvh = {k: v for k, v in feat.items() if "feature_kernel_bvhI" in k}
    assert len(bvh) == 6
    assert all(v["Occupancy [waves/SIMD]"] >= 4 and v["VGPRs"] <= 128 for v in bvh.values()), bvh

"""Occlusion queries, the part that needs no GPU (include/rt.h rt_occluded_rays): the
symbol is exported, bound and declared, the ABI version did not move, every argument check that can
answer without a device does and names its argument, the Python entry points exist with their
signatures, and the four occlusion kernels exist outside the other families' counts, without scratch
memory and within the trace kernels' registers (checked at build time)."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

import rtzig
from abi_support import ROOT, assert_bound, assert_invalid, resources, vp
from rtzig import abi


def test_symbol_exported_bound_and_declared():
    assert_bound("rt_occluded_rays", 13)
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        text = f.read()
    m = re.search(r"\bint rt_occluded_rays\(([^;]*)\);", text)
    assert m and len(m.group(1).split(",")) == 13
    assert re.search(r"#define RT_OCCLUSION_TARGETS 1u\b", text)
    assert abi.OCCLUSION_TARGETS == 1 == rtzig.OCCLUSION_TARGETS


def test_abi_version_did_not_move():
    assert rtzig.load().rt_abi_version() == 3
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        assert re.search(r"#define RT_ABI_VERSION 3\b", f.read())


def occluded_call(ctx=None, origins="ok", ends="ok", stride=3, n=4, flags=0):
    lib = rtzig.load()
    o, e = (C.c_double * 16)(), (C.c_double * 16)()
    return lib.rt_occluded_rays(ctx, vp(o) if origins == "ok" else None, vp(e) if ends == "ok" else None, stride, n,
                                1e-3, math.inf, None, flags, None, None, None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(), b"context"),                      # everything else valid: the null context answers, last
    (dict(n=0), b"context"),                   # an empty call still needs a context
    (dict(stride=0), b"context"),              # 0 means 3
    (dict(stride=4), b"context"),
    (dict(flags=1), b"context"),               # RT_OCCLUSION_TARGETS
    (dict(n=2 ** 32 - 1), b"context"),         # the largest count passes the count check
    (dict(origins=None), b"d_origins"),
    (dict(ends=None), b"d_ends"),
    (dict(stride=1), b"ray_stride"),
    (dict(stride=2), b"ray_stride"),
    (dict(n=2 ** 32), b"n_rays"),
    (dict(n=2 ** 63), b"n_rays"),
    (dict(flags=2), b"flags"),
    (dict(flags=3), b"flags"),
    (dict(flags=2 ** 31), b"flags"),
], ids=["ctx", "ctx-empty", "ctx-stride0", "ctx-stride4", "ctx-targets", "ctx-n-2^32-1", "origins", "ends", "stride1",
        "stride2", "n-2^32", "n-2^63", "flags2", "flags3", "flags-2^31"])
def test_invalid_arguments_answer_without_a_device(kw, word):
    assert_invalid(occluded_call(**kw), word)


def defaults_of(sig):
    return {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}


def test_python_entry_points_and_signatures():
    for name in ("occluded", "OCCLUSION_TARGETS", "Scene", "DeviceRenderer"):
        assert name in rtzig.__all__
    sig = inspect.signature(rtzig.occluded)
    assert list(sig.parameters) == ["spheres", "origins", "ends", "t_min", "t_max", "intervals", "targets", "device"]
    assert defaults_of(sig) == dict(t_min=1e-3, t_max=math.inf, intervals=None, targets=False, device=0)
    sig = inspect.signature(rtzig.Scene.occluded)
    assert list(sig.parameters) == ["self", "origins", "ends", "t_min", "t_max", "intervals", "targets", "device"]
    assert defaults_of(sig) == dict(t_min=1e-3, t_max=math.inf, intervals=None, targets=False, device=0)
    sig = inspect.signature(rtzig.Scene.visible)
    assert list(sig.parameters) == ["self", "a", "b", "eps", "device"]
    assert defaults_of(sig) == dict(eps=1e-3, device=0)
    sig = inspect.signature(rtzig.DeviceRenderer.occluded_rays)
    assert list(sig.parameters) == ["self", "d_origins_ptr", "d_ends_ptr", "n_rays", "t_min", "t_max", "d_occluded_ptr",
                                    "d_mask_ptr", "d_intervals_ptr", "d_stats_ptr", "ray_stride", "targets", "stream_ptr"]
    assert defaults_of(sig) == dict(t_min=1e-3, t_max=math.inf, d_occluded_ptr=None, d_mask_ptr=None,
                                    d_intervals_ptr=None, d_stats_ptr=None, ray_stride=3, targets=False, stream_ptr=None)


def test_bad_shapes_raise_before_any_device_work():
    scene = rtzig.Scene(1)
    for f in (lambda *a, **k: rtzig.occluded([], *a, **k), scene.occluded):
        with pytest.raises(ValueError):
            f([[0, 0, 0]], [[0, 0, 1], [0, 1, 0]])
        with pytest.raises(ValueError):
            f([[0, 0, 0, 0]], [[0, 0, 1, 0]])
        with pytest.raises(ValueError):
            f([0, 0, 0], [0, 0, 1])
        with pytest.raises(ValueError):
            f([[0, 0, 0]], [[0, 0, 1]], intervals=[[0, 1, 2]])
    with pytest.raises(ValueError):
        scene.visible([[0, 0, 0]], [[0, 0, 1], [0, 1, 0]])


# ---- the occlusion kernels' register budget (build time) -------------------------------------------
def test_four_occlusion_kernels_no_scratch_within_the_trace_kernels_registers():
    rows = resources("rt_kernel.hip")
    occ = {k: v for k, v in rows.items() if re.search(r"occlusion_kernel(_bvh)?I", k)}
    # the list walk (lds, smem) and the BVH walk (LDS tree, global-memory tree)
    assert len(occ) == 4, sorted(occ)
    assert len([k for k in occ if "occlusion_kernelI" in k]) == 2
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in occ.values()), occ
    bvh = {k: v for k, v in occ.items() if "occlusion_kernel_bvhI" in k}
    assert len(bvh) == 2
    assert all(v["Occupancy [waves/SIMD]"] >= 4 and v["VGPRs"] <= 128 for v in bvh.values()), bvh
    # the any-hit walk carries less state than the closest-hit walk of the same tree placement
    for placement in ("ILb1E", "ILb0E"):  # LDS tree, global-memory tree
        o = [v for k, v in bvh.items() if "occlusion_kernel_bvh" + placement in k]
        t = [v for k, v in rows.items() if "trace_kernel_bvh" + placement in k]
        assert len(o) == 1 and len(t) == 1
        assert o[0]["VGPRs"] <= t[0]["VGPRs"], (placement, o[0], t[0])
    # the other families' counts did not move
    assert len([k for k in rows if "sample_kernel" in k]) == 24
    assert len([k for k in rows if re.search(r"feature_kernel(_bvh)?I", k)]) == 12
    assert len([k for k in rows if re.search(r"trace_kernel(_bvh)?I", k)]) == 4

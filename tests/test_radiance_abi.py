"""Radiance queries, the part that needs no GPU (include/rt.h rt_radiance_rays): the
symbol is exported, bound and declared, its params struct is 48 bytes on both sides, the ABI version
did not move, every argument check that can answer without a device does and names its argument, the
Python entry points exist with their signatures, and the four radiance kernels exist outside the other
families' counts, without scratch memory and — the BVH forms — at 4 waves per SIMD within 128 VGPRs
(checked at build time)."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import rtzig
from abi_support import ROOT, assert_bound, assert_invalid, resources, vp
from rtzig import abi


def header():
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        return f.read()


def test_symbol_exported_bound_and_declared():
    assert_bound("rt_radiance_rays", 10)
    m = re.search(r"\bint rt_radiance_rays\(([^;]*)\);", header())
    assert m and len(m.group(1).split(",")) == 10


def test_params_struct_is_48_bytes_on_both_sides():
    assert C.sizeof(abi.RtRadianceParams) == 48 == abi.RADIANCE_PARAMS_SIZE
    names = [n for n, _ in abi.RtRadianceParams._fields_]
    assert names == ["seed", "ray_base", "sample_begin", "sample_count", "bounce_max", "reserved", "t_min", "t_max"]
    offs = [getattr(abi.RtRadianceParams, n).offset for n in names]
    assert offs == [0, 8, 16, 20, 24, 28, 32, 40]
    m = re.search(r"typedef struct rt_radiance_params \{(.*?)\} rt_radiance_params;\s*/\* 48 bytes \*/", header(), re.S)
    assert m
    declared = re.findall(r"\b(uint64_t|uint32_t|double)\s+([a-z_, ]+);", m.group(1))
    flat = [(t, n.strip()) for t, ns in declared for n in ns.split(",")]
    assert [n for _, n in flat] == names
    assert sum({"uint64_t": 8, "uint32_t": 4, "double": 8}[t] for t, _ in flat) == 48


def test_abi_version_did_not_move():
    assert rtzig.load().rt_abi_version() == 3
    assert re.search(r"#define RT_ABI_VERSION 3\b", header())


def radiance_call(ctx=None, origins="ok", directions="ok", params="ok", stride=3, n=4, states=None, **fields):
    lib = rtzig.load()
    o, d, st = (C.c_double * 16)(), (C.c_double * 16)(), (C.c_uint64 * 16)()
    prm = abi.RtRadianceParams(seed=1, ray_base=0, sample_begin=0, sample_count=1, bounce_max=50, reserved=0,
                               t_min=1e-3, t_max=math.inf)
    for k, v in fields.items():
        setattr(prm, k, v)
    return lib.rt_radiance_rays(ctx, vp(o) if origins == "ok" else None, vp(d) if directions == "ok" else None, stride,
                                n, C.byref(prm) if params == "ok" else None, vp(st) if states == "ok" else None,
                                None, None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(), b"context"),                                        # everything else valid: the null context answers, last
    (dict(n=0), b"context"),                                     # an empty call still needs a context
    (dict(sample_count=0), b"context"),
    (dict(stride=0), b"context"),                                # 0 means 3
    (dict(stride=4), b"context"),
    (dict(n=2 ** 32), b"context"),                               # ray_base + n_rays == 2^32 passes
    (dict(n=1, ray_base=2 ** 32 - 1), b"context"),
    (dict(sample_begin=2 ** 32 - 2, sample_count=1), b"context"),  # the last sample is 2^32 - 2
    (dict(sample_begin=0, sample_count=2 ** 32 - 1), b"context"),
    (dict(bounce_max=0), b"context"),
    (dict(bounce_max=2 ** 32 - 1), b"context"),                  # any uint32_t
    (dict(states="ok"), b"context"),                             # states with sample_count == 1
    (dict(t_min=-1.0, t_max=math.nan), b"context"),              # any interval is legal
    (dict(origins=None), b"d_origins"),
    (dict(directions=None), b"d_directions"),
    (dict(params=None), b"params"),
    (dict(stride=1), b"ray_stride"),
    (dict(stride=2), b"ray_stride"),
    (dict(reserved=1), b"reserved"),
    (dict(reserved=2 ** 31), b"reserved"),
    (dict(n=2 ** 32 + 1), b"ray_base"),
    (dict(n=2 ** 63), b"ray_base"),
    (dict(n=2, ray_base=2 ** 32 - 1), b"ray_base"),
    (dict(n=0, ray_base=2 ** 32 + 1), b"ray_base"),
    (dict(n=1, ray_base=2 ** 64 - 1), b"ray_base"),              # the sum wraps in 64 bits
    (dict(sample_begin=2 ** 32 - 1, sample_count=1), b"sample_begin"),
    (dict(sample_begin=1, sample_count=2 ** 32 - 1), b"sample_begin"),
    (dict(states="ok", sample_count=2), b"d_states"),
    (dict(states="ok", sample_count=0), b"d_states"),
], ids=["ctx", "ctx-empty", "ctx-no-samples", "ctx-stride0", "ctx-stride4", "ctx-n-2^32", "ctx-last-id", "ctx-last-sample",
        "ctx-all-samples", "ctx-bounce0", "ctx-bounce-max", "ctx-states", "ctx-interval", "origins", "directions", "params",
        "stride1", "stride2", "reserved1", "reserved-2^31", "n-2^32+1", "n-2^63", "base-past", "base-alone", "base-wrap",
        "sample-2^32-1", "samples-past", "states-2", "states-0"])
def test_invalid_arguments_answer_without_a_device(kw, word):
    assert_invalid(radiance_call(**kw), word)


def defaults_of(sig):
    return {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}


def test_python_entry_points_and_signatures():
    for name in ("radiance", "RtRadianceParams", "Scene", "DeviceRenderer"):
        assert name in rtzig.__all__
    sig = inspect.signature(rtzig.radiance)
    assert list(sig.parameters) == ["spheres", "origins", "directions", "samples", "bounce_max", "seed", "ray_base", "t_min",
                                    "t_max", "states", "device"]
    d = defaults_of(sig)
    assert isinstance(d.pop("seed"), int)
    assert d == dict(samples=1, bounce_max=50, ray_base=0, t_min=1e-3, t_max=math.inf, states=None, device=0)
    sig = inspect.signature(rtzig.Scene.radiance)
    assert list(sig.parameters) == ["self", "origins", "directions", "samples", "bounce_max", "ray_base", "t_min", "t_max",
                                    "states", "device"]
    assert defaults_of(sig) == dict(samples=1, bounce_max=50, ray_base=0, t_min=1e-3, t_max=math.inf, states=None, device=0)
    sig = inspect.signature(rtzig.DeviceRenderer.radiance_rays)
    assert list(sig.parameters) == ["self", "d_origins_ptr", "d_directions_ptr", "n_rays", "d_sum_ptr", "sample_begin",
                                    "sample_count", "bounce_max", "seed", "ray_base", "t_min", "t_max", "d_states_ptr",
                                    "d_stats_ptr", "ray_stride", "stream_ptr"]
    d = defaults_of(sig)
    assert isinstance(d.pop("seed"), int)
    assert d == dict(d_sum_ptr=None, sample_begin=0, sample_count=1, bounce_max=50, ray_base=0, t_min=1e-3, t_max=math.inf,
                     d_states_ptr=None, d_stats_ptr=None, ray_stride=3, stream_ptr=None)


def test_bad_shapes_raise_before_any_device_work():
    scene = rtzig.Scene(1)
    for f in (lambda *a, **k: rtzig.radiance([], *a, **k), scene.radiance):
        with pytest.raises(ValueError):
            f([[0, 0, 0]], [[0, 0, 1], [0, 1, 0]])
        with pytest.raises(ValueError):
            f([[0, 0, 0, 0]], [[0, 0, 1, 0]])
        with pytest.raises(ValueError):
            f([0, 0, 0], [0, 0, 1])
        with pytest.raises(ValueError):
            f([[0, 0, 0]], [[0, 0, 1]], states=[[1, 2, 3]])
        with pytest.raises(ValueError):
            f([[0, 0, 0]], [[0, 0, 1]], states=[[1, 2, 3, 4]], samples=2)
        with pytest.raises(ValueError):
            f([[0, 0, 0]], [[0, 0, 1]], samples=-1)
        with pytest.raises(ValueError):
            f([[0, 0, 0]], [[0, 0, 1]], bounce_max=2 ** 32)
        with pytest.raises(ValueError):
            f([[0, 0, 0]], [[0, 0, 1]], ray_base=2 ** 32)
        # nothing to do: no device is touched
        assert f([[0, 0, 0]], [[0, 0, 1]], samples=0).shape == (1, 3)
        assert f(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 3)


# ---- the radiance kernels' build-time resources ------------------------------------------------------
def test_four_radiance_kernels_no_scratch_bvh_forms_at_four_waves():
    rows = resources("rt_kernel.hip")
    rad = {k: v for k, v in rows.items() if re.search(r"radiance_kernel(_bvh)?I", k)}
    # the list walk (lds, smem) and the BVH walk (LDS tree, global-memory tree)
    assert len(rad) == 4, sorted(rad)
    assert len([k for k in rad if "radiance_kernelI" in k]) == 2
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in rad.values()), rad
    bvh = {k: v for k, v in rad.items() if "radiance_kernel_bvhI" in k}
    assert len(bvh) == 2
    assert all(v["Occupancy [waves/SIMD]"] >= 4 and v["VGPRs"] <= 128 for v in bvh.values()), bvh
    # the other families' counts did not move
    assert len([k for k in rows if "sample_kernel" in k]) == 24
    assert len([k for k in rows if re.search(r"feature_kernel(_bvh)?I", k)]) == 12
    assert len([k for k in rows if re.search(r"trace_kernel(_bvh)?I", k)]) == 4
    assert len([k for k in rows if re.search(r"occlusion_kernel(_bvh)?I", k)]) == 4

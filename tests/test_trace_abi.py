"""Ray queries, the part that needs no GPU (include/rt.h rt_trace_rays): the three
symbols are exported, bound and declared, rt_ray_hits has its size, the ABI version did not move, every
argument check that can answer without a device does and names its argument, the Python entry points
exist with their signatures, and the four trace kernels exist outside the sample and feature kernels'
counts, without scratch memory (checked at build time, as tests/test_kernel_resources.py does)."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

import rtzig
from abi_support import ROOT, assert_bound, assert_invalid, resources, vp
from rtzig import abi


@pytest.mark.parametrize("name, n_args", [("rt_trace_rays", 11), ("rt_context_origin_bound", 2),
                                          ("rt_context_reserve_origin_bound", 2)])
def test_symbols_exported_bound_and_declared(name, n_args):
    assert_bound(name, n_args)
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, f.read())
    assert m and len(m.group(1).split(",")) == n_args


def test_ray_hits_struct_size_and_abi_version():
    assert C.sizeof(abi.RtRayHits) == 40 == abi.RAY_HITS_SIZE
    assert [f[0] for f in abi.RtRayHits._fields_] == ["index", "t", "point", "normal", "front"]
    assert rtzig.load().rt_abi_version() == 3
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        assert re.search(r"#define RT_ABI_VERSION 3\b", f.read())


def trace_call(ctx=None, origins="ok", directions="ok", out="ok", stride=3, n=4):
    lib = rtzig.load()
    o, d = (C.c_double * 16)(), (C.c_double * 16)()
    hits = abi.RtRayHits()
    return lib.rt_trace_rays(ctx, vp(o) if origins == "ok" else None,
                             vp(d) if directions == "ok" else None, stride, n, 1e-3, math.inf, None,
                             C.byref(hits) if out == "ok" else None, None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(), b"context"),                      # everything else valid: the null context answers, last
    (dict(n=0), b"context"),                   # an empty call still needs a context
    (dict(stride=0), b"context"),              # 0 means 3
    (dict(stride=4), b"context"),
    (dict(origins=None), b"d_origins"),
    (dict(directions=None), b"d_directions"),
    (dict(out=None), b"out"),
    (dict(stride=1), b"ray_stride"),
    (dict(stride=2), b"ray_stride"),
    (dict(n=2 ** 32), b"n_rays"),
    (dict(n=2 ** 63), b"n_rays"),
], ids=["ctx", "ctx-empty", "ctx-stride0", "ctx-stride4", "origins", "directions", "out", "stride1", "stride2",
        "n-2^32", "n-2^63"])
def test_invalid_arguments_answer_without_a_device(kw, word):
    assert_invalid(trace_call(**kw), word)


def test_largest_ray_count_passes_the_count_check():
    assert_invalid(trace_call(n=2 ** 32 - 1), b"context")


@pytest.mark.parametrize("bound", [0.0, -1.0, math.inf, -math.inf, math.nan, 1.79e308])  # the last: x 1.01 overflows
def test_reserve_origin_bound_rejects_bad_bounds_before_the_context(bound):
    lib = rtzig.load()
    assert_invalid(lib.rt_context_reserve_origin_bound(None, bound), b"bound")


def test_bound_calls_reject_a_null_context():
    lib = rtzig.load()
    assert_invalid(lib.rt_context_reserve_origin_bound(None, 10.0), b"context")
    b = C.c_double()
    assert_invalid(lib.rt_context_origin_bound(None, C.byref(b)), b"context")


def test_python_entry_points_and_signatures():
    assert "trace_rays" in rtzig.__all__ and callable(rtzig.trace_rays)
    assert "RtRayHits" in rtzig.__all__ and "Scene" in rtzig.__all__
    sig = inspect.signature(rtzig.trace_rays)
    assert list(sig.parameters) == ["spheres", "origins", "directions", "t_min", "t_max", "intervals", "device"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(t_min=1e-3, t_max=math.inf, intervals=None, device=0)
    sig = inspect.signature(rtzig.Scene.hit)
    assert list(sig.parameters) == ["self", "origins", "directions", "t_min", "t_max", "intervals", "device"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(t_min=1e-3, t_max=math.inf, intervals=None, device=0)
    sig = inspect.signature(rtzig.DeviceRenderer.trace_rays)
    assert list(sig.parameters) == ["self", "d_origins_ptr", "d_directions_ptr", "n_rays", "t_min", "t_max",
                                    "d_index_ptr", "d_t_ptr", "d_point_ptr", "d_normal_ptr", "d_front_ptr",
                                    "d_intervals_ptr", "d_stats_ptr", "ray_stride", "stream_ptr"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(t_min=1e-3, t_max=math.inf, d_index_ptr=None, d_t_ptr=None, d_point_ptr=None,
                            d_normal_ptr=None, d_front_ptr=None, d_intervals_ptr=None, d_stats_ptr=None,
                            ray_stride=3, stream_ptr=None)
    assert list(inspect.signature(rtzig.DeviceRenderer.origin_bound).parameters) == ["self"]
    assert list(inspect.signature(rtzig.DeviceRenderer.reserve_origin_bound).parameters) == ["self", "bound"]


def test_trace_rays_rejects_bad_shapes_before_any_device_work():
    with pytest.raises(ValueError):
        rtzig.trace_rays([], [[0, 0, 0]], [[0, 0, 1], [0, 1, 0]])
    with pytest.raises(ValueError):
        rtzig.trace_rays([], [[0, 0, 0, 0]], [[0, 0, 1, 0]])
    with pytest.raises(ValueError):
        rtzig.trace_rays([], [[0, 0, 0]], [[0, 0, 1]], intervals=[[0, 1, 2]])


# ---- the trace kernels' register budget (build time) -----------------------------------------------
def test_four_trace_kernels_no_scratch_bvh_ones_fit_a_1024_thread_block():
    rows = resources("rt_kernel.hip")
    trace = {k: v for k, v in rows.items() if re.search(r"trace_kernel(_bvh)?I", k)}
    # the list walk (lds, smem) and the BVH walk (LDS tree, global-memory tree)
    assert len(trace) == 4, sorted(trace)
    assert len([k for k in trace if "trace_kernelI" in k]) == 2
    assert not any(w in k for k in trace for w in ("sample_kernel", "feature_kernel", "gather_kernel"))
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in trace.values()), trace
    bvh = {k: v for k, v in trace.items() if "trace_kernel_bvhI" in k}
    assert len(bvh) == 2
    assert all(v["Occupancy [waves/SIMD]"] >= 4 and v["VGPRs"] <= 128 for v in bvh.values()), bvh
    # the other families' counts did not move
    assert len([k for k in rows if "sample_kernel" in k]) == 24
    assert len([k for k in rows if re.search(r"feature_kernel(_bvh)?I", k)]) == 12

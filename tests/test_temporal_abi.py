"""The temporal accumulation, the part that needs no GPU (include/rt.h rt_temporal_accumulate, DESIGN.md
§5.11): both symbols are exported and bound, the ABI version did not move, the structs have their sizes
and the defaults are the documented ones, every argument check answers without a device and names what it
refused, the Python entry points exist with their signatures, the kernel exists alone in its translation
unit and without scratch memory (checked at build time, as tests/test_denoise_abi.py does), and the numpy
reference passes two sanity pins of its own."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import rtzig
import temporal_ref
from abi_support import RT_ERR_INVALID, ROOT, assert_bound, assert_invalid, cam_of, resources
from rtzig.abi import RtTemporalFrame, RtTemporalParams

DEFAULTS = dict(max_history=64, reserved=0, sigma_z=0.05, tau_n=0.1, tau_a=0.05, tau_h=0.5, min_weight=0.25)


def test_symbols_exported_bound_and_declared():
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        header = f.read()
    for name, nargs in (("rt_temporal_accumulate", 8), ("rt_temporal_default_params", 1)):
        assert_bound(name, nargs)
        assert re.search(r"\bint %s\(" % name, header)
    assert "typedef struct rt_temporal_frame" in header and "typedef struct rt_temporal_params" in header
    assert "Only the first frame" in header  # the header says what is bit-identical to a one-pass render


def test_abi_version_unchanged():
    assert rtzig.load().rt_abi_version() == 3
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        assert "#define RT_ABI_VERSION 3\n" in f.read()


def test_struct_sizes_and_default_params():
    assert C.sizeof(RtTemporalFrame) == rtzig.abi.TEMPORAL_FRAME_SIZE == 64
    assert C.sizeof(RtTemporalParams) == rtzig.abi.TEMPORAL_PARAMS_SIZE == 48
    p = RtTemporalParams()
    assert rtzig.load().rt_temporal_default_params(C.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in RtTemporalParams._fields_} == DEFAULTS
    assert rtzig.load().rt_temporal_default_params(None) == RT_ERR_INVALID
    q = rtzig.temporal_params()
    assert {k: getattr(q, k) for k, _ in RtTemporalParams._fields_} == DEFAULTS
    q = rtzig.temporal_params(max_history=16, sigma_z=0.02)
    assert (q.max_history, q.sigma_z, q.tau_n) == (16, 0.02, 0.1)
    with pytest.raises(TypeError):
        rtzig.temporal_params(sigma=1.0)
    assert {k: v for k, v in DEFAULTS.items() if k != "reserved"} == temporal_ref.DEFAULTS


def _frame(base, **over):
    """rt_temporal_frame of made-up non-null pointers (never dereferenced: a null context answers last)."""
    f = dict(accum=1, m2=2, counts=3, albedo=4, normal=5, depth=6, hits=7)
    f.update({k: v for k, v in over.items() if k in f})
    fr = RtTemporalFrame(**{k: (base + v) * 4096 if v else None for k, v in f.items()})
    fr.feature_samples = over.get("feature_samples", 4)
    fr.reserved = over.get("reserved", 0)
    return fr


def temporal_call(ctx=None, cam="ok", cam_prev="ok", cur=None, prev=None, params=None, null=(), history=1):
    lib = rtzig.load()
    a = dict(cam=cam_of() if cam == "ok" else cam, cam_prev=cam_of() if cam_prev == "ok" else cam_prev,
             cur=_frame(0, **(cur or {})), prev=_frame(16, **(prev or {})))
    ref = {k: (None if k in null else C.byref(v)) for k, v in a.items()}
    return lib.rt_temporal_accumulate(ctx, ref["cam"], ref["cur"], ref["cam_prev"], ref["prev"],
                                      C.byref(params) if params is not None else None,
                                      C.c_void_p(history * 4096 * 64), None)


def _cam_with(**kw):
    cam = cam_of(kw.pop("w", 4), kw.pop("h", 3))
    for name, v in kw.items():
        for k in range(3):
            getattr(cam, name)[k] = v[k]
    return cam


INF, NAN = float("inf"), float("nan")
CASES = {
    "ctx": (dict(), b"context"),  # everything else valid: the null context answers
    "ctx-no-guides": (dict(cur=dict(albedo=0, normal=0), prev=dict(albedo=0, normal=0), history=0), b"context"),
    "cam": (dict(null=("cam",)), b"camera"),
    "cam_prev": (dict(null=("cam_prev",)), b"previous camera"),
    "cur": (dict(null=("cur",)), b"current frame"),
    "prev": (dict(null=("prev",)), b"previous frame"),
    "cur-accum": (dict(cur=dict(accum=0)), b"accumulator"),
    "cur-m2": (dict(cur=dict(m2=0)), b"m2"),
    "cur-counts": (dict(cur=dict(counts=0)), b"counts"),
    "cur-depth": (dict(cur=dict(depth=0)), b"depth"),
    "cur-hits": (dict(cur=dict(hits=0)), b"hits"),
    "prev-accum": (dict(prev=dict(accum=0)), b"accumulator"),
    "prev-m2": (dict(prev=dict(m2=0)), b"m2"),
    "prev-counts": (dict(prev=dict(counts=0)), b"counts"),
    "prev-depth": (dict(prev=dict(depth=0)), b"depth"),
    "prev-hits": (dict(prev=dict(hits=0)), b"hits"),
    "albedo-cur-only": (dict(prev=dict(albedo=0)), b"albedo"),
    "albedo-prev-only": (dict(cur=dict(albedo=0)), b"albedo"),
    "normal-cur-only": (dict(prev=dict(normal=0)), b"normal"),
    "normal-prev-only": (dict(cur=dict(normal=0)), b"normal"),
    "cur-feature-samples": (dict(cur=dict(feature_samples=0)), b"feature_samples"),
    "prev-feature-samples": (dict(prev=dict(feature_samples=0)), b"feature_samples"),
    "cur-reserved": (dict(cur=dict(reserved=1)), b"reserved"),
    "prev-reserved": (dict(prev=dict(reserved=7)), b"reserved"),
    "sizes-differ-w": (dict(cam_prev=_cam_with(w=5)), b"image sizes"),
    "sizes-differ-h": (dict(cam=_cam_with(h=2)), b"image sizes"),
    "width-0": (dict(cam=_cam_with(w=0), cam_prev=_cam_with(w=0)), b"width"),
    "height-0": (dict(cam=_cam_with(h=0), cam_prev=_cam_with(h=0)), b"height"),
    "too-many-pixels": (dict(cam=_cam_with(w=65536, h=65536), cam_prev=_cam_with(w=65536, h=65536)), b"2^32"),
    "params-reserved": (dict(params=dict(reserved=1)), b"reserved"),
    "max_history-0": (dict(params=dict(max_history=0)), b"max_history"),
    "max_history-big": (dict(params=dict(max_history=2 ** 24 + 1)), b"max_history"),
    "sigma_z-negative": (dict(params=dict(sigma_z=-1e-300)), b"sigma_z"),
    "tau_n-nan": (dict(params=dict(tau_n=NAN)), b"tau_n"),
    "tau_a-negative": (dict(params=dict(tau_a=-0.5)), b"tau_a"),
    "tau_h-nan": (dict(params=dict(tau_h=NAN)), b"tau_h"),
    "min_weight-0": (dict(params=dict(min_weight=0.0)), b"min_weight"),
    "min_weight-above-1": (dict(params=dict(min_weight=1.0000001)), b"min_weight"),
    "min_weight-nan": (dict(params=dict(min_weight=NAN)), b"min_weight"),
    "nn-zero": (dict(cam_prev=_cam_with(dv=(0.25, 0.0, 0.0))), b"nn"),
    "nn-infinite": (dict(cam_prev=_cam_with(du=(1e160, 0.0, 0.0), dv=(0.0, 1e160, 0.0))), b"nn"),
    "nn-nan": (dict(cam_prev=_cam_with(du=(NAN, 0.0, 0.0))), b"nn"),
    "an-zero": (dict(cam_prev=_cam_with(pixel0=(-0.5, 0.5, 0.0))), b"an must not be 0"),
    "shared-accum": (dict(prev=dict(accum=1 - 16)), b"share"),       # prev.accum == cur.accum
    "shared-cross": (dict(prev=dict(depth=2 - 16)), b"share"),       # prev.depth == cur.m2
    "shared-guide": (dict(prev=dict(normal=5 - 16)), b"share"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_invalid_arguments_answer_without_a_device(name):
    kw, word = CASES[name]
    kw = dict(kw)
    if "params" in kw:
        kw["params"] = rtzig.temporal_params(**kw["params"])
    assert_invalid(temporal_call(**kw), word)


def test_limits_that_pass_the_checks():
    """max_history 1 and 2^24, zero tolerances, min_weight 1 and 2^32 - 65536 pixels are allowed: the null
    context answers instead."""
    big = dict(cam=_cam_with(w=65535, h=65536), cam_prev=_cam_with(w=65535, h=65536))
    for kw in (dict(params=rtzig.temporal_params(max_history=1)), dict(params=rtzig.temporal_params(max_history=2 ** 24)),
               dict(params=rtzig.temporal_params(sigma_z=0.0, tau_n=0.0, tau_a=0.0, tau_h=0.0)),
               dict(params=rtzig.temporal_params(min_weight=1.0)), big):
        assert_invalid(temporal_call(**kw), b"context")


def test_python_entry_points_and_signatures():
    for name in ("render_sequence", "temporal_params", "RtTemporalFrame", "RtTemporalParams"):
        assert name in rtzig.__all__ and hasattr(rtzig, name)
    sig = inspect.signature(rtzig.render_sequence)
    assert list(sig.parameters) == ["cams", "spheres", "spp", "feature_spp", "temporal", "denoise", "seed_step",
                                    "device", "output", "precision"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(feature_spp=4, temporal=None, denoise=None, seed_step=1, device=0, output="linear",
                            precision="f64")
    sig = inspect.signature(rtzig.DeviceRenderer.temporal_accumulate)
    assert list(sig.parameters) == ["self", "cam", "cur", "cam_prev", "prev", "params", "d_history_ptr", "stream_ptr"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(params=None, d_history_ptr=None, stream_ptr=None)
    # the entry point it stands next to did not move
    assert list(inspect.signature(rtzig.render_denoised).parameters) == [
        "cam", "spheres", "spp", "feature_spp", "params", "adaptive", "device", "output", "precision"]


@pytest.mark.parametrize("kw", [dict(spp=1), dict(spp=0), dict(spp=2 ** 32), dict(spp=4, feature_spp=0),
                                dict(spp=4, feature_spp=-1), dict(spp=4, output="hdr"), dict(spp=4, precision="f16"),
                                dict(spp=4, temporal=dict(max_history=4)), dict(spp=4, temporal=rtzig.denoise_params()),
                                dict(spp=4, denoise=rtzig.temporal_params()), dict(spp=4, cams=[]),
                                dict(spp=4, cams=[cam_of(), cam_of(5, 3)]), dict(spp=4, cams=[cam_of(0, 3)]),
                                dict(spp=4, cams=["camera"])])
def test_render_sequence_rejects_bad_arguments_before_any_device_work(kw):
    kw = dict(kw)
    cams = kw.pop("cams", [cam_of(), cam_of()])
    with pytest.raises(ValueError):
        rtzig.render_sequence(cams, [], **kw)  # at the call, not at the first next(); an empty scene: never reached


# ---- the kernel's resources (build time) ---------------------------------------------------------------
def test_one_temporal_kernel_without_scratch_or_lds():
    rows = resources("rt_temporal.hip")
    assert len(rows) == 1 and "temporal_accumulate_kernel" in next(iter(rows)), sorted(rows)
    v = next(iter(rows.values()))
    assert v["ScratchSize [bytes/lane]"] == 0 and v["LDS Size [bytes/block]"] == 0, v
    assert v["Occupancy [waves/SIMD]"] >= 4, v  # a memory-bound pass: enough waves to cover the loads
    # the other translation units did not take it in
    with open(os.path.join(ROOT, "raytracing-with-zig_amd", "csrc", "Makefile")) as f:
        assert "build/rt_temporal.o" in f.read()


# ---- the reference's own sanity pins -------------------------------------------------------------------
def _smooth(W, H, counts, fs=4):
    P = W * H
    j, i = np.divmod(np.arange(P), W)
    c = np.asarray(counts, np.int64)
    accum = np.stack([0.2 + 0.1 * i, 0.3 + 0.1 * j, 0.5 + 0.0 * i], 1) * c[:, None]
    S = (accum[:, 0] + accum[:, 1]) + accum[:, 2]
    hits = np.array([fs] * (P - 1) + [0])  # the last pixel sees the sky
    h = hits.astype(np.float64)
    return dict(accum=accum, m2=S * (S / np.maximum(c, 1)) * 1.5, counts=c, albedo=np.full((P, 3), 0.5) * h[:, None],
                normal=np.tile([0.0, 0.0, 1.0], (P, 1)) * h[:, None], depth=(2.0 + 0.01 * i) * h, hits=hits,
                feature_samples=fs)


def test_reference_identical_cameras_take_min_of_counts_and_cap():
    """A 3 x 2 image, cam_prev == cam, smooth buffers: u and v are the pixel's own coordinates to rounding,
    every tap that carries weight is the pixel itself or (at a weight of some 1e-16) a neighbour that
    passes too — history == min(counts', max_history) at every hit pixel, 0 at the sky pixel — and the
    merged mean is the previous mean."""
    W, H = 3, 2
    cam = cam_of(W, H)
    prev = _smooth(W, H, [24, 24, 24, 24, 24, 24], fs=8)
    cur = _smooth(W, H, [0, 4, 4, 4, 4, 4])
    cur["accum"][0], cur["m2"][0] = np.nan, np.nan  # counts 0: not read
    for cap in (1, 24, 64):
        accum, m2, counts, hist = temporal_ref.accumulate(W, H, cam, cur, cam, prev, max_history=cap)
        want = np.array([min(24, cap)] * 5 + [0])
        assert np.array_equal(hist, want) and np.array_equal(counts, cur["counts"] + want)
        assert np.abs(accum[0] / hist[0] - prev["accum"][0] / 24).max() < 1e-12
        assert np.array_equal(accum[5], cur["accum"][5]) and m2[5] == cur["m2"][5]  # the sky pixel: untouched
        mean = (accum[1:5] - cur["accum"][1:5]) / hist[1:5, None]
        assert np.abs(mean - prev["accum"][1:5] / 24).max() < 1e-12


def test_reference_without_previous_samples_changes_nothing():
    W, H = 3, 2
    cam = cam_of(W, H)
    prev = _smooth(W, H, [0] * 6, fs=8)
    cur = _smooth(W, H, [0, 4, 4, 4, 4, 4])
    cur["accum"][0], cur["m2"][0] = np.nan, np.nan
    accum, m2, counts, hist = temporal_ref.accumulate(W, H, cam, cur, cam, prev)
    assert (hist == 0).all() and np.array_equal(counts, cur["counts"])
    assert np.array_equal(accum.view(np.int64), cur["accum"].view(np.int64))
    assert np.array_equal(m2.view(np.int64), cur["m2"].view(np.int64))

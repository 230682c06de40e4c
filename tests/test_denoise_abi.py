"""The denoiser, the part that needs no GPU (include/rt.h rt_denoise): both symbols are
exported and bound, the ABI version did not move, the defaults are the documented ones, every argument
check answers without a device and names what it refused, the Python entry points exist with their
signatures, the denoise kernels exist without scratch memory (checked at build time, as
tests/test_features_abi.py does for the feature kernels), and the numpy reference passes a sanity pin
of its own."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import denoise_ref
import rtzig
from abi_support import RT_ERR_INVALID, ROOT, assert_bound, assert_invalid, cam_of, resources
from rtzig.abi import RtDenoiseParams

DEFAULTS = dict(levels=2, reserved=0, sigma_l=4.0, sigma_n=32.0, sigma_a=32.0, sigma_z=0.05, sigma_h=4.0,
                epsilon=1e-6)


def test_symbols_exported_bound_and_declared():
    with open(os.path.join(ROOT, "include", "rt.h")) as f:
        header = f.read()
    for name, nargs in (("rt_denoise", 16), ("rt_denoise_default_params", 1)):
        assert_bound(name, nargs)
        assert re.search(r"\bint %s\(" % name, header)
    assert "typedef struct rt_denoise_params" in header


def test_abi_version_unchanged():
    assert rtzig.load().rt_abi_version() == 3


def test_default_params():
    p = RtDenoiseParams()
    assert C.sizeof(p) == rtzig.abi.DENOISE_PARAMS_SIZE == 56
    assert rtzig.load().rt_denoise_default_params(C.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in RtDenoiseParams._fields_} == DEFAULTS
    assert rtzig.load().rt_denoise_default_params(None) == RT_ERR_INVALID
    q = rtzig.denoise_params()
    assert {k: getattr(q, k) for k, _ in RtDenoiseParams._fields_} == DEFAULTS
    q = rtzig.denoise_params(levels=2, sigma_z=0.5)
    assert (q.levels, q.sigma_z, q.sigma_l) == (2, 0.5, 4.0)
    with pytest.raises(TypeError):
        rtzig.denoise_params(sigma=1.0)
    assert {k: v for k, v in DEFAULTS.items() if k != "reserved"} == denoise_ref.DEFAULTS


def denoise_call(ctx=None, width=4, height=3, accum=1, m2=1, counts=1, albedo=0, normal=0, depth=0, hits=0,
                 feature_samples=0, params=None, fmt=0, out=1, var_out=0):
    """rt_denoise with made-up non-null pointers (never dereferenced: a null context answers last)."""
    lib = rtzig.load()
    p = C.c_void_p
    return lib.rt_denoise(ctx, width, height, p(accum * 4096), p(m2 * 4096), p(counts * 4096), p(albedo * 4096),
                          p(normal * 4096), p(depth * 4096), p(hits * 4096), feature_samples,
                          C.byref(params) if params is not None else None, fmt, p(out * 4096), p(var_out * 4096),
                          None)


@pytest.mark.parametrize("kw, word", [
    (dict(), b"context"),                                    # everything else valid: the null context answers
    (dict(albedo=1, normal=1, depth=1, hits=1, feature_samples=4, var_out=1), b"context"),
    (dict(accum=0), b"accumulator"),
    (dict(m2=0), b"m2"),
    (dict(counts=0), b"counts"),
    (dict(out=0), b"output"),
    (dict(width=0), b"width"),
    (dict(height=0), b"height"),
    (dict(width=65536, height=65536), b"2^32"),
    (dict(depth=1, feature_samples=4), b"depth"),
    (dict(albedo=1), b"feature_samples"),
    (dict(normal=1), b"feature_samples"),
    (dict(hits=1), b"feature_samples"),
    (dict(depth=1, hits=1), b"feature_samples"),
    (dict(params=dict(levels=17)), b"levels"),
    (dict(params=dict(sigma_l=-1.0)), b"sigma_l"),
    (dict(params=dict(sigma_n=float("nan"))), b"sigma_n"),
    (dict(params=dict(sigma_a=-0.5)), b"sigma_a"),
    (dict(params=dict(sigma_z=float("nan"))), b"sigma_z"),
    (dict(params=dict(sigma_h=-1e-300)), b"sigma_h"),
    (dict(params=dict(epsilon=0.0)), b"epsilon"),
    (dict(params=dict(epsilon=float("nan"))), b"epsilon"),
    (dict(params=dict(reserved=1)), b"reserved"),
    (dict(fmt=2), b"output_format"),
], ids=["ctx", "ctx-all-guides", "accum", "m2", "counts", "out", "width", "height", "too-many-pixels",
        "depth-without-hits", "albedo-no-samples", "normal-no-samples", "hits-no-samples", "depth-no-samples", "levels",
        "sigma_l", "sigma_n", "sigma_a", "sigma_z", "sigma_h", "epsilon-zero", "epsilon-nan", "reserved", "format"])
def test_invalid_arguments_answer_without_a_device(kw, word):
    kw = dict(kw)
    if "params" in kw:
        kw["params"] = rtzig.denoise_params(**kw["params"])
    assert_invalid(denoise_call(**kw), word)


def test_limits_that_pass_the_checks():
    """levels == 16, a zero sigma and 2^32 - 65536 pixels are allowed: the null context answers instead."""
    for kw in (dict(params=rtzig.denoise_params(levels=16, sigma_l=0.0, sigma_z=0.0)),
               dict(width=65535, height=65536)):
        assert_invalid(denoise_call(**kw), b"context")


def test_python_entry_points_and_signatures():
    for name in ("render_denoised", "denoise_params", "RtDenoiseParams"):
        assert name in rtzig.__all__ and hasattr(rtzig, name)
    sig = inspect.signature(rtzig.render_denoised)
    assert list(sig.parameters) == ["cam", "spheres", "spp", "feature_spp", "params", "adaptive", "device", "output",
                                    "precision"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(feature_spp=4, params=None, adaptive=None, device=0, output="linear", precision="f64")
    msig = inspect.signature(rtzig.Camera.render_denoised)
    assert list(msig.parameters) == ["self"] + list(sig.parameters)[2:]
    assert {k: v.default for k, v in msig.parameters.items() if v.default is not inspect.Parameter.empty} == defaults
    sig = inspect.signature(rtzig.DeviceRenderer.denoise)
    assert list(sig.parameters) == ["self", "width", "height", "d_accum_ptr", "d_m2_ptr", "d_counts_ptr", "d_out_ptr",
                                    "d_albedo_ptr", "d_normal_ptr", "d_depth_ptr", "d_hits_ptr", "feature_samples",
                                    "params", "output", "d_var_out_ptr", "stream_ptr"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(d_albedo_ptr=None, d_normal_ptr=None, d_depth_ptr=None, d_hits_ptr=None, feature_samples=0,
                            params=None, output="linear", d_var_out_ptr=None, stream_ptr=None)
    # the existing adaptive entry point did not move
    assert list(inspect.signature(rtzig.render_adaptive).parameters) == [
        "cam", "spheres", "min_spp", "max_spp", "step", "tolerance", "floor", "device", "output", "precision",
        "on_round"]


@pytest.mark.parametrize("kw", [dict(spp=1), dict(spp=0), dict(spp=-3), dict(spp=2 ** 32), dict(spp=4, feature_spp=0),
                                dict(spp=4, feature_spp=-1), dict(spp=4, output="hdr"),
                                dict(spp=4, adaptive=dict(max_spp=8)), dict(spp=4, adaptive=dict(max_spp=2, step=1, tolerance=0.1)),
                                dict(spp=4, adaptive=dict(max_spp=8, step=1, tolerance=0.1, ceiling=1))])
def test_render_denoised_rejects_bad_arguments_before_any_device_work(kw):
    with pytest.raises(ValueError):
        rtzig.render_denoised(cam_of(), [], **kw)  # an empty scene: never reached


# ---- the denoise kernels' resources (build time) ----------------------------------------------------
def test_denoise_kernels_exist_without_scratch_outside_the_other_counts():
    rows = resources("rt_denoise.hip")
    assert rows and all("denoise_" in k for k in rows), sorted(rows)  # the translation unit holds nothing else
    for stage in ("denoise_prepare_kernel", "denoise_prefilter_kernel", "denoise_level_tile_kernel",
                  "denoise_level_direct_kernel"):
        assert len([k for k in rows if stage in k]) == 1, (stage, sorted(rows))
    assert not any("sample_kernel" in k or "feature_kernel" in k for k in rows)
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in rows.values()), rows
    tile = next(v for k, v in rows.items() if "denoise_level_tile_kernel" in k)
    # 12 planes of 36 x 12 doubles; three blocks fit a CU's 160 KiB
    assert tile["LDS Size [bytes/block]"] == 12 * 36 * 12 * 8 and 3 * tile["LDS Size [bytes/block]"] <= 160 * 1024
    assert tile["Occupancy [waves/SIMD]"] >= 3


# ---- the reference's own sanity pin ------------------------------------------------------------------
def test_reference_on_one_pixel():
    """A 1 x 1 image has the centre tap only: d = 0, t = 1, w = 36/256, and a level returns
    (w * c) * (1 / w) and ((w * w) * v) * ((1 / w) * (1 / w)).  With levels == 0 the result IS the
    prepared colour and variance.  With levels > 0 it is not bit-equal in general — w * c rounds (9 c needs
    up to four more bits than c) and 1 / w = 64 / 9 is not a binary fraction (measured: 1329 of 2000 random
    colours move after five levels) — but every level is three roundings of the colour (w * c, 1 / w, the
    product) and five of the variance, so after k levels it is within 3k resp. 5k relative half-ulps
    (k * 3 * 2^-53, first order; asserted with the second-order slack of a factor 1 + 2^-40).  For c = 1
    and c = 0 the round trip is exact: fl(w * fl(1 / w)) == 1."""
    rng = np.random.default_rng(7)
    u = 2.0 ** -53
    for trial in range(50):
        n = int(rng.integers(2, 40))
        accum = rng.random((1, 3)) * n
        S = (accum[0, 0] + accum[0, 1]) + accum[0, 2]
        m2 = np.array([S * (S / n) * (1.0 + rng.random())])
        counts = np.array([n])
        c0, v0 = denoise_ref.denoise(1, 1, accum, m2, counts, levels=0)
        want_c = accum * (1.0 / np.float64(n))
        want_v = ((m2 - S * (S / np.float64(n))) / (n - 1.0)) / n
        assert np.array_equal(c0.reshape(1, 3), want_c) and np.array_equal(v0.reshape(1), want_v)
        assert v0[0, 0] > 0
        for k in (1, 3, 5, 6):
            ck, vk = denoise_ref.denoise(1, 1, accum, m2, counts, levels=k)
            assert (np.abs(ck - c0) <= 3 * k * u * (1 + 2.0 ** -40) * np.abs(c0)).all()
            assert (np.abs(vk - v0) <= 5 * k * u * (1 + 2.0 ** -40) * np.abs(v0)).all()
    one = np.array([[4.0, 4.0, 0.0]])  # n = 4: c = (1, 1, 0)
    c5, _ = denoise_ref.denoise(1, 1, one, np.array([16.0]), np.array([4]))
    assert np.array_equal(c5.reshape(3), [1.0, 1.0, 0.0])

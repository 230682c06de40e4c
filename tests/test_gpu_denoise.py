"""The denoiser on the GPU (include/rt.h rt_denoise).  The filter is defined operation
by operation in f64, so every comparison here is of bits: rt_denoise's image and variance against
tests/denoise_ref.py (numpy) on synthetic buffers — no render, which isolates the filter — for shapes
that cross the 32 x 8 tile in both directions and are multiples of nothing, level counts up to a step
beyond the image, both forced kernel forms, and inputs that reach every branch of the definition.
Then the layers above it end to end on chapter 13, with the GPU's own one-pass renders (which other
tests pin to oracle B) as yardsticks."""
import numpy as np
import pytest
import torch

import denoise_ref
import domain_values
import rtzig
from gpu_support import DEV, rmse, same_bits
from gpu_support import module_renderers, renderers  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (1, 40), (37, 23), (70, 45)]  # (W, H)
LEVELS = [0, 1, 3, 6]                                   # at 6 the step of 32 exceeds several dimensions
FORMS = [None, "tile", "direct"]                        # RTZIG_DENOISE_FORM: the default choice and both forced
ALT = dict(sigma_l=1.5, sigma_n=3.0, sigma_a=0.75, sigma_z=0.4, sigma_h=0.0, epsilon=1e-3)
FS = 4                                                  # feature samples of the synthetic guides
PATTERNS = ["smooth", "random", "constant", "counts", "v-negative", "zero-variance", "hits-zero", "huge-counts"]


def synthetic(pattern, W, H):
    """Host buffers as the gather and feature passes leave them: accum (P, 3), m2 (P), counts (P),
    albedo (P, 3), normal (P, 3), depth (P), hits (P); finite everywhere.
      smooth         guides vary slowly, colour is a smooth image plus noise: weights mostly in (0, 1)
      random         guides are noise: weights mostly 0
      constant       every pixel the same
      counts         counts of 0, 1, 2 and uneven larger values
      v-negative     m2 slightly below S * mean: the variance clamps to 0
      zero-variance  dyadic values, m2 == S * mean exactly: v == 0, the luminance weight is 1 / epsilon wide
      hits-zero      pixels without a hit (z == 0, coverage 0) next to hit pixels
      huge-counts    counts of 2^31 and 2^32 - 1 beside 16: the u32 converts to double unsigned"""
    P = W * H
    rng = np.random.default_rng(1000 * W + H + len(pattern))
    j, i = np.divmod(np.arange(P), W)
    x, y = i / max(W - 1, 1), j / max(H - 1, 1)
    counts = np.full(P, 16, np.int64)
    hits = np.full(P, FS, np.int64)
    base = np.stack([0.2 + 0.6 * x, 0.3 + 0.4 * y, 0.5 + 0.2 * x * y], 1)
    noise = 1 + 0.3 * (rng.random((P, 3)) - 0.5)
    nrm = np.stack([0.3 * x, 0.3 * y, 1 - 0.1 * x], 1)
    alb = np.stack([0.5 + 0.1 * x, 0.4 + 0.1 * y, 0.6 - 0.1 * x], 1)
    zed = 3 + x + 0.5 * y
    spread = 1.05 + 0.5 * rng.random(P)  # m2 / (S * mean): > 1, so v > 0
    if pattern == "random":
        nrm, alb, zed = rng.random((P, 3)) * 2 - 1, rng.random((P, 3)), 1 + 9 * rng.random(P)
        hits = rng.integers(0, FS + 1, P)
    elif pattern == "constant":
        base, noise = np.tile([0.4, 0.5, 0.3], (P, 1)), 1.0
        nrm, alb, zed = np.tile([0.0, 0.6, 0.8], (P, 1)), np.tile([0.5, 0.5, 0.5], (P, 1)), np.full(P, 4.0)
        spread = np.full(P, 1.25)
    elif pattern == "counts":
        counts = rng.choice([0, 1, 2, 3, 16, 40, 500], P)
    elif pattern == "zero-variance":
        base, noise = rng.integers(0, 9, (P, 3)) / 8.0, 1.0
    elif pattern == "hits-zero":
        hits = np.where((i // 3 + j // 2) % 2 == 0, 0, rng.integers(1, FS + 1, P))
    elif pattern == "huge-counts":
        counts = np.array([2 ** 31, 2 ** 32 - 1, 16], np.int64)[(i + 2 * j) % 3] if P > 1 else np.array([2 ** 31])
    c = counts.astype(np.float64)
    accum = base * noise * c[:, None]
    S = (accum[:, 0] + accum[:, 1]) + accum[:, 2]
    mean = S / np.maximum(c, 1)
    m2 = S * mean * spread
    if pattern == "v-negative":
        m2 = S * mean * (1 - 1e-12)
    if pattern == "zero-variance":
        m2 = S * mean  # exact: S and mean are small dyadic numbers
    h = hits.astype(np.float64)
    return dict(accum=accum, m2=m2, counts=counts, albedo=alb * h[:, None], normal=nrm * h[:, None], depth=zed * h,
                hits=hits)


class Device:
    """The buffers of one image on the device, and the call."""

    def __init__(self, W, H, host):
        self.W, self.H, self.host = W, H, host
        # counts and hits are u32 on the device: the low 32 bits, carried in an int32 tensor
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v.astype(np.uint32).view(np.int32) if k in ("counts", "hits")
                                                           else v)).to(DEV)
                  for k, v in host.items()}
        self.before = {k: v.clone() for k, v in self.t.items()}

    def run(self, r, params=None, output="linear", var=True, skip=(), feature_samples=FS):
        P = self.W * self.H
        if output == "linear":
            out = torch.full((P, 3), float("nan"), dtype=torch.float64, device=DEV)
        else:
            out = torch.full((P, 3), 77, dtype=torch.uint8, device=DEV)
        v = torch.full((P,), float("nan"), dtype=torch.float64, device=DEV) if var else None
        g = {k: (None if k in skip else self.t[k].data_ptr()) for k in ("albedo", "normal", "depth", "hits")}
        r.denoise(self.W, self.H, self.t["accum"].data_ptr(), self.t["m2"].data_ptr(), self.t["counts"].data_ptr(),
                  out.data_ptr(), d_albedo_ptr=g["albedo"], d_normal_ptr=g["normal"], d_depth_ptr=g["depth"],
                  d_hits_ptr=g["hits"], feature_samples=feature_samples, params=params, output=output,
                  d_var_out_ptr=v.data_ptr() if var else None)
        torch.cuda.synchronize()
        return out.cpu().numpy(), (v.cpu().numpy() if var else None)

    def ref(self, skip=(), feature_samples=FS, **params):
        g = {k: (None if k in skip else self.host[k]) for k in ("albedo", "normal", "depth", "hits")}
        c, v = denoise_ref.denoise(self.W, self.H, self.host["accum"], self.host["m2"], self.host["counts"],
                                   feature_samples=feature_samples, **g, **params)
        return c.reshape(-1, 3), v.reshape(-1)

    def unchanged(self):
        return all(torch.equal(self.t[k].view(torch.uint8), self.before[k].view(torch.uint8)) for k in self.t)


@pytest.fixture(scope="module")
def rend(module_renderers):
    return module_renderers()


# ---- the filter against its definition --------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_bits_against_numpy(rend, monkeypatch, shape, pattern):
    W, H = shape
    d = Device(W, H, synthetic(pattern, W, H))
    for sig in ({}, ALT):
        for levels in LEVELS:
            want_c, want_v = d.ref(levels=levels, **sig)
            assert np.isfinite(want_c).all() and np.isfinite(want_v).all()  # the inputs keep the contract
            for form in FORMS:
                if form is None:
                    monkeypatch.delenv("RTZIG_DENOISE_FORM", raising=False)
                else:
                    monkeypatch.setenv("RTZIG_DENOISE_FORM", form)
                got_c, got_v = d.run(rend, rtzig.denoise_params(levels=levels, **sig))
                where = (pattern, shape, levels, form, bool(sig))
                assert same_bits(got_c, want_c), where  # NaN pre-fill: also "fully overwritten"
                assert same_bits(got_v, want_v), where
    assert d.unchanged()
    if pattern == "v-negative":
        assert (denoise_ref.prepare(W, H, **{k: d.host[k] for k in ("accum", "m2", "counts")})[1] == 0).all()
    if pattern == "constant" and W * H > 1:
        c5, _ = d.ref()
        assert np.abs(c5 - [0.4, 0.5, 0.3]).max() < 1e-12  # a constant image stays (to rounding) constant


@pytest.mark.parametrize("shape, levels", [((37, 23), 16), ((300, 2), 9), ((2, 100), 9)],
                         ids=["37x23-levels16", "300x2-levels9", "2x100-levels9"])
def test_every_level_rt_h_allows_and_long_thin_images(rend, monkeypatch, shape, levels):
    """levels = 16 (step 32768, the most rt.h allows) and two long thin images at levels = 9: step 256
    still has taps inside the 300-wide image, and a step's lattice has more than one 32 x 8 tile at
    steps 1 to 8 of 300 x 2 and at step 8 of 2 x 100, which no image up to 70 x 45 reaches beyond
    step 4.  Level counts from 0 up to `levels`, all three forms."""
    W, H = shape
    for pattern in ("smooth", "huge-counts"):
        d = Device(W, H, synthetic(pattern, W, H))
        for lv in sorted({0, 1, 4, 7, levels - 1, levels}):
            want_c, want_v = d.ref(levels=lv)
            assert np.isfinite(want_c).all() and np.isfinite(want_v).all()
            for form in FORMS:
                if form is None:
                    monkeypatch.delenv("RTZIG_DENOISE_FORM", raising=False)
                else:
                    monkeypatch.setenv("RTZIG_DENOISE_FORM", form)
                got_c, got_v = d.run(rend, rtzig.denoise_params(levels=lv))
                assert same_bits(got_c, want_c) and same_bits(got_v, want_v), (pattern, shape, lv, form)
        assert d.unchanged()
    if W == 300:  # the large steps do reach pixels: level 9 (step 256) still moves the image
        assert not same_bits(d.ref(levels=8)[0], d.ref(levels=9)[0])


def test_huge_counts_reach_the_prepare_pass_unsigned():
    """What the huge-counts pattern is for, on the reference: its prepared colours are those of the
    same means at count 16 to rounding, where a count read as a signed 32-bit number would flip the
    sign (2^31) or scale by -1 (2^32 - 1)."""
    W, H = 37, 23
    h = synthetic("huge-counts", W, H)
    assert set(np.unique(h["counts"])) == {16, 2 ** 31, 2 ** 32 - 1}
    c, var = denoise_ref.prepare(W, H, h["accum"], h["m2"], h["counts"])[:2]
    assert (c > 0.05).all() and (c < 1.0).all() and (var >= 0).all()
    signed = h["counts"].astype(np.uint32).view(np.int32).astype(np.int64)
    assert (denoise_ref.prepare(W, H, h["accum"], h["m2"], signed)[0] < 0).any()


def test_rgb8_sink_on_the_byte_boundaries(rend, oracle):
    """The denoiser's RGB8 sink at levels = 0 (the prepared colour, counts of 1) on every input at which
    Color.toRgb changes its byte, and on zero, negative, huge and subnormal sums.  Finite values only:
    finite sums are the contract."""
    vals = domain_values.channel_values(finite_only=True)
    W, H = len(vals) // 2, 2
    P = W * H
    assert P == len(vals) and np.isfinite(vals).all()
    accum = domain_values.pixels(P, finite_only=True)
    host = dict(accum=accum, m2=np.zeros(P), counts=np.ones(P, np.int64), albedo=np.zeros((P, 3)),
                normal=np.zeros((P, 3)), depth=np.zeros(P), hits=np.zeros(P, np.int64))
    d = Device(W, H, host)
    p0 = rtzig.denoise_params(levels=0)
    lin, var = d.run(rend, p0)
    assert same_bits(lin, accum) and (var == 0).all()  # x * (1.0 / 1.0) is x; one sample has no variance
    rgb, _ = d.run(rend, p0, output="rgb8", var=False)
    assert np.array_equal(rgb, oracle.to_rgb8(accum)), np.argwhere(rgb != oracle.to_rgb8(accum))[:8].tolist()
    assert len(np.unique(rgb)) == 256 and d.unchanged()


def test_the_patterns_reach_partial_weights_and_zero_weights():
    """What the synthetic inputs are for, checked on the reference: 'smooth' has most tap weights
    strictly between 0 and the full kernel weight, 'random' has most of them 0."""
    W, H = 37, 23
    frac = {}
    for pattern in ("smooth", "random"):
        h = synthetic(pattern, W, H)
        c0, v0 = denoise_ref.denoise(W, H, h["accum"], h["m2"], h["counts"], h["albedo"], h["normal"], h["depth"],
                                     h["hits"], FS, levels=0)
        c1, _ = denoise_ref.denoise(W, H, h["accum"], h["m2"], h["counts"], h["albedo"], h["normal"], h["depth"],
                                    h["hits"], FS, levels=1)
        frac[pattern] = float(np.mean(np.abs(c1 - c0).max(-1) > 1e-9))  # pixels a level moved at all
    assert frac["smooth"] > 0.9 and frac["random"] < frac["smooth"]


@pytest.mark.parametrize("skip", [("albedo",), ("normal",), ("depth",), ("depth", "hits"),
                                  ("albedo", "normal", "depth", "hits")],
                         ids=["no-albedo", "no-normal", "no-depth", "no-hits", "no-guides"])
def test_null_guides(rend, skip):
    """A guide whose pointer is NULL is 0 everywhere.  hits is the divisor of depth, so it leaves with depth."""
    W, H = 37, 23
    d = Device(W, H, synthetic("hits-zero", W, H))
    fs = 0 if len(skip) == 4 else FS
    for levels in (0, 3):
        want_c, want_v = d.ref(skip=skip, feature_samples=fs, levels=levels)
        got_c, got_v = d.run(rend, rtzig.denoise_params(levels=levels), skip=skip, feature_samples=fs)
        assert same_bits(got_c, want_c) and same_bits(got_v, want_v), (skip, levels)
    full_c, _ = d.ref(levels=3)
    assert not same_bits(full_c, want_c)  # the guide that left did matter


def test_rgb8_default_params_no_variance_and_determinism(rend, oracle):
    W, H = 70, 45
    d = Device(W, H, synthetic("smooth", W, H))
    lin, var = d.run(rend)  # params None: the defaults
    want_c, want_v = d.ref()
    assert same_bits(lin, want_c) and same_bits(var, want_v)
    rgb, none = d.run(rend, output="rgb8", var=False)  # d_var_out is optional
    assert none is None and rgb.dtype == np.uint8
    assert np.array_equal(rgb, oracle.to_rgb8(lin))
    assert len(np.unique(rgb)) > 20
    rgb0, _ = d.run(rend, rtzig.denoise_params(levels=0), output="rgb8", var=False)
    assert np.array_equal(rgb0, oracle.to_rgb8(d.ref(levels=0)[0]))
    lin2, var2 = d.run(rend)
    assert same_bits(lin2, lin) and same_bits(var2, var)
    assert d.unchanged()


def test_other_stream_and_timing(rend):
    """Asynchronous on the caller's stream; the context's events report the call as the sample kernel."""
    W, H = 70, 45
    d = Device(W, H, synthetic("smooth", W, H))
    want_c, want_v = d.ref()
    out = torch.full((W * H, 3), float("nan"), dtype=torch.float64, device=DEV)
    var = torch.full((W * H,), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    rend.enable_timing(True)
    try:
        for _ in range(2):  # the second call reuses the planes the first one still reads: stream order
            rend.denoise(W, H, d.t["accum"].data_ptr(), d.t["m2"].data_ptr(), d.t["counts"].data_ptr(), out.data_ptr(),
                         d_albedo_ptr=d.t["albedo"].data_ptr(), d_normal_ptr=d.t["normal"].data_ptr(),
                         d_depth_ptr=d.t["depth"].data_ptr(), d_hits_ptr=d.t["hits"].data_ptr(), feature_samples=FS,
                         d_var_out_ptr=var.data_ptr(), stream_ptr=s.cuda_stream)
        sample_ms, reduce_ms = rend.kernel_times()
    finally:
        rend.enable_timing(False)
    s.synchronize()
    assert sample_ms > 0 and reduce_ms < 0.05 * sample_ms + 0.01
    assert same_bits(out.cpu().numpy(), want_c) and same_bits(var.cpu().numpy(), want_v)


def test_workspace_is_128_bytes_per_pixel_and_given_back(renderers):
    r = renderers()
    base = r.workspace_bytes()
    for (W, H), want in (((70, 45), 128 * 3150),    # a fresh context: exactly the planes
                         ((64, 45), 128 * 3150),    # 2880 pixels: within 25% of what is held, kept
                         ((37, 23), 128 * 851),     # far smaller: given back and reallocated
                         ((70, 45), 128 * 3150)):
        d = Device(W, H, synthetic("smooth", W, H))
        got_c, got_v = d.run(r, rtzig.denoise_params(levels=2))
        assert r.workspace_bytes() - base == want, (W, H)
        want_c, want_v = d.ref(levels=2)
        assert same_bits(got_c, want_c) and same_bits(got_v, want_v)
    r.enable_profile(True)  # instrumented contexts are accepted
    got_c, _ = d.run(r, rtzig.denoise_params(levels=2))
    assert same_bits(got_c, want_c)
    r.sync()
    r.close()


def test_argument_errors_with_a_live_context_and_a_pending_deferred_pass(monkeypatch, renderers):
    """Every refusal leaves the buffers alone; a good call is a plain call: it first runs the reduce pass
    a deferred render left pending, whose frame is then complete on that render's out stream."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", "direct")
    cam = rtzig.final_scene_camera(width=37, aspect_ratio=16 / 9, spp=4)
    W, H = cam.width, cam.height
    r = renderers(cam)
    plain = torch.zeros((H, W, 3), dtype=torch.float64, device=DEV)
    r.render_rows_async(cam.cam, plain.data_ptr())
    d = Device(W, H, synthetic("smooth", W, H))
    out = torch.full((W * H, 3), float("nan"), dtype=torch.float64, device=DEV)
    a, m, c = d.t["accum"].data_ptr(), d.t["m2"].data_ptr(), d.t["counts"].data_ptr()
    g = dict(d_albedo_ptr=d.t["albedo"].data_ptr(), d_normal_ptr=d.t["normal"].data_ptr(),
             d_depth_ptr=d.t["depth"].data_ptr(), d_hits_ptr=d.t["hits"].data_ptr(), feature_samples=FS)
    torch.cuda.synchronize()
    held = r.workspace_bytes()
    for args, kw, word in (((W, H, None, m, c, out.data_ptr()), g, "accumulator"),
                           ((W, H, a, None, c, out.data_ptr()), g, "m2"),
                           ((W, H, a, m, None, out.data_ptr()), g, "counts"),
                           ((W, H, a, m, c, None), g, "output"),
                           ((0, H, a, m, c, out.data_ptr()), g, "width"),
                           ((W, H, a, m, c, out.data_ptr()), dict(g, d_hits_ptr=None), "depth"),
                           ((W, H, a, m, c, out.data_ptr()), dict(g, feature_samples=0), "feature_samples"),
                           ((W, H, a, m, c, out.data_ptr()), dict(g, params=rtzig.denoise_params(levels=17)), "levels"),
                           ((W, H, a, m, c, out.data_ptr()), dict(g, params=rtzig.denoise_params(sigma_z=-1.0)), "sigma_z"),
                           ((W, H, a, m, c, out.data_ptr()), dict(g, params=rtzig.denoise_params(epsilon=0.0)), "epsilon"),
                           ((W, H, a, m, c, out.data_ptr()), dict(g, params=rtzig.denoise_params(reserved=3)), "reserved")):
        with pytest.raises(rtzig.RtError) as e:
            r.denoise(*args, **kw)
        assert e.value.code == -1 and word in str(e.value), word
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and d.unchanged() and r.workspace_bytes() == held
    frame = torch.zeros((H, W, 3), dtype=torch.float64, device=DEV)
    render, coll = torch.cuda.Stream(), torch.cuda.Stream()
    r.render_rows_async(cam.cam, frame.data_ptr(), stream_ptr=render.cuda_stream, out_stream_ptr=coll.cuda_stream,
                        deferred=True)
    assert r.fold_pending()
    r.denoise(W, H, a, m, c, out.data_ptr(), stream_ptr=render.cuda_stream, **g)
    assert not r.fold_pending()
    with torch.cuda.stream(coll):
        got = frame.clone()  # ordered after the deferred frame's output
    torch.cuda.synchronize()
    r.sync()
    r.close()
    assert torch.equal(got, plain)
    assert same_bits(out.cpu().numpy(), d.ref()[0])


# ---- end to end: chapter 13 at width 96 ------------------------------------------------------------
SPP, FSPP = 16, 4


def cam13(spp=1):
    return rtzig.chapter13_camera(width=96, aspect_ratio=16 / 9, spp=spp)


_ONE_PASS = {}


def one_pass(spp):
    """The GPU's one-pass render of the scene at `spp` (other tests pin it to oracle B); computed once."""
    if spp not in _ONE_PASS:
        cam = cam13(spp)
        img = rtzig.render(cam.cam, cam.scene.world, n_gpus=1)
        img.setflags(write=False)
        _ONE_PASS[spp] = img
    return _ONE_PASS[spp]


def fill_buffers(make, cam, counts):
    """The buffers the test fills itself: every pixel brought to its count by gather passes (one pass per
    distinct count, over the pixels that have it), and FSPP feature samples.  Host arrays."""
    W, H = cam.width, cam.height
    P = W * H
    r = make(cam)
    accum = torch.empty((P, 3), dtype=torch.float64, device=DEV)
    m2 = torch.empty(P, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(P, dtype=torch.int32, device=DEV)
    sums = torch.empty((2, P, 3), dtype=torch.float64, device=DEV)
    depth = torch.empty(P, dtype=torch.float64, device=DEV)
    hits = torch.empty(P, dtype=torch.int32, device=DEV)
    flat = np.asarray(counts).reshape(-1).astype(np.int64)
    for n in np.unique(flat):
        lst = None if (flat == n).all() else np.flatnonzero(flat == n)
        r.accumulate_pixels(cam.cam, lst, int(n), accum.data_ptr(), m2.data_ptr(), cnt.data_ptr())
    r.features(cam.cam, 0, FSPP, sums[0].data_ptr(), sums[1].data_ptr(), depth.data_ptr(), hits.data_ptr())
    torch.cuda.synchronize()
    host = dict(accum=accum.cpu().numpy(), m2=m2.cpu().numpy(), counts=cnt.cpu().numpy().astype(np.int64),
                albedo=sums[0].cpu().numpy(), normal=sums[1].cpu().numpy(), depth=depth.cpu().numpy(),
                hits=hits.cpu().numpy().astype(np.int64))
    r.sync()
    r.close()
    assert np.array_equal(host["counts"], flat)
    return host


def test_render_denoised_end_to_end(oracle, renderers):
    cam = cam13()
    W, H = cam.width, cam.height
    res = rtzig.render_denoised(cam.cam, cam.scene.world, SPP, feature_spp=FSPP)
    assert res["image"].shape == (H, W, 3) and res["noisy"].shape == (H, W, 3)
    assert res["variance"].shape == (H, W) and res["counts"].shape == (H, W) and res["counts"].dtype == np.uint32
    assert (res["counts"] == SPP).all()
    assert same_bits(res["noisy"], one_pass(SPP))
    host = fill_buffers(renderers, cam, res["counts"])
    want_c, want_v = denoise_ref.denoise(W, H, host["accum"], host["m2"], host["counts"], host["albedo"],
                                         host["normal"], host["depth"], host["hits"], FSPP)
    assert same_bits(res["image"], want_c) and same_bits(res["variance"], want_v)  # the layers add nothing
    # quality: better than doubling the samples (the CPU prototype: 0.0199 against 0.0283)
    R = one_pass(2048)
    e_noisy, e_denoised, e_32 = rmse(res["noisy"], R), rmse(res["image"], R), rmse(one_pass(32), R)
    print(f"RMSE vs 2048 spp: noisy 16 spp {e_noisy:.5f}, denoised {e_denoised:.5f}, plain 32 spp {e_32:.5f}")
    assert e_denoised < e_32
    # the Camera method and the fused rgb8 output
    res8 = cam.render_denoised(SPP, feature_spp=FSPP, output="rgb8")
    assert np.array_equal(res8["image"], oracle.to_rgb8(res["image"]))
    assert np.array_equal(res8["noisy"], oracle.to_rgb8(res["noisy"]))
    assert same_bits(res8["variance"], res["variance"])


def test_render_denoised_adaptive(renderers):
    cam = cam13()
    W, H = cam.width, cam.height
    res = rtzig.render_denoised(cam.cam, cam.scene.world, SPP, feature_spp=FSPP,
                                adaptive=dict(max_spp=64, step=16, tolerance=0.05), params=rtzig.denoise_params(levels=3))
    counts = res["counts"].astype(np.int64)
    assert set(np.unique(counts)) <= {16, 32, 48, 64} and len(np.unique(counts)) >= 2, np.unique(counts, return_counts=True)
    want_noisy = np.zeros((H, W, 3))
    for n in np.unique(counts):  # every pixel is the pixel of the one-pass render at its own count
        want_noisy[counts == n] = one_pass(int(n))[counts == n]
    assert same_bits(res["noisy"], want_noisy)
    img, cnt = rtzig.render_adaptive(cam.cam, cam.scene.world, SPP, 64, 16, 0.05)
    assert np.array_equal(cnt, res["counts"]) and same_bits(img, res["noisy"])  # render_adaptive's loop, unchanged
    host = fill_buffers(renderers, cam, counts)
    want_c, want_v = denoise_ref.denoise(W, H, host["accum"], host["m2"], host["counts"], host["albedo"],
                                         host["normal"], host["depth"], host["hits"], FSPP, levels=3)
    assert same_bits(res["image"], want_c) and same_bits(res["variance"], want_v)

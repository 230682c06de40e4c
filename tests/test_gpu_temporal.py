"""The temporal accumulation on the GPU (include/rt.h rt_temporal_accumulate).  The
operation is defined step by step in f64, so every comparison of the first part is of bits: the merged
accum, m2, counts and d_history against tests/temporal_ref.py (numpy) on synthetic buffers — no render,
which isolates the kernel — for shapes that cross the 32 x 8 tile in both directions and are multiples of
nothing, camera pairs that reach every exit of the projection, and buffers that reach every branch of the
tap tests and the merge.  Then properties with exact expectations that do not go through the numpy file,
and the layers above end to end (render_sequence) with the GPU's own one-pass renders as yardsticks."""
import numpy as np
import pytest
import torch

import rtzig
import temporal_ref
from gpu_support import DEV, bits, rmse, same_bits
from gpu_support import module_renderers  # noqa: F401 (fixture)
from rtzig.abi import RtCamera

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (1, 40), (37, 23), (70, 45)]  # (W, H)
FS, FS_PREV = 4, 8                                      # feature samples of the two frames' guides
R_WORLD = 12.0                                          # the synthetic world: the inside of this sphere
FROM, AT = (0.2, 0.4, 1.5), (0.0, 0.0, -1.0)


def build(W, H, look_from=FROM, look_at=AT, v_up=(0, 1, 0), vfov=40.0):
    """An rt_camera of exactly W x H pixels through rt_camera_build."""
    b = rtzig.CameraBuilder(W, W / (H + 0.5)).setViewport(look_from, look_at, vfov).setVUp(v_up)
    b.setSamplesPerPixel(1)
    cam = b.build().cam
    assert (cam.image_width, cam.image_height) == (W, H)
    return cam


def copy_cam(cam):
    return RtCamera.from_buffer_copy(cam)


def hit_points(cam):
    """Where the pixel-centre rays of `cam` meet the world sphere from inside: (X (P, 3), distance (P))."""
    W, H = cam.image_width, cam.image_height
    j, i = np.divmod(np.arange(W * H), W)
    o = np.array(list(cam.center))
    D = np.array(list(cam.pixel0)) + np.outer(i, list(cam.du)) + np.outer(j, list(cam.dv)) - o
    D /= np.linalg.norm(D, axis=1)[:, None]
    bq = D @ o
    t = -bq + np.sqrt(bq * bq - (o @ o - R_WORLD ** 2))
    return o + D * t[:, None], t


def shade(X):
    """Smooth, view-independent colour, albedo and normal of a world point."""
    x, y, z = X[:, 0] / R_WORLD, X[:, 1] / R_WORLD, X[:, 2] / R_WORLD
    col = np.stack([0.5 + 0.3 * x, 0.4 + 0.3 * y, 0.6 + 0.2 * z], 1)
    alb = np.stack([0.5 + 0.1 * x, 0.4 + 0.1 * y, 0.6 - 0.1 * z], 1)
    return col, alb, -X / R_WORLD


PATTERNS = ["smooth", "random", "counts", "cur-empty", "hits-zero", "cur-full", "half-guides"]


def frame(cam, pattern, which, fs):
    """Host buffers of one frame as the gather and feature passes leave them.  `which`: "cur" or "prev".
      smooth       consistent guides and depths: most taps valid
      random       the previous frame's guides and depths are noise: most taps invalid
      counts       previous counts of 0, 1 and uneven values
      cur-empty    current counts of 0, accum and m2 poisoned with NaN (they must not be read)
      hits-zero    pixels without a hit in either frame, next to hit pixels
      cur-full     current counts of 2^32 - 3: the last clamp of nh
      half-guides  feature sums of partly covered pixels: coverage and scaled guides differ between taps"""
    W, H = cam.image_width, cam.image_height
    P = W * H
    rng = np.random.default_rng(1000 * W + H + 7 * len(pattern) + (which == "prev"))
    j, i = np.divmod(np.arange(P), W)
    X, dist = hit_points(cam)
    col, alb, nrm = shade(X)
    counts = np.full(P, 16 if which == "cur" else 24, np.int64)
    hits = np.full(P, fs, np.int64)
    if pattern == "random" and which == "prev":
        nrm, alb = rng.random((P, 3)) * 2 - 1, rng.random((P, 3))
        dist = dist * (0.8 + 0.4 * rng.random(P))
    if pattern == "counts" and which == "prev":
        counts = rng.choice([0, 1, 2, 3, 16, 40, 500], P, p=[0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.4])
    if pattern == "cur-empty" and which == "cur":
        counts = np.where((i + j) % 3 == 0, 16, 0)
    if pattern == "hits-zero":
        hits = np.where((i // 3 + j // 2 + (which == "prev")) % 3 == 0, 0, rng.integers(1, fs + 1, P))
    if pattern == "cur-full" and which == "cur":
        counts = np.where((i + j) % 2 == 0, 2 ** 32 - 3, 2 ** 32 - 1)
    if pattern == "half-guides":
        hits = rng.integers(1, fs + 1, P)
    c = counts.astype(np.float64)
    accum = col * (1 + 0.3 * (rng.random((P, 3)) - 0.5)) * c[:, None]
    S = (accum[:, 0] + accum[:, 1]) + accum[:, 2]
    m2 = S * (S / np.maximum(c, 1)) * (1.05 + 0.5 * rng.random(P))
    if pattern == "cur-empty" and which == "cur":
        accum[counts == 0] = np.nan
        m2[counts == 0] = np.nan
    h = hits.astype(np.float64)
    return dict(accum=accum, m2=m2, counts=counts, albedo=alb * h[:, None], normal=nrm * h[:, None], depth=dist * h,
                hits=hits, feature_samples=fs)


def reconstructed_point(cam, depth, hits, p):
    """X of pixel p by the definition's own operations (temporal_ref's vectors are np.float64)."""
    pixel0, du, dv, center = temporal_ref.camera_vectors(cam)
    i, j = np.float64(p % cam.image_width), np.float64(p // cam.image_width)
    z = np.float64(depth[p]) / np.float64(hits[p])
    D = tuple(((pixel0[k] + du[k] * i) + dv[k] * j) - center[k] for k in range(3))
    g = z / np.sqrt(temporal_ref.dot(D, D))
    return tuple(float(center[k] + D[k] * g) for k in range(3))


def lattice_camera(W, H):
    """A hand-made camera on a dyadic lattice (centre 0, du = (2^-6, 0, 0), dv = (0, -2^-6, 0), image plane
    z = -1): with depth = 2 * |D| every step of the projection is exact, so u and v are exact integers."""
    cam = build(W, H)
    s = 2.0 ** -6
    for k in range(3):
        cam.center[k] = 0.0
        cam.du[k] = (s, 0.0, 0.0)[k]
        cam.dv[k] = (0.0, -s, 0.0)[k]
        cam.pixel0[k] = (-s * (W // 2), s * (H // 2), -1.0)[k]
    return cam


def lattice_depth(cam):
    W, H = cam.image_width, cam.image_height
    j, i = np.divmod(np.arange(W * H), W)
    D = np.array(list(cam.pixel0)) + np.outer(i, list(cam.du)) + np.outer(j, list(cam.dv))
    return 2.0 * np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])


def camera_pair(name, W, H):
    """(cam, cam_prev) of one named pair."""
    cam = build(W, H)
    if name == "identical":
        return cam, copy_cam(cam)
    if name == "subpixel-pan":
        return cam, build(W, H, look_at=(AT[0] + 0.0004, AT[1] - 0.0003, AT[2]))
    if name == "translation":
        return cam, build(W, H, look_from=(FROM[0] + 0.9, FROM[1] - 0.5, FROM[2]), look_at=(AT[0] + 0.9, AT[1] - 0.5, AT[2]))
    if name == "rotation":
        return cam, build(W, H, v_up=(0.25, 1, 0), look_at=(AT[0] + 0.05, AT[1], AT[2]))
    if name == "looking-away":
        return cam, build(W, H, look_at=(2 * FROM[0] - AT[0], 2 * FROM[1] - AT[1], 2 * FROM[2] - AT[2]))
    if name == "on-a-point":  # the previous centre IS the reconstructed point of the middle pixel: E == 0 there
        f = frame(cam, "smooth", "cur", FS)
        p = (H // 2) * W + W // 2
        X = reconstructed_point(cam, f["depth"], f["hits"], p)
        prev = build(W, H, look_from=X, look_at=FROM)
        assert tuple(prev.center) == X
        return cam, prev
    shift = {"out-left": (0.35, 0), "out-right": (-0.35, 0), "out-top": (0, -0.2), "out-bottom": (0, 0.2)}
    if name in shift:  # the previous camera pans so that part of the image reprojects outside on one side
        dx, dy = shift[name]
        return cam, build(W, H, look_at=(AT[0] + dx * 2.5, AT[1] + dy * 2.5, AT[2]))
    raise KeyError(name)


PAIRS = ["identical", "subpixel-pan", "translation", "rotation", "looking-away", "on-a-point", "out-left", "out-right",
         "out-top", "out-bottom"]


class Frames:
    """Both frames on the device, and the call."""

    def __init__(self, cam, cur, cam_prev, prev):
        self.cam, self.cam_prev = cam, cam_prev
        self.W, self.H = cam.image_width, cam.image_height
        self.host = {"cur": cur, "prev": prev}
        self.t = {w: {k: self._up(k, v) for k, v in f.items() if k != "feature_samples"}
                  for w, f in self.host.items()}
        self.before = {w: {k: v.clone() for k, v in f.items()} for w, f in self.t.items()}

    @staticmethod
    def _up(k, v):
        if k in ("counts", "hits"):
            v = np.asarray(v).astype(np.uint32).view(np.int32)  # u32 on the device
        return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)

    def ptrs(self, which, skip=()):
        d = {k: (None if k in skip else v.data_ptr()) for k, v in self.t[which].items()}
        d["feature_samples"] = self.host[which]["feature_samples"]
        return d

    def reset(self):
        for k, v in self.t["cur"].items():
            v.copy_(self.before["cur"][k])

    def run(self, r, params=None, skip=(), history=True, stream_ptr=None):
        """One call on fresh copies of the current frame; returns (accum, m2, counts, history) host arrays."""
        self.reset()
        P = self.W * self.H
        hist = torch.full((P,), 0x5a5a5a5a, dtype=torch.int32, device=DEV) if history else None
        torch.cuda.synchronize()
        r.temporal_accumulate(self.cam, self.ptrs("cur", skip), self.cam_prev, self.ptrs("prev", skip), params=params,
                              d_history_ptr=hist.data_ptr() if history else None, stream_ptr=stream_ptr)
        torch.cuda.synchronize()
        c = self.t["cur"]
        return (c["accum"].cpu().numpy(), c["m2"].cpu().numpy(), c["counts"].cpu().numpy().view(np.uint32).astype(np.int64),
                hist.cpu().numpy().view(np.uint32).astype(np.int64) if history else None)

    def ref(self, skip=(), **params):
        f = {w: {k: (None if k in skip else v) for k, v in d.items()} for w, d in self.host.items()}
        return temporal_ref.accumulate(self.W, self.H, self.cam, f["cur"], self.cam_prev, f["prev"], **params)

    def prev_unchanged(self):
        return all(torch.equal(v.view(torch.uint8), self.before["prev"][k].view(torch.uint8))
                   for k, v in self.t["prev"].items())

    def cur_unchanged(self):
        return all(torch.equal(v.view(torch.uint8), self.before["cur"][k].view(torch.uint8))
                   for k, v in self.t["cur"].items())


@pytest.fixture(scope="module")
def rend(module_renderers):
    return module_renderers()


# ---- the kernel against its definition -----------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_bits_against_numpy(rend, shape, pair):
    W, H = shape
    cam, cam_prev = camera_pair(pair, W, H)
    taken = 0
    for pattern in PATTERNS:
        fr = Frames(cam, frame(cam, pattern, "cur", FS), cam_prev, frame(cam_prev, pattern, "prev", FS_PREV))
        for prm in ({}, dict(max_history=1), dict(max_history=20, sigma_z=0.002, tau_n=1e-4, tau_a=1e-5, tau_h=0.3,
                                                  min_weight=0.9)):
            want = fr.ref(**prm)
            got = fr.run(rend, rtzig.temporal_params(**prm))
            assert same_bits(got, want), (pattern, shape, pair, prm)
            taken += int((want[3] > 0).sum())
        assert fr.prev_unchanged()
    if pair in ("identical", "subpixel-pan"):
        assert taken > 0
    if pair == "looking-away":
        assert taken == 0


def test_the_cases_reach_what_they_are_for():
    """Checked on the reference, at 70 x 45: the projection exits ('looking-away': nothing in front; the
    four 'out-' pairs: some pixels out of range on the named side and some in range; 'on-a-point': E == 0
    at the middle pixel), 'smooth' takes history at most pixels, 'random' at few, and the history counts
    reach every clamp."""
    W, H = 70, 45
    cam = build(W, H)
    f = frame(cam, "smooth", "cur", FS)
    sides = {"left": lambda u, v: u < -1, "right": lambda u, v: u >= W, "top": lambda u, v: v < -1,
             "bottom": lambda u, v: v >= H}
    reached = set()
    for pair in PAIRS:
        cam, cam_prev = camera_pair(pair, W, H)
        front, in_range, u, v, r = temporal_ref.project(W, H, cam, f["depth"], f["hits"], cam_prev)
        if pair == "looking-away":
            assert not front.any()
        elif pair == "on-a-point":
            p = (H // 2) * W + W // 2
            assert r[p] == 0 and not front[p] and front.sum() > 0
        else:
            assert front.all()
        if pair.startswith("out-"):
            assert in_range.any() and not in_range.all(), pair
            for name, test in sides.items():
                out = test(u, v)
                assert not in_range[out].any()
                if out.any():
                    reached.add(name)
        if pair == "identical":
            jj, ii = np.divmod(np.arange(W * H), W)
            assert np.abs(u - ii).max() < 1e-9 and np.abs(v - jj).max() < 1e-9
    assert reached == set(sides)
    cam, cam_prev = camera_pair("subpixel-pan", W, H)
    frac = {}
    for pattern in ("smooth", "random"):
        h = temporal_ref.accumulate(W, H, cam, frame(cam, pattern, "cur", FS), cam_prev,
                                    frame(cam_prev, pattern, "prev", FS_PREV))[3]
        frac[pattern] = float((h > 0).mean())
    assert frac["smooth"] > 0.9 and frac["random"] < 0.2, frac
    h = temporal_ref.accumulate(W, H, cam, frame(cam, "counts", "cur", FS), cam_prev, frame(cam_prev, "counts", "prev", FS_PREV))[3]
    assert {1, 2, 3, 16, 40, 64} <= set(np.unique(h))  # nmin below, max_history at and below the tap counts
    h = temporal_ref.accumulate(W, H, cam, frame(cam, "cur-full", "cur", FS), cam_prev,
                                frame(cam_prev, "cur-full", "prev", FS_PREV))[3]
    assert set(np.unique(h)) == {0, 2}  # room for 2 at counts 2^32 - 3, for none at 2^32 - 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_exact_integer_coordinates_skip_the_zero_weight_taps(rend, shape):
    """On the dyadic lattice camera u is an exact integer (fx == 0), and with the previous pixel0 moved a
    quarter pixel along dv, v = j - 0.25 exactly: the taps at a = 1 have bw == 0 and must be skipped — with
    uneven previous counts a tap that was not skipped would lower nmin."""
    W, H = shape
    cam = lattice_camera(W, H)
    prev_cam = copy_cam(cam)
    for k in range(3):
        prev_cam.pixel0[k] = cam.pixel0[k] + 0.25 * cam.dv[k]
    P = W * H
    rng = np.random.default_rng(W * 100 + H)
    cur, prev = frame(cam, "smooth", "cur", 4), frame(prev_cam, "smooth", "prev", 8)
    cur["depth"], prev["depth"] = lattice_depth(cam) * 4, lattice_depth(prev_cam) * 8
    prev["counts"] = rng.integers(1, 200, P)
    wide = dict(sigma_z=0.5, tau_n=10.0, tau_a=10.0, tau_h=10.0, min_weight=0.25, max_history=1000)
    front, in_range, u, v, _ = temporal_ref.project(W, H, cam, cur["depth"], cur["hits"], prev_cam)
    jj, ii = np.divmod(np.arange(P), W)
    assert front.all() and in_range.all() and np.array_equal(u, ii) and np.array_equal(v, jj - 0.25)
    fr = Frames(cam, cur, prev_cam, prev)
    want = fr.ref(**wide)
    got = fr.run(rend, rtzig.temporal_params(**wide))
    assert same_bits(got, want)
    # independent of the reference: the taps are (i, j - 1) at weight 0.25 and (i, j) at 0.75, nothing else
    cnt = prev["counts"].reshape(H, W)
    up = np.vstack([np.full((1, W), 2 ** 40), cnt[:-1]])  # row -1 is outside the image
    assert np.array_equal(got[3].reshape(H, W), np.minimum(cnt, up))


@pytest.mark.parametrize("skip", [("albedo",), ("normal",), ("albedo", "normal")], ids=["no-albedo", "no-normal", "neither"])
def test_null_guides(rend, skip):
    """A guide that is NULL (in both frames) contributes no test."""
    W, H = 37, 23
    cam, cam_prev = camera_pair("subpixel-pan", W, H)
    fr = Frames(cam, frame(cam, "random", "cur", FS), cam_prev, frame(cam_prev, "random", "prev", FS_PREV))
    prm = dict(sigma_z=1.0)  # the random depths pass: the guide tests decide
    want = fr.ref(skip=skip, **prm)
    assert same_bits(fr.run(rend, rtzig.temporal_params(**prm), skip=skip), want)
    full = fr.ref(**prm)
    assert (want[3] > 0).sum() > (full[3] > 0).sum()  # the guide that left did refuse taps
    if len(skip) == 2:
        assert (want[3] > 0).mean() > 0.9


# ---- properties with exact expectations ------------------------------------------------------------------
def test_no_previous_samples_leaves_everything_alone(rend):
    W, H = 70, 45
    cam, cam_prev = camera_pair("subpixel-pan", W, H)
    prev = frame(cam_prev, "smooth", "prev", FS_PREV)
    prev["counts"] = np.zeros(W * H, np.int64)
    fr = Frames(cam, frame(cam, "cur-empty", "cur", FS), cam_prev, prev)
    got = fr.run(rend)
    assert (got[3] == 0).all() and fr.cur_unchanged() and fr.prev_unchanged()
    got = fr.run(rend, history=False)  # d_history is optional
    assert got[3] is None and fr.cur_unchanged()


def test_default_params_determinism_and_no_history_buffer(rend):
    W, H = 70, 45
    cam, cam_prev = camera_pair("translation", W, H)
    fr = Frames(cam, frame(cam, "counts", "cur", FS), cam_prev, frame(cam_prev, "counts", "prev", FS_PREV))
    want = fr.ref()
    a = fr.run(rend)  # params None: the defaults
    b = fr.run(rend)
    assert same_bits(a, want) and same_bits(b, a)
    c = fr.run(rend, history=False)
    assert same_bits(c[:3], want[:3])
    assert 0 < (want[3] > 0).sum() < W * H and fr.prev_unchanged()
    # pixels without history: not one byte written (the call ran on the poisoned copy above as well)
    untouched = want[3] == 0
    assert np.array_equal(bits(a[0])[untouched], bits(fr.host["cur"]["accum"])[untouched])


def test_other_stream_and_timing(rend):
    """Asynchronous on the caller's stream; the context's events report the call as the sample kernel."""
    W, H = 70, 45
    cam, cam_prev = camera_pair("rotation", W, H)
    fr = Frames(cam, frame(cam, "smooth", "cur", FS), cam_prev, frame(cam_prev, "smooth", "prev", FS_PREV))
    want = fr.ref()
    s = torch.cuda.Stream()
    rend.enable_timing(True)
    try:
        got = fr.run(rend, stream_ptr=s.cuda_stream)
        sample_ms, reduce_ms = rend.kernel_times()
    finally:
        rend.enable_timing(False)
    assert sample_ms > 0 and reduce_ms < 0.05 * sample_ms + 0.01
    assert same_bits(got, want)
    assert rend.kernel_name() == "temporal_accumulate"


def test_argument_errors_with_a_live_context_leave_the_buffers_alone(rend):
    W, H = 37, 23
    cam, cam_prev = camera_pair("subpixel-pan", W, H)
    fr = Frames(cam, frame(cam, "smooth", "cur", FS), cam_prev, frame(cam_prev, "smooth", "prev", FS_PREV))
    cur, prev = fr.ptrs("cur"), fr.ptrs("prev")
    other = build(W + 1, H)
    flat = copy_cam(cam_prev)
    for k in range(3):
        flat.dv[k] = flat.du[k]  # du x dv == 0
    for args, kw, word in (((cam, dict(cur, accum=None), cam_prev, prev), {}, "accumulator"),
                           ((cam, cur, cam_prev, dict(prev, hits=None)), {}, "hits"),
                           ((cam, dict(cur, albedo=None), cam_prev, prev), {}, "albedo"),
                           ((cam, cur, cam_prev, dict(prev, feature_samples=0)), {}, "feature_samples"),
                           ((other, cur, cam_prev, prev), {}, "image sizes"),
                           ((cam, cur, flat, prev), {}, "nn"),
                           ((cam, cur, cam_prev, dict(prev, m2=cur["m2"])), {}, "share"),
                           ((cam, cur, cam_prev, prev), dict(params=rtzig.temporal_params(max_history=0)), "max_history"),
                           ((cam, cur, cam_prev, prev), dict(params=rtzig.temporal_params(min_weight=0.0)), "min_weight")):
        with pytest.raises(rtzig.RtError) as e:
            rend.temporal_accumulate(*args, **kw)
        assert e.value.code == -1 and word in str(e.value), word
    torch.cuda.synchronize()
    assert fr.cur_unchanged() and fr.prev_unchanged()


def test_pixel_convention(rend):
    """Independent of the numpy file: identical cameras, smooth buffers, current counts 0 and wide
    tolerances.  Every hit pixel then takes min(counts'[p], max_history) pseudo-samples (the previous counts
    are even: u is i only to some 1e-14, and the neighbour tap that weight brings in counts for nmin) and its merged mean
    is the previous mean at the SAME pixel to 1e-9 relative (rounding moves u by some 1e-14 of a pixel; an
    off-by-half or a swapped axis moves the mean by the image's gradient)."""
    W, H = 70, 45
    cam, cam_prev = camera_pair("identical", W, H)
    P = W * H
    rng = np.random.default_rng(5)
    prev = frame(cam_prev, "hits-zero", "prev", FS_PREV)
    cur = frame(cam, "hits-zero", "cur", FS)
    prev["hits"] = np.maximum(prev["hits"], 1)  # every previous pixel saw a surface
    X, dist = hit_points(cam)
    prev["depth"] = dist * prev["hits"]
    prev["counts"] = np.full(P, 24, np.int64)  # even: a neighbour tap of weight 1e-14 must not lower nmin
    prev["accum"] = shade(X)[0] * prev["counts"][:, None]
    cur["counts"] = np.zeros(P, np.int64)
    cur["accum"][:], cur["m2"][:] = np.nan, np.nan
    fr = Frames(cam, cur, cam_prev, prev)
    hit = cur["hits"] > 0
    assert 0 < hit.sum() < P
    for cap in (64, 16):
        wide = dict(sigma_z=0.5, tau_n=10.0, tau_a=10.0, tau_h=10.0, min_weight=0.25, max_history=cap)
        accum, m2, counts, hist = fr.run(rend, rtzig.temporal_params(**wide))
        assert np.array_equal(hist, np.where(hit, np.minimum(prev["counts"], cap), 0)) and np.array_equal(counts, hist)
        mean = accum[hit] / counts[hit][:, None]
        want = prev["accum"][hit] / prev["counts"][hit][:, None]
        assert np.abs(mean / want - 1).max() < 1e-9
        m2_mean, m2_want = m2[hit] / counts[hit], prev["m2"][hit] / prev["counts"][hit]
        assert np.abs(m2_mean / m2_want - 1).max() < 1e-9
    assert np.isnan(accum[~hit]).all() and np.isnan(m2[~hit]).all()  # not written


# ---- end to end: render_sequence on 96 x 54 images -------------------------------------------------------
def yardstick(cam, world):
    """A 2048-spp one-pass render of `cam` with a seed of its own."""
    c = copy_cam(cam)
    c.samples_per_pixel, c.pixel_samples_scale = 2048, 1.0 / 2048
    c.seed = 0x5EED0F175E1F
    return rtzig.render(c, world, n_gpus=1)


def last_frames(cams, world, spp):
    """The last frame of render_sequence with the temporal pass and without it."""
    out = {}
    for key, temporal in (("on", None), ("off", False)):
        frames = list(rtzig.render_sequence(cams, world, spp, temporal=temporal))
        assert len(frames) == len(cams)
        out[key] = frames
    return out


def test_sequence_static_camera():
    cam = rtzig.chapter13_camera(width=96, aspect_ratio=16 / 9, spp=1)
    world = cam.scene.world
    W, H = cam.width, cam.height
    seq = last_frames([cam.cam] * 4, world, 4)
    R = yardstick(cam.cam, world)
    on, off = seq["on"], seq["off"]
    for f in on + off:
        assert f["image"].shape == (H, W, 3) and f["noisy"].shape == (H, W, 3) and f["variance"].shape == (H, W)
        assert f["counts"].dtype == np.uint32 and f["history"].dtype == np.uint32
    assert all((f["history"] == 0).all() and (f["counts"] == 4).all() for f in off)
    assert (on[0]["history"] == 0).all() and same_bits([on[0]["image"], on[0]["noisy"]],
                                                       [off[0]["image"], off[0]["noisy"]])
    # frames differ in their seeds: the baseline's frames are four different renders
    assert not np.array_equal(off[0]["noisy"], off[1]["noisy"])
    # the first frame is the one-pass render at its counts and seed
    c = copy_cam(cam.cam)
    c.samples_per_pixel, c.pixel_samples_scale = 4, 0.25
    assert same_bits([on[0]["noisy"]], [rtzig.render(c, world, n_gpus=1)])
    assert np.array_equal(on[3]["counts"], on[3]["history"] + 4)
    assert on[3]["history"].max() == 12  # three frames of 4 behind it, below max_history
    e_on, e_off = rmse(on[3]["image"], R), rmse(off[3]["image"], R)
    print(f"static chapter 13, frame 4 of 4 at 4 spp, denoised RMSE vs 2048 spp: temporal {e_on:.5f}, off {e_off:.5f}; "
          f"noisy: temporal {rmse(on[3]['noisy'], R):.5f}, off {rmse(off[3]['noisy'], R):.5f}")
    assert e_on < e_off


def lambertian_path(n_frames):
    """A ground sphere and three spheres, Lambertian only (the outgoing radiance does not depend on the
    view, so reprojected history is unbiased), and a camera that moves about one pixel per frame."""
    scene = rtzig.Scene.init(0xC0FFEE)
    scene.add((0, -100.5, -1), 100, rtzig.RT_LAMBERTIAN, albedo=(0.5, 0.6, 0.4))
    scene.add((0, 0, -1), 0.5, rtzig.RT_LAMBERTIAN, albedo=(0.7, 0.3, 0.3))
    scene.add((-1.1, 0, -1.3), 0.5, rtzig.RT_LAMBERTIAN, albedo=(0.3, 0.4, 0.8))
    scene.add((1.0, -0.2, -0.6), 0.3, rtzig.RT_LAMBERTIAN, albedo=(0.8, 0.7, 0.2))
    cams = []
    for f in range(n_frames):
        # 96 pixels span about 2 * 3 * tan(20 deg) = 2.2 units at the spheres' distance: 0.023 units per pixel
        x = 0.023 * f
        cams.append(rtzig.Camera.builder(96, 16 / 9).setScene(scene).setViewport((x, 0.6, 2.0), (x, 0.0, -1.0), 40)
                    .setSamplesPerPixel(1).build().cam)
    return cams, scene.world


def test_sequence_moving_camera_lambertian():
    cams, world = lambertian_path(6)
    seq = last_frames(cams, world, 4)
    R = yardstick(cams[-1], world)
    on, off = seq["on"][-1], seq["off"][-1]
    last = copy_cam(cams[-1])
    last.seed = cams[-1].seed + 5  # the sequence's seed of frame 5
    feat = rtzig.render_features(last, world, 4)
    hit = feat["hits"] > 0
    taken = float((on["history"][hit] > 0).mean())
    e_on, e_off = rmse(on["image"], R), rmse(off["image"], R)
    print(f"moving Lambertian, frame 6 of 6 at 4 spp, denoised RMSE vs 2048 spp: temporal {e_on:.5f}, off {e_off:.5f}; "
          f"hit pixels with history {taken:.3f}")
    assert (on["history"][~hit] == 0).all()
    assert taken > 0.5
    assert e_on < e_off

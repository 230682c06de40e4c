"""What the GPU tests share: the renderer factory fixtures, the bit comparisons, the 37-wide final
scene with its oracle B reference, the device buffer holders and the CPU reference implementations
that more than one test file relies on.  A helper module, not a test: pytest does not rewrite its
asserts, so every assert here carries its own message."""
import math

import numpy as np
import pytest
import torch

import rtzig
from rtzig.abi import RT_DIELECTRIC

DEV = "cuda:0"


# ---- renderer factories --------------------------------------------------------------------------------
def _renderers():
    """Yields make(world=None, precision="f64", profile=False, timing=False): a DeviceRenderer on GPU 0
    with the scene set (a camera object stands for its scene's world), then precision, profile, timing.
    Tests close their renderers themselves (close() reports a failure the kernel recorded); whatever a
    failing test left open is closed here, newest first, so no context outlives its test or module."""
    made = []

    def make(world=None, precision="f64", profile=False, timing=False):
        r = rtzig.DeviceRenderer(0)
        made.append(r)
        if world is not None:
            r.set_scene(world.scene.world if hasattr(world, "scene") else world)
        r.set_precision(precision)
        if profile:
            r.enable_profile(True)
        if timing:
            r.enable_timing(True)
        return r

    yield make
    errors = []
    for r in reversed(made):
        try:
            r.close()  # a no-op on a renderer the test closed
        except Exception as e:  # close the rest before reporting
            errors.append(e)
    if errors:
        raise errors[0]


renderers = pytest.fixture(_renderers)
module_renderers = pytest.fixture(scope="module")(_renderers)


# ---- comparisons ---------------------------------------------------------------------------------------
def bits(a):
    """An f64 array as int64 (a NaN-safe comparison of bits); any other array as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(got, want):
    """Equal shapes and equal bits, of two arrays or of two tuples of arrays taken pairwise."""
    if isinstance(got, np.ndarray):
        got, want = (got,), (want,)
    return all(g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))


def box_rmse(a, b):
    box = lambda x: x[:224].reshape(28, 8, 50, 8, 3).astype(np.float64).mean(axis=(1, 3))
    return float(np.sqrt(((box(a) - box(b)) ** 2).mean()))


def i32(x):
    """The int32 with the bits of the uint32 x (torch has no uint32 arithmetic; the device reads u32)."""
    return int(np.array(x, np.uint32).view(np.int32))


_CACHE = {}


def cached(key, make):
    """A camera, a ray set or a reference, computed once per session and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the 37-wide final scene ---------------------------------------------------------------------------
W37, H37, NPIX37 = 37, 20, 740  # 740 pixels: a partial last group of 64, a partial last tile


def cam37(spp=1):
    return rtzig.final_scene_camera(width=W37, aspect_ratio=16 / 9, spp=spp)


def ref37(oracle, n):
    """Oracle B's read-only (20, 37, 3) image and rays of the 37-wide scene at spp = n (computed once
    per n)."""
    def render():
        cam = cam37(n)
        img, rays = oracle.render_b(cam.cam, cam.scene.world, threads=16)
        img.setflags(write=False)
        return img, rays
    return cached(("ref37", n), render)


# ---- device buffer holders -----------------------------------------------------------------------------
class Buffers:
    """The four device buffers of P pixels, optionally pre-filled with NaN / 0xFFFFFFFF."""

    def __init__(self, P, poison=False):
        self.albedo = torch.empty((P, 3), dtype=torch.float64, device=DEV)
        self.normal = torch.empty((P, 3), dtype=torch.float64, device=DEV)
        self.depth = torch.empty(P, dtype=torch.float64, device=DEV)
        self.hits = torch.empty(P, dtype=torch.int32, device=DEV)  # u32 on the device
        if poison:
            for t in (self.albedo, self.normal, self.depth):
                t.fill_(float("nan"))
            self.hits.fill_(-1)

    def ptrs(self):
        return dict(d_albedo_ptr=self.albedo.data_ptr(), d_normal_ptr=self.normal.data_ptr(),
                    d_depth_ptr=self.depth.data_ptr(), d_hits_ptr=self.hits.data_ptr())

    def host(self):
        torch.cuda.synchronize()
        return (self.albedo.cpu().numpy(), self.normal.cpu().numpy(), self.depth.cpu().numpy(),
                self.hits.cpu().numpy().view(np.uint32))


class Bufs:
    """The caller's buffers of one image: sums, squared-luminance sums, counts, stats."""

    def __init__(self, n=NPIX37, fill=None, m2=True):
        self.n = n
        self.accum = torch.empty((n, 3), dtype=torch.float64, device=DEV)
        self.m2 = torch.empty(n, dtype=torch.float64, device=DEV) if m2 else None
        if fill is not None:
            self.accum.fill_(fill)
            if m2:
                self.m2.fill_(fill)
        self.counts = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.stats = torch.zeros(2, dtype=torch.int64, device=DEV)

    def add(self, r, cam, pixels, count, **kw):
        r.accumulate_pixels(cam.cam, pixels, count, self.accum.data_ptr(),
                            self.m2.data_ptr() if self.m2 is not None else None, self.counts.data_ptr(),
                            d_stats_ptr=self.stats.data_ptr(), **kw)

    def bits(self):
        """(accum, m2, counts) on the host as integers: NaN-safe bit comparisons."""
        torch.cuda.synchronize()
        m2 = self.m2.cpu().numpy().view(np.int64) if self.m2 is not None else None
        return self.accum.cpu().numpy().view(np.int64), m2, self.counts.cpu().numpy()

    def resolved(self, r, output="linear"):
        out = torch.empty((self.n, 3), dtype=torch.float64 if output == "linear" else torch.uint8, device=DEV)
        r.resolve_counts(self.accum.data_ptr(), self.counts.data_ptr(), self.n, out.data_ptr(), output=output)
        return out.cpu().numpy()


# ---- the selection rule and its inputs --------------------------------------------------
SEL_BLOCK = 1024  # rtk::kSelBlock, the selection kernels' block size
MIN_C, MAX_C, TOL, FLOOR = 4, 32, 0.1, 0.01


def list_a():
    """Pixels 0, 63, 64, 739 (the ends of the first group of 64, the start of the second, the last
    pixel) plus every third pixel, shuffled.  Every third pixel from 2 on shares none of the four, so
    the list has 246 + 4 = 250 pairwise distinct entries (the contract asks for distinct indices)."""
    a = np.array(sorted({0, 63, 64, 739} | set(range(2, NPIX37, 3))))
    assert len(a) == 250, "list A has %d entries, not 250" % len(a)
    return np.random.default_rng(1).permutation(a)


def list_b():
    """Half overlaps A: every other entry of A plus as many pixels outside A, shuffled."""
    a = np.sort(list_a())
    outside = np.setdiff1d(np.arange(NPIX37), a)
    b = np.concatenate([a[::2], outside[::3][:125]])
    assert len(b) == 250 and len(np.intersect1d(a, b)) == 125, \
        "list B has %d entries, %d of them in A (250 and 125 wanted)" % (len(b), len(np.intersect1d(a, b)))
    return np.random.default_rng(2).permutation(b)


def unchanged_outside(before, after, listed):
    mask = np.ones(NPIX37, bool)
    mask[listed] = False
    for name, x, y in zip(("accum", "m2", "counts"), before, after):
        assert np.array_equal(x[mask], y[mask]), \
            "%s: %d elements of unlisted pixels changed" % (name, int((x[mask] != y[mask]).sum()))


def synthetic(pattern, n):
    """(accum (n, 3), m2 (n), counts (n)) on the host.  'quiet' pixels have every sample at luminance
    0.6 (v rounds to about 0), 'noisy' ones a variance of at least mean^2 (err >= sqrt(1 / 39) > TOL)."""
    rng = np.random.default_rng(n * 31 + len(pattern))
    counts = np.full(n, 16, np.int64)
    noisy = np.zeros(n, bool)
    if pattern == "all":
        counts[:] = 2
    elif pattern == "alternating":
        noisy[::2] = True
    elif pattern == "single-last":
        noisy[-1] = True
    elif pattern == "below-min":
        counts = rng.integers(0, 8, n)
    elif pattern == "at-max":
        noisy[:] = True
        counts = rng.choice([31, 32, 40], n)
    elif pattern == "random":
        noisy = rng.random(n) < 0.5
        counts = rng.integers(0, 40, n)
    c = counts.astype(np.float64)
    accum = np.stack([0.1 * c, 0.2 * c, 0.3 * c], 1) * (1 + rng.random((n, 1)))
    S = (accum[:, 0] + accum[:, 1]) + accum[:, 2]
    mean = S / np.maximum(c, 1)
    m2 = S * mean * np.where(noisy, 2.0 + rng.random(n) * 5, 1.0)
    if pattern == "v-negative":
        m2 = S * mean * (1 - 1e-12)  # v = m2 - S * mean < 0: clamped to 0
    if pattern == "nan-m2":
        m2[::3] = np.nan
        counts[::5] = MAX_C  # a NaN error samples on until max_count, not beyond
    if pattern == "random":
        m2[rng.random(n) < 0.1] = np.nan
        accum[rng.random(n) < 0.1] = 0.0  # mean 0: the floor divides
    return accum, m2, counts


def select_numpy(accum, m2, counts, min_c=MIN_C, max_c=MAX_C, tol=TOL, floor=FLOOR):
    with np.errstate(all="ignore"):
        n = counts.astype(np.float64)
        S = (accum[:, 0] + accum[:, 1]) + accum[:, 2]
        mean = S / n
        v = m2 - S * mean
        v = np.where(v < 0, 0.0, v)
        sem = np.sqrt((v / (n - 1)) / n)
        err = sem / np.where(mean > floor, mean, floor)
        err = np.where(counts < 2, 0.0, err)
        sel = (counts < min_c) | ((counts < max_c) & ~(err <= tol))
    return np.flatnonzero(sel), err


# ---- the feature reference --------------------------------------------------------------
MAX_DRAWS = 64  # 2 sampleSquare draws + 31 rejection trips: more is a test bug (p < 1e-20)


def get_ray(cam, i, j, u):
    """getRay (camera.zig:187-215) from the draws u of one sample's stream: (origin, direction)."""
    ox = u[0] - 0.5
    oy = u[1] - 0.5
    fi, fj = float(i) + ox, float(j) + oy
    ps = [(cam.pixel0[c] + cam.du[c] * fi) + cam.dv[c] * fj for c in range(3)]
    if cam.defocus_angle <= 0:
        origin = [cam.center[c] for c in range(3)]
    else:
        k = 2
        while True:
            assert k + 2 <= MAX_DRAWS, "more than 31 rejection trips: a test bug"
            x = -1.0 + 2.0 * u[k]      # rdr(-1, 1) = -1 + (1 - -1) * u
            y = -1.0 + 2.0 * u[k + 1]
            k += 2
            if x * x + y * y < 1:
                break
        origin = [(cam.center[c] + cam.defocus_disk_u[c] * x) + cam.defocus_disk_v[c] * y for c in range(3)]
    return origin, [ps[c] - origin[c] for c in range(3)]


def add_sample(oracle, cam, spheres, s, alb, nrm, dep, hits):
    """Adds sample s of every pixel, in place, to the four sums (albedo (H*W, 3), normal (H*W, 3),
    depth (H*W), hits (H*W) u32)."""
    W, H = cam.image_width, cam.image_height
    for p in range(H * W):
        j, i = divmod(p, W)
        u = [float(x) for x in oracle.random_doubles(oracle.sample_key(cam.seed, p, s), MAX_DRAWS)]
        orig, d = get_ray(cam, i, j, u)
        k, t = oracle.world_hit(spheres, orig, d, cam.t_min, cam.t_max)
        if k < 0:
            continue  # a miss contributes exactly nothing
        sp = spheres[k]
        rec = oracle.sphere_hit(sp, orig, d, cam.t_min, cam.t_max)
        assert rec is not None and rec["t"] == t, \
            "pixel %d, sample %d: sphere_hit of the winning sphere %d gives %r, world_hit t = %r" % (p, s, k, rec, t)
        a = (1.0, 1.0, 1.0) if sp.material == RT_DIELECTRIC else tuple(sp.albedo)
        depth = t * math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        for c in range(3):
            alb[p, c] = alb[p, c] + a[c]
            nrm[p, c] = nrm[p, c] + rec["normal"][c]
        dep[p] = dep[p] + depth
        hits[p] += 1


def reference(oracle, cam, spheres, n_samples):
    """Prefix sums: ref[n] = (albedo (H*W, 3), normal (H*W, 3), depth (H*W), hits (H*W) u32) after
    samples [0, n), for n = 0..n_samples."""
    W, H = cam.image_width, cam.image_height
    alb, nrm = np.zeros((H * W, 3)), np.zeros((H * W, 3))
    dep, hits = np.zeros(H * W), np.zeros(H * W, np.uint32)
    ref = [(alb.copy(), nrm.copy(), dep.copy(), hits.copy())]
    for s in range(n_samples):
        add_sample(oracle, cam, spheres, s, alb, nrm, dep, hits)
        ref.append((alb.copy(), nrm.copy(), dep.copy(), hits.copy()))
    return ref


def assert_equal(got, want, what=""):
    for name, g, w in zip(("albedo", "normal", "depth", "hits"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, int((g != w).sum()))

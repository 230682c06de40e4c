"""What the slab-certificate tests share: the skimming rays, a numpy model of the BVH walk's f32 slab test
and per-sphere boxes at a chosen share of the builder's pad.  A helper module, not a test: pytest does not
rewrite its asserts, so every assert here carries its own message.

BvhWalker::descend (csrc/rt_kernel.hip) decides in f32 whether a child box can be skipped; that it never
skips a box holding the closest hit rests on the "Padding rules" of csrc/rt_bvh.cpp.  A skimming ray is
the ray that argument is tightest for: it passes within a few f32 ulps under a sphere's axis-aligned pole,
nearly parallel to the box face the pole touches, so the hit exists only inside the pad.

The model (slab_keeps) is the arithmetic of run_f64 and descend restated in numpy, every f32 rounding in
its place.  tests/test_slab_inputs.py uses it for the control alone: that these rays, on boxes without
the pad, do lose hits.  What the device does is tested on the device (tests/test_gpu_slab.py)."""
import math

import numpy as np

INF = math.inf
F32 = np.float32
CLAMP = F32(1e30)
VARIANT_SHARE = 16  # one ray in 16 of each d_a variant: 0, 2^-140 (an f32 denormal), 2^-160 (0 in f32)


# ---- spheres as arrays ---------------------------------------------------------------------------------
def centres_radii(spheres):
    """(centres (n, 3), radii (n,)) of an RtSphere array; the radius clamped at 0 as Sphere.init does."""
    c = np.array([list(s.center) for s in spheres], np.float64).reshape(-1, 3)
    r = np.array([max(0.0, s.radius) for s in spheres], np.float64)
    return c, r


def extent(spheres):
    """rtbvh::scene_extent: max |coordinate| of any sphere's box."""
    c, r = centres_radii(spheres)
    return float((np.abs(c) + r[:, None]).max())


def bound_needed(spheres, O):
    """The origin bound a tree needs for these origins: the scene's extent (every tree has that) or the
    largest |coordinate| of an origin.  The GPU tests reserve it where the context's own bound is short."""
    return max(extent(spheres), float(np.abs(O).max()))


def ulp32(x):
    """The spacing of f32 at |x|, as f64."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


# ---- the rays ------------------------------------------------------------------------------------------
def skimming_rays(spheres, n, rng, depth_log2=(-3, 3), tilt_log2=(-40, -12), reach=(1, 8)):
    """(O, D), each (n, 3) f64.  Ray q picks a sphere k with r > 0, an axis a, a sign s and a travel axis
    b != a (c: the third).  With face = c_a + s r and delta = ulp_f32(|face|) 2^U(depth_log2), it passes
    through the sphere's centre moved to face - s delta on axis a — a point delta under the pole — along
    d_b = +-1, d_a = +-2^U(tilt_log2), d_c = 1e-3 U(-1, 1), and starts L = U(reach) before that point.
    The last three 16ths of the rays have d_a = 0, +-2^-140 and +-2^-160 in turn: the reciprocal's clamp,
    with the origin itself delta under the face.  Deterministic for a generator's state."""
    c, r = centres_radii(spheres)
    real = np.flatnonzero(r > 0)
    assert len(real), "skimming_rays: no sphere with r > 0"
    k = real[rng.integers(0, len(real), n)]
    a = rng.integers(0, 3, n)
    b = (a + rng.integers(1, 3, n)) % 3
    cc = 3 - a - b
    s = rng.choice([-1.0, 1.0], n)
    q = np.arange(n)
    face = c[k, a] + s * r[k]
    delta = ulp32(face) * 2.0 ** rng.uniform(depth_log2[0], depth_log2[1], n)
    target = c[k].copy()
    target[q, a] = face - s * delta
    D = np.zeros((n, 3))
    D[q, b] = rng.choice([-1.0, 1.0], n)
    D[q, a] = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(tilt_log2[0], tilt_log2[1], n)
    D[q, cc] = 1e-3 * rng.uniform(-1, 1, n)
    sign = rng.choice([-1.0, 1.0], n)
    m = n // VARIANT_SHARE
    for v, val in enumerate((0.0, 2.0 ** -140, 2.0 ** -160)):
        sl = slice(n - (3 - v) * m, n - (2 - v) * m)
        D[q[sl], a[sl]] = sign[sl] * val
    L = rng.uniform(reach[0], reach[1], n)
    O = target - L[:, None] * D
    return O, D


def tree_ok(O, D, t_min, origin_bound):
    """rtk::trace_tree_ok (csrc/rt_trace.h) per ray: may the tree of this origin bound answer it?"""
    O, D = np.asarray(O, np.float64), np.asarray(D, np.float64)
    ao, ad = np.abs(O), np.abs(D)
    with np.errstate(invalid="ignore"):
        om, dm = ao.max(axis=1), ad.max(axis=1)  # NaN propagates through max
        dir_ok = (dm >= 2.0 ** -20) & (dm <= 2.0 ** 20)
        org_ok = (om <= origin_bound) & np.isfinite(om)
        tmin_ok = bool(t_min >= 0 and math.isfinite(t_min))
        prod_ok = (ao <= 2.0 ** 126 * np.maximum(ad, 2.0 ** -100)).all(axis=1)
    return dir_ok & org_ok & prod_ok & tmin_ok


# ---- f32 arithmetic, rounding by rounding ----------------------------------------------------------------
def fma32(b, m, a):
    """fmaf(b, m, a) of f32 arrays: one rounding.  The product of two f32 is exact in f64; the sum is
    rounded to odd in f64 (TwoSum gives the residual), which the final rounding to f32 then sees as the
    exact value would be seen (f64 carries more than two bits beyond f32)."""
    b, m, a = (np.asarray(x, F32).astype(np.float64) for x in (b, m, a))
    with np.errstate(invalid="ignore", over="ignore"):
        p = b * m
        s = p + a
        bb = s - p
        err = (p - (s - bb)) + (a - bb)
        inexact = np.isfinite(s) & (err != 0)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        toward = np.where(err > 0, INF, -INF)
        s = np.where(inexact & even, np.nextafter(s, toward), s)
        return s.astype(F32)


def rcp_clamp(d32, rcp_ulps=0):
    """The walk's reciprocal: the correctly rounded f32 1 / d, moved by rcp_ulps f32 neighbours (v_rcp_f32
    is allowed 1 ulp), then clamped to +-1e30 as v_med3 does; 1 / +-0 = +-inf keeps its sign."""
    d32 = np.asarray(d32, F32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = (1.0 / d32.astype(np.float64)).astype(F32)
    for _ in range(abs(rcp_ulps)):
        inv = np.where(np.isfinite(inv), np.nextafter(inv, F32(math.copysign(INF, rcp_ulps))), inv).astype(F32)
    return np.clip(inv, -CLAMP, CLAMP).astype(F32)


def widen(t_min, closest):
    """(lower, upper) in f32 as run_f64 widens them."""
    with np.errstate(over="ignore"):
        lower = np.asarray(t_min, np.float64).astype(F32)
        lower = (lower - np.abs(lower) * F32(2.0 ** -20)).astype(F32) - F32(1e-30)
        upper = np.asarray(closest, np.float64).astype(F32)
        upper = (upper + np.abs(upper) * F32(2.0 ** -20)).astype(F32)
    return lower.astype(F32), upper


def slab_keeps(O, D, lo, hi, t_min, closest, rcp_ulps=0):
    """(n,) bool: does the walk keep the f32 box (lo[q], hi[q]) for ray q whose closest hit so far is
    closest[q]?  run_f64's setup and descend's test: cast, reciprocal and clamp, noi = -(o inv), each
    plane one fma, near and far picked by the sign of inv, NaN dropped by max and min."""
    o = np.asarray(O, np.float64).astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        d = np.asarray(D, np.float64).astype(F32)
    inv = rcp_clamp(d, rcp_ulps)
    with np.errstate(over="ignore", invalid="ignore"):
        noi = -(o * inv).astype(F32)
    lo, hi = np.broadcast_to(np.asarray(lo, F32), o.shape), np.broadcast_to(np.asarray(hi, F32), o.shape)
    t_lo, t_hi = fma32(lo, inv, noi), fma32(hi, inv, noi)
    neg = inv < 0
    near, far = np.where(neg, t_hi, t_lo), np.where(neg, t_lo, t_hi)
    lower, upper = widen(t_min, closest)
    lower, upper = np.broadcast_to(lower, o.shape[:1]), np.broadcast_to(upper, o.shape[:1])
    n = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], lower))
    f = np.fmin(np.fmin(far[:, 0], far[:, 1]), np.fmin(far[:, 2], upper))
    return n <= f


# ---- boxes ---------------------------------------------------------------------------------------------
def round_out(lo, hi):
    """f64 bounds as f32, rounded outward (Builder::down / up)."""
    flo, fhi = lo.astype(F32), hi.astype(F32)
    flo = np.where(flo.astype(np.float64) > lo, np.nextafter(flo, F32(-INF)), flo)
    fhi = np.where(fhi.astype(np.float64) < hi, np.nextafter(fhi, F32(INF)), fhi)
    return flo.astype(F32), fhi.astype(F32)


def tight_boxes(spheres, pad_scale, origin_bound=0.0):
    """(lo, hi), each (n, 3) f32: every sphere's own box padded by pad_scale x the builder's pad
    (2^-17 (|c|_inf + r) + 2^-21 origin_bound + 2^-60, csrc/rt_bvh.cpp), rounded outward."""
    c, r = centres_radii(spheres)
    pad = pad_scale * ((np.abs(c).max(axis=1) + r) * 2.0 ** -17 + origin_bound * 2.0 ** -21 + 2.0 ** -60)
    return round_out(c - (r + pad)[:, None], c + (r + pad)[:, None])


# ---- the reference -------------------------------------------------------------------------------------
def ref_hits(oracle, spheres, O, D, t_min=1e-3, t_max=INF):
    """HittableList.hit of every ray: the dict rt_trace_rays fills (index, t, point, normal, front), from
    oracle.world_hit for the winning sphere and oracle.sphere_hit on it.  Read-only."""
    n = len(O)
    out = dict(index=np.full(n, -1, np.int32), t=np.full(n, INF), point=np.zeros((n, 3)), normal=np.zeros((n, 3)),
               front=np.zeros(n, np.uint8))
    for q in range(n):
        o, d = O[q].tolist(), D[q].tolist()
        k, t = oracle.world_hit(spheres, o, d, t_min, t_max)
        if k < 0:
            continue
        rec = oracle.sphere_hit(spheres[k], o, d, t_min, t_max)
        assert rec is not None and rec["t"] == t, "ray %d: sphere_hit of the winner %d gives %r, world_hit t = %r" % (q, k, rec, t)
        out["index"][q], out["t"][q], out["front"][q] = k, t, rec["front"]
        out["point"][q], out["normal"][q] = rec["point"], rec["normal"]
    for x in out.values():
        x.setflags(write=False)
    return out


# ---- the cases -----------------------------------------------------------------------------------------
N = 4096
LATTICE_T = (0, 64, 1024)
SEED = 20


def case_rays(name, spheres, n=N, **kw):
    """The skimming rays of a named case, the same in every test file (seeded by the name)."""
    rng = np.random.default_rng([SEED, sum(name.encode())])
    O, D = skimming_rays(spheres, n, rng, **kw)
    O.setflags(write=False)
    D.setflags(write=False)
    return O, D

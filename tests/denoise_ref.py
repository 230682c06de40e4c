"""The numpy restatement of rt_denoise (include/rt.h): the bit-level reference of the
GPU filter.  Every step is a whole-array numpy operation over the overlapping slices of a tap, and the
sums grow with `x = x + ...` in tap order (ty outer, tx inner).  Numpy's separate ufunc calls never
fuse into a multiply-add and its f64 `/` and `sqrt` are correctly rounded: that is what makes this a
reference for bits, not for approximate values.  A helper module, not a test."""
import numpy as np

DEFAULTS = dict(levels=2, sigma_l=4.0, sigma_n=32.0, sigma_a=32.0, sigma_z=0.05, sigma_h=4.0, epsilon=1e-6)


def prepare(W, H, accum, m2, counts, albedo=None, normal=None, depth=None, hits=None, feature_samples=0):
    """The prepare pass.  accum (P, 3), m2 (P), counts (P) integers; the guides as rt_render_rows_features
    leaves them (albedo / normal (P, 3), depth (P), hits (P)) or None.  Returns c (H, W, 3), var (H, W)
    and the guides N (H, W, 3), A (H, W, 3), cov (H, W), z (H, W)."""
    P = W * H
    accum = np.asarray(accum, np.float64).reshape(P, 3)
    m2 = np.asarray(m2, np.float64).reshape(P)
    counts = np.asarray(counts).reshape(P).astype(np.int64)
    with np.errstate(all="ignore"):
        n = counts.astype(np.float64)
        scale = 1.0 / n
        c = accum * scale[:, None]
        c = np.where((counts == 0)[:, None], 0.0, c)
        S = (accum[:, 0] + accum[:, 1]) + accum[:, 2]
        mean = S / n
        v = m2 - S * mean
        var = np.where(v > 0, (v / (n - 1)) / n, 0.0)
        var = np.where(counts < 2, 0.0, var)
        fi = np.float64(1.0) / np.float64(feature_samples) if feature_samples else np.float64(0.0)
        zero3, zero1 = np.zeros((P, 3)), np.zeros(P)
        A = np.asarray(albedo, np.float64).reshape(P, 3) * fi if albedo is not None else zero3
        N = np.asarray(normal, np.float64).reshape(P, 3) * fi if normal is not None else zero3
        cov, z = zero1, zero1
        if hits is not None:
            hc = np.asarray(hits).reshape(P).astype(np.int64)
            h = hc.astype(np.float64)
            cov = h * fi
            if depth is not None:
                z = np.where(hc != 0, np.asarray(depth, np.float64).reshape(P) / h, 0.0)
    return (c.reshape(H, W, 3), var.reshape(H, W), N.reshape(H, W, 3), A.reshape(H, W, 3), cov.reshape(H, W),
            z.reshape(H, W))


def _slices(n, d):
    """(destination slice, source slice) of the pixels p in [0, n) whose tap p + d is in [0, n)."""
    lo, hi = max(0, -d), min(n, n - d)
    if lo >= hi:
        return None
    return slice(lo, hi), slice(lo + d, hi + d)


def prefilter(var):
    H, W = var.shape
    G = {-1: 0.25, 0: 0.5, 1: 0.25}
    sv, sg = np.zeros((H, W)), np.zeros((H, W))
    for ty in (-1, 0, 1):
        for tx in (-1, 0, 1):
            ys, xs = _slices(H, ty), _slices(W, tx)
            if ys is None or xs is None:
                continue
            g = G[ty] * G[tx]
            sv[ys[0], xs[0]] = sv[ys[0], xs[0]] + g * var[ys[1], xs[1]]
            sg[ys[0], xs[0]] = sg[ys[0], xs[0]] + g
    return sv / sg


def level(c, v, N, A, cov, z, s, prm):
    """One à-trous level at step s: (c, v) -> (c', v')."""
    H, W = v.shape
    K = {-2: 1, -1: 4, 0: 6, 1: 4, 2: 1}
    eps = prm["epsilon"]
    with np.errstate(all="ignore"):
        lum = (c[..., 0] + c[..., 1]) + c[..., 2]
        isd = 1.0 / (prm["sigma_l"] * np.sqrt(v) + eps)
        sw, sv = np.zeros((H, W)), np.zeros((H, W))
        sc = np.zeros((H, W, 3))
        for ty in range(-2, 3):
            for tx in range(-2, 3):
                ys, xs = _slices(H, ty * s), _slices(W, tx * s)
                if ys is None or xs is None:
                    continue
                p, q = (ys[0], xs[0]), (ys[1], xs[1])
                dl = np.abs(lum[p] - lum[q]) * isd[p]
                e = N[p] - N[q]
                dn = prm["sigma_n"] * ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
                f = A[p] - A[q]
                da = prm["sigma_a"] * ((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2])
                dh = prm["sigma_h"] * np.abs(cov[p] - cov[q])
                r = float(max(abs(tx), abs(ty)) * s)
                if r > 0:
                    dz = np.where((z[p] > 0) & (z[q] > 0),
                                  np.abs(z[p] - z[q]) / ((prm["sigma_z"] * r) * (z[p] + z[q]) + eps), 0.0)
                else:
                    dz = np.zeros_like(dl)
                d = ((dl + dn) + da) + (dh + dz)
                x = 1.0 - d * 0.125
                t = np.where(x > 0, x, 0.0)
                t = t * t
                t = t * t
                t = t * t
                w = t * ((K[ty] * K[tx]) / 256.0)  # the kernel weight is exact
                sw[p] = sw[p] + w
                sc[p] = sc[p] + w[..., None] * c[q]
                sv[p] = sv[p] + (w * w) * v[q]
        rs = 1.0 / sw
        return sc * rs[..., None], sv * (rs * rs)


def denoise(W, H, accum, m2, counts, albedo=None, normal=None, depth=None, hits=None, feature_samples=0, **params):
    """rt_denoise: (image (H, W, 3), variance (H, W)).  params: fields of rt_denoise_params over DEFAULTS."""
    prm = dict(DEFAULTS)
    for k in params:
        if k not in prm:
            raise TypeError(k)
    prm.update(params)
    c, var, N, A, cov, z = prepare(W, H, accum, m2, counts, albedo, normal, depth, hits, feature_samples)
    with np.errstate(all="ignore"):
        v = prefilter(var)
    for k in range(int(prm["levels"])):
        c, v = level(c, v, N, A, cov, z, 1 << k, prm)
    return c, v

"""The numpy restatement of rt_temporal_accumulate (include/rt.h): the bit-level
reference of the GPU kernel.  Every step is a whole-image numpy operation, one ufunc per operation of the
definition, and the sums grow with `x = x + ...` in tap order (b outer, a inner) under a mask.  Numpy's
separate ufunc calls never fuse into a multiply-add and its f64 `/`, `sqrt` and `floor` are correctly
rounded: that is what makes this a reference for bits, not for approximate values.  A helper module, not
a test."""
import numpy as np

DEFAULTS = dict(max_history=64, sigma_z=0.05, tau_n=0.1, tau_a=0.05, tau_h=0.5, min_weight=0.25)
U32_MAX = 2 ** 32 - 1


def dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def camera_vectors(cam):
    """(pixel0, du, dv, center) of an rt_camera as tuples of three np.float64."""
    return tuple(tuple(np.float64(x) for x in getattr(cam, k)) for k in ("pixel0", "du", "dv", "center"))


def per_call(cam_prev):
    """A, n, an, nn, rnn of the previous camera."""
    pixel0, du, dv, center = camera_vectors(cam_prev)
    A = tuple(pixel0[k] - center[k] for k in range(3))
    n = cross(du, dv)
    an = dot(A, n)
    nn = dot(n, n)
    with np.errstate(all="ignore"):
        rnn = np.float64(1.0) / nn
    return A, n, an, nn, rnn


def _frame(W, H, f):
    P = W * H
    g = dict(accum=np.asarray(f["accum"], np.float64).reshape(P, 3), m2=np.asarray(f["m2"], np.float64).reshape(P),
             counts=np.asarray(f["counts"]).reshape(P).astype(np.int64),
             depth=np.asarray(f["depth"], np.float64).reshape(P), hits=np.asarray(f["hits"]).reshape(P).astype(np.int64))
    for k in ("albedo", "normal"):
        g[k] = None if f.get(k) is None else np.asarray(f[k], np.float64).reshape(P, 3)
    g["fi"] = np.float64(1.0) / np.float64(f["feature_samples"])
    return g


def project(W, H, cam, cur_depth, cur_hits, cam_prev):
    """Steps 1-4 for every pixel: (front, in_range, u, v, r), each of shape (P,); front already includes
    hits > 0.  Values at pixels that are not `front` are meaningless."""
    P = W * H
    pixel0, du, dv, center = camera_vectors(cam)
    pc = camera_vectors(cam_prev)[3]
    _, pdu, pdv, _ = camera_vectors(cam_prev)
    A, n, an, nn, rnn = per_call(cam_prev)
    jj, ii = np.divmod(np.arange(P, dtype=np.int64), W)
    di, dj = ii.astype(np.float64), jj.astype(np.float64)
    h = np.asarray(cur_hits).reshape(P).astype(np.int64)
    with np.errstate(all="ignore"):
        z = np.asarray(cur_depth, np.float64).reshape(P) / h.astype(np.float64)
        D = tuple(((pixel0[k] + du[k] * di) + dv[k] * dj) - center[k] for k in range(3))
        L = np.sqrt(dot(D, D))
        g = z / L
        X = tuple(center[k] + D[k] * g for k in range(3))
        E = tuple(X[k] - pc[k] for k in range(3))
        en = dot(E, n)
        s = an / en
        front = (h != 0) & (s > 0) & (s < np.inf)
        Q = tuple(s * E[k] - A[k] for k in range(3))
        u = dot(cross(Q, pdv), n) * rnn
        v = dot(cross(pdu, Q), n) * rnn
        r = np.sqrt(dot(E, E))
        fu, fv = np.floor(u), np.floor(v)
        in_range = front & (fu >= -1) & (fu <= W - 1) & (fv >= -1) & (fv <= H - 1)
    return front, in_range, u, v, r


def accumulate(W, H, cam, cur, cam_prev, prev, **params):
    """rt_temporal_accumulate.  cur / prev: dicts of accum (P, 3), m2 (P), counts (P), depth (P), hits (P),
    albedo / normal (P, 3) or None, feature_samples.  Returns the merged (accum (P, 3), m2 (P), counts (P)
    int64, history (P) int64); the inputs are not modified."""
    prm = dict(DEFAULTS)
    for k in params:
        if k not in prm:
            raise TypeError(k)
    prm.update(params)
    P = W * H
    c, q_ = _frame(W, H, cur), _frame(W, H, prev)
    _, in_range, u, v, r = project(W, H, cam, c["depth"], c["hits"], cam_prev)
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u), np.floor(v)
        i0 = np.where(in_range, fu, 0.0).astype(np.int64)
        j0 = np.where(in_range, fv, 0.0).astype(np.int64)
        fx, fy = u - fu, v - fv
        cov_p = c["hits"].astype(np.float64) * c["fi"]
        Np = c["normal"] * c["fi"] if c["normal"] is not None else None
        Ap = c["albedo"] * c["fi"] if c["albedo"] is not None else None
        zt = prm["sigma_z"] * r
        sw, sq = np.zeros(P), np.zeros(P)
        sc = np.zeros((P, 3))
        nmin = np.full(P, U32_MAX, np.int64)
        anyv = np.zeros(P, bool)
        for b in (0, 1):
            for a in (0, 1):
                qi, qj = i0 + a, j0 + b
                inside = in_range & (qi >= 0) & (qi < W) & (qj >= 0) & (qj < H)
                bw = (fx if a else 1.0 - fx) * (fy if b else 1.0 - fy)
                q = np.where(inside, qj * W + qi, 0)
                cq, hq = q_["counts"][q], q_["hits"][q]
                valid = inside & (bw != 0) & (cq > 0) & (hq > 0)
                zq = q_["depth"][q] / hq.astype(np.float64)
                valid &= np.abs(zq - r) <= zt
                if Np is not None:
                    Nq = q_["normal"][q] * q_["fi"]
                    e = Np - Nq
                    valid &= ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) <= prm["tau_n"]
                if Ap is not None:
                    Aq = q_["albedo"][q] * q_["fi"]
                    e = Ap - Aq
                    valid &= ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) <= prm["tau_a"]
                cov_q = hq.astype(np.float64) * q_["fi"]
                valid &= np.abs(cov_p - cov_q) <= prm["tau_h"]
                rn = 1.0 / cq.astype(np.float64)
                sw = np.where(valid, sw + bw, sw)
                sc = np.where(valid[:, None], sc + bw[:, None] * (q_["accum"][q] * rn[:, None]), sc)
                sq = np.where(valid, sq + bw * (q_["m2"][q] * rn), sq)
                nmin = np.where(valid, np.minimum(nmin, cq), nmin)
                anyv |= valid
        take = anyv & (sw >= prm["min_weight"])
        cnt = c["counts"]
        nh = np.minimum(np.minimum(nmin, int(prm["max_history"])), U32_MAX - cnt)
        nh = np.where(take, nh, 0)
        got = nh > 0
        rs = 1.0 / sw
        hd = nh.astype(np.float64)
        base_a = np.where((cnt != 0)[:, None], c["accum"], 0.0)
        base_m = np.where(cnt != 0, c["m2"], 0.0)
        accum = np.where(got[:, None], base_a + (sc * rs[:, None]) * hd[:, None], c["accum"])
        m2 = np.where(got, base_m + (sq * rs) * hd, c["m2"])
    return accum, m2, cnt + nh, nh

// rt_temporal.hip — the temporal accumulation's kernel for gfx950 (rt.h rt_temporal_accumulate;
// DESIGN.md §5.11): every pixel's first-hit point is reprojected into the previous frame, the four
// bilinear taps there are tested against the pixel's own guides, and the surviving history is merged
// into the current sums as pseudo-samples.  Every operation is spelled out in f64 in the order rt.h
// gives, with no transcendental function and no fused multiply-add (contraction is off in this file and
// in the build), so the result is checked bit for bit against a numpy restatement
// (tests/temporal_ref.py).
//
//   temporal_accumulate_kernel  one thread per pixel, 256-thread blocks shaped as 32 x 8 pixels.  No
//                               LDS: the taps of a block cover about (32 + 1) x (8 + 1) records of the
//                               previous frame, which the block's waves fetch once from L2 between them.
// Loads: the colour, albedo and normal records are 24 bytes, so a record is only 8-byte aligned and
// each is read as three 8-byte loads; the three loads of a wave's 32 consecutive pixels together cover
// one contiguous 768-byte run, every cache line of which is used whole.
#include "rt_temporal.h"

#pragma clang fp contract(off)

namespace rtk {

namespace {

struct Tp3 {
    double x, y, z;
};

__device__ __forceinline__ double tp_dot(const Tp3& a, const Tp3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ Tp3 tp_cross(const Tp3& a, const Tp3& b) {
    return Tp3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ Tp3 tp_load(const double* p) { return Tp3{p[0], p[1], p[2]}; }
__device__ __forceinline__ Tp3 tp_vec(const double v[3]) { return Tp3{v[0], v[1], v[2]}; }
// ((a0 - b0)^2 + (a1 - b1)^2) + (a2 - b2)^2
__device__ __forceinline__ double tp_dist2(const Tp3& a, const Tp3& b) {
    const double e0 = a.x - b.x, e1 = a.y - b.y, e2 = a.z - b.z;
    return (e0 * e0 + e1 * e1) + e2 * e2;
}

}  // namespace

__global__ __launch_bounds__(256) void temporal_accumulate_kernel(TemporalArgs a) {
    const uint32_t bx = blockIdx.x % a.tx, by = blockIdx.x / a.tx;
    const uint64_t i = (uint64_t)bx * kTpTileW + threadIdx.x, j = (uint64_t)by * kTpTileH + threadIdx.y;
    if (i >= a.W || j >= a.H) return;
    const int64_t W = a.W, H = a.H;
    const size_t p = (size_t)(j * a.W + i);
    uint32_t nh = 0;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, mq = 0.0;  // the history's per-sample means (sc * rs, sq * rs)
    const uint32_t c = a.cur.counts[p];
    const uint32_t h = a.cur.hits[p];
    if (h != 0) {  // a pixel without a hit has no point to reproject
        const double z = a.cur.depth[p] / (double)h;
        const double di = (double)i, dj = (double)j;
        Tp3 D;  // getRay's order with a zero offset
        D.x = ((a.pixel0[0] + a.du[0] * di) + a.dv[0] * dj) - a.center[0];
        D.y = ((a.pixel0[1] + a.du[1] * di) + a.dv[1] * dj) - a.center[1];
        D.z = ((a.pixel0[2] + a.du[2] * di) + a.dv[2] * dj) - a.center[2];
        const double L = __builtin_sqrt(tp_dot(D, D));
        const double g = z / L;
        const Tp3 X{a.center[0] + D.x * g, a.center[1] + D.y * g, a.center[2] + D.z * g};
        const Tp3 E{X.x - a.pc[0], X.y - a.pc[1], X.z - a.pc[2]};
        const Tp3 n = tp_vec(a.n);
        const double en = tp_dot(E, n);
        const double s = a.an / en;
        if (s > 0 && s < __builtin_inf()) {  // in front of the previous camera (false for a NaN)
            const Tp3 Q{s * E.x - a.A[0], s * E.y - a.A[1], s * E.z - a.A[2]};
            const double u = tp_dot(tp_cross(Q, tp_vec(a.pdv)), n) * a.rnn;
            const double v = tp_dot(tp_cross(tp_vec(a.pdu), Q), n) * a.rnn;
            const double r = __builtin_sqrt(tp_dot(E, E));
            const double fu = __builtin_floor(u), fv = __builtin_floor(v);
            if (fu >= -1.0 && fu <= (double)(W - 1) && fv >= -1.0 && fv <= (double)(H - 1)) {
                const int64_t i0 = (int64_t)fu, j0 = (int64_t)fv;  // in [-1, W - 1] x [-1, H - 1]
                const double fx = u - fu, fy = v - fv;
                const double cov_p = (double)h * a.cur.fi;
                Tp3 Np{0.0, 0.0, 0.0}, Ap{0.0, 0.0, 0.0};
                if (a.cur.normal) {
                    const Tp3 t = tp_load(a.cur.normal + 3 * p);
                    Np = Tp3{t.x * a.cur.fi, t.y * a.cur.fi, t.z * a.cur.fi};
                }
                if (a.cur.albedo) {
                    const Tp3 t = tp_load(a.cur.albedo + 3 * p);
                    Ap = Tp3{t.x * a.cur.fi, t.y * a.cur.fi, t.z * a.cur.fi};
                }
                const double zt = a.sigma_z * r;
                double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, sq = 0.0;
                uint32_t nmin = 0xffffffffu;
                bool any = false;
#pragma unroll
                for (int b = 0; b < 2; ++b) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int64_t qi = i0 + t, qj = j0 + b;
                        if (qi < 0 || qi >= W || qj < 0 || qj >= H) continue;
                        const double bw = (t ? fx : 1.0 - fx) * (b ? fy : 1.0 - fy);
                        if (bw == 0) continue;
                        const size_t q = (size_t)(qj * W + qi);
                        const uint32_t cq = a.prev.counts[q], hq = a.prev.hits[q];
                        if (cq == 0 || hq == 0) continue;
                        const double zq = a.prev.depth[q] / (double)hq;
                        if (!(__builtin_fabs(zq - r) <= zt)) continue;
                        if (a.prev.normal) {
                            const Tp3 w = tp_load(a.prev.normal + 3 * q);
                            const Tp3 Nq{w.x * a.prev.fi, w.y * a.prev.fi, w.z * a.prev.fi};
                            if (!(tp_dist2(Np, Nq) <= a.tau_n)) continue;
                        }
                        if (a.prev.albedo) {
                            const Tp3 w = tp_load(a.prev.albedo + 3 * q);
                            const Tp3 Aq{w.x * a.prev.fi, w.y * a.prev.fi, w.z * a.prev.fi};
                            if (!(tp_dist2(Ap, Aq) <= a.tau_a)) continue;
                        }
                        const double cov_q = (double)hq * a.prev.fi;
                        if (!(__builtin_fabs(cov_p - cov_q) <= a.tau_h)) continue;
                        const double rn = 1.0 / (double)cq;
                        const Tp3 aq = tp_load(a.prev.accum + 3 * q);
                        sw = sw + bw;
                        s0 = s0 + bw * (aq.x * rn);
                        s1 = s1 + bw * (aq.y * rn);
                        s2 = s2 + bw * (aq.z * rn);
                        sq = sq + bw * (a.prev.m2[q] * rn);
                        nmin = cq < nmin ? cq : nmin;
                        any = true;
                    }
                }
                if (any && sw >= a.min_weight) {
                    nh = nmin < a.max_history ? nmin : a.max_history;
                    const uint32_t room = 0xffffffffu - c;
                    nh = nh < room ? nh : room;
                    const double rs = 1.0 / sw;
                    m0 = s0 * rs, m1 = s1 * rs, m2 = s2 * rs, mq = sq * rs;
                }
            }
        }
    }
    if (a.history) a.history[p] = nh;
    if (nh == 0) return;  // no history: no byte of the current frame at this pixel is written
    const double hd = (double)nh;
    double b0 = 0.0, b1 = 0.0, b2 = 0.0, bq = 0.0;
    if (c != 0) {  // a pixel without samples starts from 0: its sums are not read
        const Tp3 t = tp_load(a.cur.accum + 3 * p);
        b0 = t.x, b1 = t.y, b2 = t.z;
        bq = a.cur.m2[p];
    }
    a.cur.accum[3 * p] = b0 + m0 * hd;
    a.cur.accum[3 * p + 1] = b1 + m1 * hd;
    a.cur.accum[3 * p + 2] = b2 + m2 * hd;
    a.cur.m2[p] = bq + mq * hd;
    a.cur.counts[p] = c + nh;
}

}  // namespace rtk

extern "C" hipError_t rtk_launch_temporal(rtk::TemporalArgs* a, hipStream_t stream) {
    if (a->W == 0 || a->H == 0) return hipErrorInvalidConfiguration;
    const uint64_t tx = ((uint64_t)a->W + rtk::kTpTileW - 1) / rtk::kTpTileW;
    const uint64_t ty = ((uint64_t)a->H + rtk::kTpTileH - 1) / rtk::kTpTileH;
    if (tx * ty > 0x7fffffffull) return hipErrorInvalidConfiguration;
    a->tx = (uint32_t)tx;
    hipLaunchKernelGGL(rtk::temporal_accumulate_kernel, dim3((uint32_t)(tx * ty)), dim3(rtk::kTpTileW, rtk::kTpTileH), 0,
                       stream, *a);
    return hipGetLastError();
}

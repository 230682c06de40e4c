// rt_denoise.hip — the denoiser's kernels for gfx950 (rt.h rt_denoise): a variance-
// and feature-guided à-trous filter whose every operation is spelled out in f64, so the result is
// checked bit for bit against a numpy restatement (tests/denoise_ref.py).  No transcendental
// function, no fused multiply-add (contraction is off in this file and in the build), a fixed
// summation order: taps ty = -2..2 outer, tx = -2..2 inner.
//
//   denoise_prepare_kernel    one thread per pixel: the caller's sums -> colour + variance (32 B) and
//                             the eight guide doubles (64 B) in the context's workspace
//   denoise_prefilter_kernel  the 3x3 variance prefilter
//   denoise_level_tile_kernel one level, taps read from an LDS tile.  At step s the pixels congruent
//                             mod s form s x s independent lattices; a block takes 32 x 8 pixels of
//                             one lattice plus a 2-pixel lattice halo (432 records in 12 planes of
//                             doubles, 40.5 KiB), so one kernel serves every step
//   denoise_level_direct_kernel  the same level, one thread per pixel, taps read from global memory
// Both level forms call the same tap function on the same values in the same order: same bits.
#include "rt_denoise.h"

#include "rt_device.h"

#pragma clang fp contract(off)

namespace rtk {

namespace {

struct DnCenter {
    double l, isd, n0, n1, n2, a0, a1, a2, cov, z;
};
struct DnAcc {
    double sw, s0, s1, s2, sv;
};

// K = {1, 4, 6, 4, 1} / 16 as integers: K[ty] * K[tx] = (k(ty) * k(tx)) / 256, exact in f64
__device__ __forceinline__ constexpr int dn_k(int t) { return t == 0 ? 6 : ((t == 1 || t == -1) ? 4 : 1); }

__device__ __forceinline__ DnCenter dn_center(const DenoiseParams& P, double c0, double c1, double c2, double v,
                                              double n0, double n1, double n2, double a0, double a1, double a2,
                                              double cov, double z) {
    DnCenter c;
    c.l = (c0 + c1) + c2;
    c.isd = 1.0 / (P.sigma_l * __builtin_sqrt(v) + P.epsilon);
    c.n0 = n0, c.n1 = n1, c.n2 = n2;
    c.a0 = a0, c.a1 = a1, c.a2 = a2;
    c.cov = cov;
    c.z = z;
    return c;
}

// One tap (rt.h: the operation order is the contract).  r = (double)(max(|tx|, |ty|) * step),
// kw = K[ty] * K[tx].
__device__ __forceinline__ void dn_tap(const DenoiseParams& P, const DnCenter& c, double r, double kw, double q0,
                                       double q1, double q2, double qv, double qn0, double qn1, double qn2, double qa0,
                                       double qa1, double qa2, double qcov, double qz, DnAcc& a) {
    const double lq = (q0 + q1) + q2;
    const double dl = __builtin_fabs(c.l - lq) * c.isd;
    const double e0 = c.n0 - qn0, e1 = c.n1 - qn1, e2 = c.n2 - qn2;
    const double dn = P.sigma_n * ((e0 * e0 + e1 * e1) + e2 * e2);
    const double f0 = c.a0 - qa0, f1 = c.a1 - qa1, f2 = c.a2 - qa2;
    const double da = P.sigma_a * ((f0 * f0 + f1 * f1) + f2 * f2);
    const double dh = P.sigma_h * __builtin_fabs(c.cov - qcov);
    double dz = 0.0;
    if (r > 0 && c.z > 0 && qz > 0) dz = __builtin_fabs(c.z - qz) / ((P.sigma_z * r) * (c.z + qz) + P.epsilon);
    const double d = ((dl + dn) + da) + (dh + dz);
    const double x = 1.0 - d * 0.125;
    double t = x > 0 ? x : 0.0;
    t = t * t;
    t = t * t;
    t = t * t;
    const double w = t * kw;
    a.sw = a.sw + w;
    a.s0 = a.s0 + w * q0;
    a.s1 = a.s1 + w * q1;
    a.s2 = a.s2 + w * q2;
    a.sv = a.sv + (w * w) * qv;
}

// A pass's result for pixel p: the next pass's record, or the caller's buffers (last pass).
__device__ __forceinline__ void dn_store(const DenoiseSink& s, size_t p, double c0, double c1, double c2, double v) {
    if (s.cv) {
        double2* o = (double2*)(s.cv + 4 * p);
        o[0] = double2{c0, c1};
        o[1] = double2{c2, v};
        return;
    }
    if (s.format == 0) {
        double* o = (double*)s.out + 3 * p;
        o[0] = c0;
        o[1] = c1;
        o[2] = c2;
    } else {
        uint8_t* o = (uint8_t*)s.out + 3 * p;
        o[0] = to_byte(c0);
        o[1] = to_byte(c1);
        o[2] = to_byte(c2);
    }
    if (s.var_out) s.var_out[p] = v;
}

__device__ __forceinline__ void dn_finish(const DenoiseSink& s, size_t p, const DnAcc& a) {
    const double rs = 1.0 / a.sw;
    dn_store(s, p, a.s0 * rs, a.s1 * rs, a.s2 * rs, a.sv * (rs * rs));
}

}  // namespace

__global__ __launch_bounds__(256) void denoise_prepare_kernel(DenoisePrepareArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.P) return;
    const uint32_t cnt = a.counts[p];
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, var = 0.0;
    if (cnt != 0) {
        const double n = (double)cnt;
        const double x = a.accum[3 * (size_t)p], y = a.accum[3 * (size_t)p + 1], z = a.accum[3 * (size_t)p + 2];
        const double scale = 1.0 / n;  // rt_accum_resolve_counts' bits
        c0 = x * scale;
        c1 = y * scale;
        c2 = z * scale;
        if (cnt >= 2) {  // rt_accum_select's operations without the square root
            const double S = (x + y) + z;
            const double mean = S / n;
            const double v = a.m2[p] - S * mean;
            var = v > 0 ? (v / (n - 1)) / n : 0.0;
        }
    }
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, cov = 0.0, z = 0.0;
    if (a.normal) {
        n0 = a.normal[3 * (size_t)p] * a.fi;
        n1 = a.normal[3 * (size_t)p + 1] * a.fi;
        n2 = a.normal[3 * (size_t)p + 2] * a.fi;
    }
    if (a.albedo) {
        a0 = a.albedo[3 * (size_t)p] * a.fi;
        a1 = a.albedo[3 * (size_t)p + 1] * a.fi;
        a2 = a.albedo[3 * (size_t)p + 2] * a.fi;
    }
    if (a.hits) {
        const uint32_t hc = a.hits[p];
        const double h = (double)hc;
        cov = h * a.fi;
        if (a.depth && hc != 0) z = a.depth[p] / h;
    }
    double2* ocv = (double2*)(a.cv + 4 * (size_t)p);
    ocv[0] = double2{c0, c1};
    ocv[1] = double2{c2, var};
    double2* og = (double2*)(a.g + 8 * (size_t)p);
    og[0] = double2{n0, n1};
    og[1] = double2{n2, a0};
    og[2] = double2{a1, a2};
    og[3] = double2{cov, z};
}

// v0 = sum(g * var_q) / sum(g) over the 3x3 taps inside the image, g = G[ty] * G[tx], G = {1, 2, 1} / 4
__global__ __launch_bounds__(256) void denoise_prefilter_kernel(const double* __restrict__ cv, uint32_t W, uint32_t H,
                                                                DenoiseSink sink) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint64_t)W * H) return;
    const int64_t i = (int64_t)(p % W), j = (int64_t)(p / W);
    double sv = 0.0, sg = 0.0;
#pragma unroll
    for (int ty = -1; ty <= 1; ++ty) {
#pragma unroll
        for (int tx = -1; tx <= 1; ++tx) {
            const int64_t qi = i + tx, qj = j + ty;
            if (qi < 0 || qi >= (int64_t)W || qj < 0 || qj >= (int64_t)H) continue;
            const double g = (double)((ty == 0 ? 2 : 1) * (tx == 0 ? 2 : 1)) * 0.0625;  // exact
            sv = sv + g * cv[4 * (size_t)(qj * W + qi) + 3];
            sg = sg + g;
        }
    }
    const double* c = cv + 4 * (size_t)p;
    dn_store(sink, (size_t)p, c[0], c[1], c[2], sv / sg);
}

__global__ __launch_bounds__(256) void denoise_level_direct_kernel(DenoiseLevelArgs a) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint64_t)a.W * a.H) return;
    const int64_t W = a.W, H = a.H, s = a.step;
    const int64_t i = (int64_t)(p % a.W), j = (int64_t)(p / a.W);
    const double2* pc = (const double2*)(a.cv + 4 * (size_t)p);
    const double2* pg = (const double2*)(a.g + 8 * (size_t)p);
    const double2 c01 = pc[0], c2v = pc[1], g0 = pg[0], g1 = pg[1], g2 = pg[2], g3 = pg[3];
    const DnCenter c = dn_center(a.p, c01.x, c01.y, c2v.x, c2v.y, g0.x, g0.y, g1.x, g1.y, g2.x, g2.y, g3.x, g3.y);
    DnAcc acc{0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ty = -2; ty <= 2; ++ty) {
#pragma unroll
        for (int tx = -2; tx <= 2; ++tx) {
            const int64_t qi = i + tx * s, qj = j + ty * s;
            if (qi < 0 || qi >= W || qj < 0 || qj >= H) continue;
            const size_t q = (size_t)(qj * W + qi);
            const double2* qc = (const double2*)(a.cv + 4 * q);
            const double2* qg = (const double2*)(a.g + 8 * q);
            const double2 q01 = qc[0], q2v = qc[1], h0 = qg[0], h1 = qg[1], h2 = qg[2], h3 = qg[3];
            const int m = (tx < 0 ? -tx : tx) > (ty < 0 ? -ty : ty) ? (tx < 0 ? -tx : tx) : (ty < 0 ? -ty : ty);
            const double r = (double)((int64_t)m * s);
            const double kw = (double)(dn_k(ty) * dn_k(tx)) * 0.00390625;  // / 256, exact
            dn_tap(a.p, c, r, kw, q01.x, q01.y, q2v.x, q2v.y, h0.x, h0.y, h1.x, h1.y, h2.x, h2.y, h3.x, h3.y, acc);
        }
    }
    dn_finish(a.sink, (size_t)p, acc);
}

__global__ __launch_bounds__(256) void denoise_level_tile_kernel(DenoiseLevelArgs a) {
    __shared__ double lds[kDnPlanes][kDnRecords];
    const int64_t W = a.W, H = a.H, s = a.step;
    const uint32_t bxn = a.lx * a.tx;  // blocks along x: lattices x tiles per lattice
    const uint32_t bx = blockIdx.x % bxn, by = blockIdx.x / bxn;
    const int64_t ri = bx / a.tx, rj = by / a.ty;                      // the lattice: pixels (ri + u s, rj + v s)
    const int64_t u0 = (int64_t)(bx % a.tx) * kDnTileW, v0 = (int64_t)(by % a.ty) * kDnTileH;  // the tile's origin in it
    if (ri + u0 * s >= W || rj + v0 * s >= H) return;  // block-uniform: a tile past the lattice's end
    for (uint32_t rec = threadIdx.x; rec < kDnRecords; rec += 256u) {
        const int64_t u = u0 + (int64_t)(rec % kDnPitch) - kDnHalo, v = v0 + (int64_t)(rec / kDnPitch) - kDnHalo;
        const int64_t qi = ri + u * s, qj = rj + v * s;
        double2 q01{0.0, 0.0}, q2v = q01, h0 = q01, h1 = q01, h2 = q01, h3 = q01;
        if (u >= 0 && v >= 0 && qi < W && qj < H) {
            const size_t q = (size_t)(qj * W + qi);
            const double2* qc = (const double2*)(a.cv + 4 * q);
            const double2* qg = (const double2*)(a.g + 8 * q);
            q01 = qc[0], q2v = qc[1], h0 = qg[0], h1 = qg[1], h2 = qg[2], h3 = qg[3];
        }
        lds[0][rec] = q01.x, lds[1][rec] = q01.y, lds[2][rec] = q2v.x, lds[3][rec] = q2v.y;
        lds[4][rec] = h0.x, lds[5][rec] = h0.y, lds[6][rec] = h1.x, lds[7][rec] = h1.y;
        lds[8][rec] = h2.x, lds[9][rec] = h2.y, lds[10][rec] = h3.x, lds[11][rec] = h3.y;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % kDnTileW, ly = threadIdx.x / kDnTileW;
    const int64_t i = ri + (u0 + lx) * s, j = rj + (v0 + ly) * s;
    if (i >= W || j >= H) return;
    const uint32_t ctr = (ly + kDnHalo) * kDnPitch + lx + kDnHalo;
    const DnCenter c = dn_center(a.p, lds[0][ctr], lds[1][ctr], lds[2][ctr], lds[3][ctr], lds[4][ctr], lds[5][ctr],
                                 lds[6][ctr], lds[7][ctr], lds[8][ctr], lds[9][ctr], lds[10][ctr], lds[11][ctr]);
    DnAcc acc{0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ty = -2; ty <= 2; ++ty) {
#pragma unroll
        for (int tx = -2; tx <= 2; ++tx) {
            const int64_t qi = i + tx * s, qj = j + ty * s;
            if (qi < 0 || qi >= W || qj < 0 || qj >= H) continue;
            const uint32_t q = (uint32_t)((int)ctr + ty * (int)kDnPitch + tx);  // within the 36 x 12 records
            const int m = (tx < 0 ? -tx : tx) > (ty < 0 ? -ty : ty) ? (tx < 0 ? -tx : tx) : (ty < 0 ? -ty : ty);
            const double r = (double)((int64_t)m * s);
            const double kw = (double)(dn_k(ty) * dn_k(tx)) * 0.00390625;  // / 256, exact
            dn_tap(a.p, c, r, kw, lds[0][q], lds[1][q], lds[2][q], lds[3][q], lds[4][q], lds[5][q], lds[6][q],
                   lds[7][q], lds[8][q], lds[9][q], lds[10][q], lds[11][q], acc);
        }
    }
    dn_finish(a.sink, (size_t)(j * W + i), acc);
}

namespace {

// the tile form's grid for step s: {lattices x, lattices y, tiles per lattice x, y}; false if the
// block count does not fit a 1-D launch
bool dn_tile_grid(uint32_t W, uint32_t H, uint32_t s, uint32_t g[4], uint64_t* blocks) {
    if (W == 0 || H == 0 || s == 0) return false;
    g[0] = s < W ? s : W;
    g[1] = s < H ? s : H;
    const uint32_t la = (uint32_t)(((uint64_t)W + s - 1) / s), lb = (uint32_t)(((uint64_t)H + s - 1) / s);
    g[2] = (la + kDnTileW - 1) / kDnTileW;
    g[3] = (lb + kDnTileH - 1) / kDnTileH;
    const uint64_t bx = (uint64_t)g[0] * g[2], by = (uint64_t)g[1] * g[3];
    if (bx > 0x7fffffffull || by > 0x7fffffffull) return false;
    *blocks = bx * by;
    return *blocks <= 0x7fffffffull;
}

}  // namespace

}  // namespace rtk

extern "C" hipError_t rtk_launch_denoise_prepare(const rtk::DenoisePrepareArgs* a, hipStream_t stream) {
    const uint32_t blocks = (uint32_t)(((uint64_t)a->P + 255) / 256);
    hipLaunchKernelGGL(rtk::denoise_prepare_kernel, dim3(blocks), dim3(256), 0, stream, *a);
    return hipGetLastError();
}

extern "C" hipError_t rtk_launch_denoise_prefilter(const double* cv, uint32_t W, uint32_t H,
                                                   const rtk::DenoiseSink* sink, hipStream_t stream) {
    const uint32_t blocks = (uint32_t)(((uint64_t)W * H + 255) / 256);
    hipLaunchKernelGGL(rtk::denoise_prefilter_kernel, dim3(blocks), dim3(256), 0, stream, cv, W, H, *sink);
    return hipGetLastError();
}

extern "C" int rtk_denoise_tile_ok(uint32_t W, uint32_t H, uint32_t step) {
    uint32_t g[4];
    uint64_t blocks = 0;
    return rtk::dn_tile_grid(W, H, step, g, &blocks) ? 1 : 0;
}

extern "C" hipError_t rtk_launch_denoise_level(rtk::DenoiseLevelArgs* a, int tile, hipStream_t stream) {
    if (tile) {
        uint32_t g[4];
        uint64_t blocks = 0;
        if (!rtk::dn_tile_grid(a->W, a->H, a->step, g, &blocks)) return hipErrorInvalidConfiguration;
        a->lx = g[0], a->ly = g[1], a->tx = g[2], a->ty = g[3];
        hipLaunchKernelGGL(rtk::denoise_level_tile_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, *a);
    } else {
        const uint32_t blocks = (uint32_t)(((uint64_t)a->W * a->H + 255) / 256);
        hipLaunchKernelGGL(rtk::denoise_level_direct_kernel, dim3(blocks), dim3(256), 0, stream, *a);
    }
    return hipGetLastError();
}

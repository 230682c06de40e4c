// rt_probe.hip — the path tracer's f64 primitives (csrc/rt_device.h, csrc/rt_leaf_filter.h) and the BVH
// walk's f32 slab primitives (csrc/rt_slab.h), one small kernel each, so that a test can feed them operands value by value (tests/test_gpu_primitives.py).
// Test infrastructure like the oracle: built as raytracing-with-zig_amd/librtzig_probe.so with the
// kernels' own flags, never linked into the product.
//
// One entry point, rt_probe_run(op, in, in_bytes, out, out_bytes, n, k, stream).  Buffers are planes
// of n 8-byte elements: input plane p of element i at in[p * n + i], output plane likewise (the leaf
// filter's output is one plane of n bytes).  n is a multiple of 256: kernels run whole blocks of 256
// threads with every lane active (RayDiv, sqrt_g, unit and Random.float take wave-wide ballots), and
// the caller pads.  An f32 operand or result is the low half of its 8-byte element (the high half of a
// result is 0).  k is the number of RNG steps per element (RNG ops only, at most kMaxDraws = 64).
// Every kernel reads and writes planes of its own element index only, and the entry point refuses
// buffers smaller than the op's planes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../raytracing-with-zig_amd/csrc/rt_device.h"
#include "../../raytracing-with-zig_amd/csrc/rt_leaf_filter.h"
#include "../../raytracing-with-zig_amd/csrc/rt_slab.h"

namespace {
using namespace rtk;

constexpr int kBlock = 256;
constexpr uint32_t kMaxDraws = 64;
constexpr uint64_t kNoDraw = 0xfff8dead0000beefULL;  // what a lane that does not draw writes (a NaN)

enum Op : int {
    kSqrt = 0,         // x -> sqrt_g(x)
    kUnit = 1,         // v -> unit(v)
    kUnitAccepted = 2, // p -> p / sqrt(|p|^2) as the scatter finish computes it
    kRayDiv = 3,       // a, x -> RayDiv(a).div(x)
    kReflect = 4,      // v, n -> reflect(v, n)
    kRefract = 5,      // v, n, eta -> refract(v, n, eta)
    kRangePm1 = 6,     // u -> Rng::pm1_of(u)
    kSampleKey = 7,    // seed, pixel, sample -> sample_key(mix(seed), pixel, sample)
    kSeedWords = 8,    // key -> k words of Rng::seed(key)
    kStateWordsLean = 9,      // s0..s3, mask -> k masked next() words, RngT<true>
    kStateWordsFull = 10,     // ... RngT<false>
    kStateUniformLean = 11,   // s0..s3, mask -> k masked uniform() doubles, RngT<true>
    kStateUniformFull = 12,   // ... RngT<false>
    kLeafBehind = 13,  // a, t_min, h, disc -> LeafFilter::make(a, t_min).behind(h, disc), one byte
    kMulRcp = 14,      // a, x -> x * (1.0 / a): the control, two roundings
    kRcpClamp = 15,    // d -> rcp_clamp(d) (f32)
    kPkFmaLo = 16,     // b.x, b.y, m.x, m.y, a.x, a.y -> pk_fma_lo(b, m, a).x, .y (f32)
    kPkMulAdd = 17,    // ... -> b.x * m.x + a.x, b.y * m.x + a.x: the control, two roundings each
    kSlabNear = 18,    // x, y, z, lower -> slab_near (f32)
    kSlabFar = 19,     // x, y, z, upper -> slab_far (f32)
    kOps = 20
};

struct Planes { int in, out; bool draws, bytes; };  // out planes are per draw when `draws`
__host__ constexpr Planes planes(int op) {
    switch (op) {
        case kSqrt: return {1, 1, false, false};
        case kUnit: case kUnitAccepted: return {3, 3, false, false};
        case kRayDiv: case kMulRcp: return {2, 1, false, false};
        case kReflect: return {6, 3, false, false};
        case kRefract: return {7, 3, false, false};
        case kRangePm1: return {1, 1, false, false};
        case kSampleKey: return {3, 1, false, false};
        case kSeedWords: return {1, 1, true, false};
        case kStateWordsLean: case kStateWordsFull: case kStateUniformLean: case kStateUniformFull:
            return {5, 1, true, false};
        case kLeafBehind: return {4, 1, false, true};
        case kRcpClamp: return {1, 1, false, false};
        case kPkFmaLo: case kPkMulAdd: return {6, 2, false, false};
        case kSlabNear: case kSlabFar: return {4, 1, false, false};
        default: return {0, 0, false, false};
    }
}

__device__ __forceinline__ uint64_t gid() { return (uint64_t)blockIdx.x * kBlock + threadIdx.x; }
__device__ __forceinline__ v3 ld3(const double* in, uint64_t n, uint64_t i, int p) {
    return mk(in[(uint64_t)p * n + i], in[(uint64_t)(p + 1) * n + i], in[(uint64_t)(p + 2) * n + i]);
}
__device__ __forceinline__ void st3(double* out, uint64_t n, uint64_t i, v3 v) {
    out[i] = v.x;
    out[n + i] = v.y;
    out[2 * n + i] = v.z;
}

__global__ __launch_bounds__(kBlock) void k_sqrt(const double* in, double* out, uint64_t n) {
    const uint64_t i = gid();
    out[i] = sqrt_g(in[i]);
}
__global__ __launch_bounds__(kBlock) void k_unit(const double* in, double* out, uint64_t n) {
    const uint64_t i = gid();
    st3(out, n, i, unit(ld3(in, n, i, 0)));
}
// the scatter finish of the path loop (rt_kernel.hip "scat_finish"), line for line
__global__ __launch_bounds__(kBlock) void k_unit_accepted(const double* in, double* out, uint64_t n) {
    const uint64_t i = gid();
    const v3 p = ld3(in, n, i, 0);
    const double uls = (p.x * p.x + p.y * p.y) + p.z * p.z;
    const double l = sqrt_normal(uls);
    const SharedRcp rl(l);
    st3(out, n, i, mk(rl.div(p.x), rl.div(p.y), rl.div(p.z)));
}
__global__ __launch_bounds__(kBlock) void k_raydiv(const double* in, double* out, uint64_t n) {
    const uint64_t i = gid();
    const RayDiv ad(in[i]);
    out[i] = ad.div(in[n + i]);
}
__global__ __launch_bounds__(kBlock) void k_mulrcp(const double* in, double* out, uint64_t n) {
    const uint64_t i = gid();
    const double inv = 1.0 / in[i];
    out[i] = in[n + i] * inv;
}
__global__ __launch_bounds__(kBlock) void k_reflect(const double* in, double* out, uint64_t n) {
    const uint64_t i = gid();
    st3(out, n, i, reflect(ld3(in, n, i, 0), ld3(in, n, i, 3)));
}
__global__ __launch_bounds__(kBlock) void k_refract(const double* in, double* out, uint64_t n) {
    const uint64_t i = gid();
    st3(out, n, i, refract(ld3(in, n, i, 0), ld3(in, n, i, 3), in[6 * n + i]));
}
__global__ __launch_bounds__(kBlock) void k_range_pm1(const double* in, double* out, uint64_t n) {
    const uint64_t i = gid();
    out[i] = Rng::pm1_of(in[i]);
}
__global__ __launch_bounds__(kBlock) void k_sample_key(const uint64_t* in, uint64_t* out, uint64_t n) {
    const uint64_t i = gid();
    out[i] = sample_key(sm_mix_hd(in[i]), in[n + i], (uint32_t)in[2 * n + i]);
}
__global__ __launch_bounds__(kBlock) void k_seed_words(const uint64_t* in, uint64_t* out, uint64_t n, uint32_t k) {
    const uint64_t i = gid();
    Rng g;
    g.seed(in[i]);
    if (k > kMaxDraws) k = kMaxDraws;
    for (uint32_t d = 0; d < kMaxDraws; d++) {
        if (d >= k) break;
        out[(uint64_t)d * n + i] = g.next();
    }
}
// k steps from an injected state; lane i draws at step d only if bit d of its mask is set, under a
// divergent `if` like the trip loop's third draw, and the state carries on to the next step.
template <bool kLean, bool kUniform>
__global__ __launch_bounds__(kBlock) void k_state(const uint64_t* in, uint64_t* out, uint64_t n, uint32_t k) {
    const uint64_t i = gid();
    RngT<kLean> g;
    g.s0 = in[i];
    g.s1 = in[n + i];
    g.s2 = in[2 * n + i];
    g.s3 = in[3 * n + i];
    const uint64_t mask = in[4 * n + i];
    if (k > kMaxDraws) k = kMaxDraws;
    for (uint32_t d = 0; d < kMaxDraws; d++) {
        if (d >= k) break;
        uint64_t w = kNoDraw;
        if ((mask >> d) & 1) {
            if constexpr (kUniform) w = __builtin_bit_cast(uint64_t, g.uniform());
            else w = g.next();
        }
        out[(uint64_t)d * n + i] = w;
    }
}
__global__ __launch_bounds__(kBlock) void k_leaf_behind(const double* in, uint8_t* out, uint64_t n) {
    const uint64_t i = gid();
    const LeafFilter f = LeafFilter::make(in[i], in[n + i]);
    out[i] = f.behind(in[2 * n + i], in[3 * n + i]) ? 1 : 0;
}

// f32 operands and results: the low half of an 8-byte element
__device__ __forceinline__ float ldf(const uint64_t* in, uint64_t n, uint64_t i, int p) {
    return __builtin_bit_cast(float, (uint32_t)in[(uint64_t)p * n + i]);
}
__device__ __forceinline__ uint64_t bits_of(float x) { return (uint64_t)__builtin_bit_cast(uint32_t, x); }

__global__ __launch_bounds__(kBlock) void k_rcp_clamp(const uint64_t* in, uint64_t* out, uint64_t n) {
    const uint64_t i = gid();
    out[i] = bits_of(rcp_clamp(ldf(in, n, i, 0)));
}
// the walk's call: the constants of an axis in the low halves of m and a, whose high halves are never read
__global__ __launch_bounds__(kBlock) void k_pk_fma_lo(const uint64_t* in, uint64_t* out, uint64_t n) {
    const uint64_t i = gid();
    const f2 b = {ldf(in, n, i, 0), ldf(in, n, i, 1)}, m = {ldf(in, n, i, 2), ldf(in, n, i, 3)};
    const f2 a = {ldf(in, n, i, 4), ldf(in, n, i, 5)};
    const f2 r = pk_fma_lo(b, m, a);
    out[i] = bits_of(r.x);
    out[n + i] = bits_of(r.y);
}
__global__ __launch_bounds__(kBlock) void k_pk_mul_add(const uint64_t* in, uint64_t* out, uint64_t n) {
    const uint64_t i = gid();
    const float m = ldf(in, n, i, 2), a = ldf(in, n, i, 4);
    const float px = ldf(in, n, i, 0) * m, py = ldf(in, n, i, 1) * m;  // contraction is off (rt_device.h)
    out[i] = bits_of(px + a);
    out[n + i] = bits_of(py + a);
}
template <bool kFar>
__global__ __launch_bounds__(kBlock) void k_slab(const uint64_t* in, uint64_t* out, uint64_t n) {
    const uint64_t i = gid();
    const float x = ldf(in, n, i, 0), y = ldf(in, n, i, 1), z = ldf(in, n, i, 2), w = ldf(in, n, i, 3);
    out[i] = bits_of(kFar ? slab_far(x, y, z, w) : slab_near(x, y, z, w));
}

}  // namespace

extern "C" {

// what a masked lane writes at a step it does not draw
__attribute__((visibility("default"))) uint64_t rt_probe_no_draw(void) { return kNoDraw; }

// the op's plane counts: 0, or -1 for an unknown op.  Output planes are per draw for the RNG ops.
__attribute__((visibility("default"))) int rt_probe_planes(int op, int* in_planes, int* out_planes, int* per_draw, int* byte_out) {
    const Planes p = planes(op);
    if (p.in == 0) return -1;
    *in_planes = p.in;
    *out_planes = p.out;
    *per_draw = p.draws;
    *byte_out = p.bytes;
    return 0;
}

// Runs `op` over n elements on `stream` (asynchronous).  0, or: -1 unknown op, -2 n not a positive
// multiple of 256 or too large, -3 k out of range, -4 a buffer too small or null, -5 launch failed.
__attribute__((visibility("default"))) int rt_probe_run(int op, const void* in, uint64_t in_bytes, void* out, uint64_t out_bytes,
                                                         uint64_t n, uint32_t k, void* stream) {
    const Planes p = planes(op);
    if (p.in == 0) return -1;
    if (n == 0 || n % kBlock != 0 || n > (1ull << 24)) return -2;
    if (p.draws && (k == 0 || k > kMaxDraws)) return -3;
    const uint64_t out_planes = p.draws ? k : (uint64_t)p.out;
    if (!in || !out || in_bytes < (uint64_t)p.in * n * 8 || out_bytes < out_planes * n * (p.bytes ? 1 : 8)) return -4;
    const dim3 grid((unsigned)(n / kBlock)), block(kBlock);
    hipStream_t s = (hipStream_t)stream;
    const double* din = (const double*)in;
    const uint64_t* uin = (const uint64_t*)in;
    double* dout = (double*)out;
    uint64_t* uout = (uint64_t*)out;
    switch (op) {
        case kSqrt: k_sqrt<<<grid, block, 0, s>>>(din, dout, n); break;
        case kUnit: k_unit<<<grid, block, 0, s>>>(din, dout, n); break;
        case kUnitAccepted: k_unit_accepted<<<grid, block, 0, s>>>(din, dout, n); break;
        case kRayDiv: k_raydiv<<<grid, block, 0, s>>>(din, dout, n); break;
        case kReflect: k_reflect<<<grid, block, 0, s>>>(din, dout, n); break;
        case kRefract: k_refract<<<grid, block, 0, s>>>(din, dout, n); break;
        case kRangePm1: k_range_pm1<<<grid, block, 0, s>>>(din, dout, n); break;
        case kSampleKey: k_sample_key<<<grid, block, 0, s>>>(uin, uout, n); break;
        case kSeedWords: k_seed_words<<<grid, block, 0, s>>>(uin, uout, n, k); break;
        case kStateWordsLean: k_state<true, false><<<grid, block, 0, s>>>(uin, uout, n, k); break;
        case kStateWordsFull: k_state<false, false><<<grid, block, 0, s>>>(uin, uout, n, k); break;
        case kStateUniformLean: k_state<true, true><<<grid, block, 0, s>>>(uin, uout, n, k); break;
        case kStateUniformFull: k_state<false, true><<<grid, block, 0, s>>>(uin, uout, n, k); break;
        case kLeafBehind: k_leaf_behind<<<grid, block, 0, s>>>(din, (uint8_t*)out, n); break;
        case kMulRcp: k_mulrcp<<<grid, block, 0, s>>>(din, dout, n); break;
        case kRcpClamp: k_rcp_clamp<<<grid, block, 0, s>>>(uin, uout, n); break;
        case kPkFmaLo: k_pk_fma_lo<<<grid, block, 0, s>>>(uin, uout, n); break;
        case kPkMulAdd: k_pk_mul_add<<<grid, block, 0, s>>>(uin, uout, n); break;
        case kSlabNear: k_slab<false><<<grid, block, 0, s>>>(uin, uout, n); break;
        case kSlabFar: k_slab<true><<<grid, block, 0, s>>>(uin, uout, n); break;
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"

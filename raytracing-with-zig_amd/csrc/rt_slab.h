// rt_slab.h — the f32 slab primitives of the BVH walk (BvhWalker::descend, run_f32 / run_f64 / any-hit in
// rt_kernel.hip): the clamped reciprocal of a direction component, the packed plane fma with its
// broadcast operands and the interval ends.  The only inline-asm arithmetic of the walk, in a header of
// their own so that tests/hip/rt_probe.hip can feed them operands value by value
// (tests/test_gpu_primitives.py).  The error budget they stand in: rt_bvh.cpp "Padding rules".
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtk {

// The walk's reciprocal: v_rcp_f32 (1 ulp) instead of a correctly rounded f32 division (~11 ops), then
// clamped to +-1e30 by one v_med3: the inverse of a component clamped to +-1e-30 (rcp(+-0) = +-inf keeps
// its sign), one op instead of compare + copysign + select.  A NaN component gives -1e30, whatever its
// sign: v_med3_f32 returns the least of its three operands when one of them is a NaN.  Nothing is lost
// by that: no f64 sphere test passes for a NaN direction, and rt_trace.h keeps such rays off the tree.
__device__ __forceinline__ float rcp_clamp(float d) {
    return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d), -1e30f, 1e30f);
}

// Slab-interval ends: max(x, y, z, lower) and min(x, y, z, upper) as hardware v_max3/v_min3 +
// v_max/v_min.  With IEEE mode on (the default) these return the non-NaN operand for quiet NaNs —
// exactly fmaxf/fminf on every value this walk produces (arithmetic never yields signaling NaNs) —
// but written as builtins the compiler re-canonicalizes the loop-carried bounds every iteration.
#ifndef RTZIG_WALK_FORM
#define RTZIG_WALK_FORM 0
#endif
#if RTZIG_WALK_FORM == 4
__device__ __forceinline__ float slab_near(float x, float y, float z, float lower) {
    float t, r;
    asm("v_max_f32 %0, %1, %2" : "=v"(t) : "v"(z), "v"(lower));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(t));
    return r;
}
__device__ __forceinline__ float slab_far(float x, float y, float z, float upper) {
    float t, r;
    asm("v_min_f32 %0, %1, %2" : "=v"(t) : "v"(z), "v"(upper));
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(t));
    return r;
}
#elif RTZIG_WALK_FORM >= 1
__device__ __forceinline__ float slab_near(float x, float y, float z, float lower) {
    return __builtin_fmaxf(__builtin_fmaxf(x, y), __builtin_fmaxf(z, lower));
}
__device__ __forceinline__ float slab_far(float x, float y, float z, float upper) {
    return __builtin_fminf(__builtin_fminf(x, y), __builtin_fminf(z, upper));
}
#else
__device__ __forceinline__ float slab_near(float x, float y, float z, float lower) {
    float t, r;
    asm volatile("v_max_f32 %0, %1, %2" : "=v"(t) : "v"(z), "v"(lower));
    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(t));
    return r;
}
__device__ __forceinline__ float slab_far(float x, float y, float z, float upper) {
    float t, r;
    asm volatile("v_min_f32 %0, %1, %2" : "=v"(t) : "v"(z), "v"(upper));
    asm volatile("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(t));
    return r;
}
#endif

typedef float f2 __attribute__((ext_vector_type(2)));
// {b.x * m.x + a.x, b.y * m.x + a.x}: v_pk_fma_f32 with the second and third operands' low halves
// broadcast to the high lane (op_sel_hi:[1,0,0]); their high halves are never read
// Forms of the inner step (A/B knob): 0 the shipped one (inline-asm v_pk_fma_f32 with a
// broadcast operand, volatile-asm v_max3/v_min3, asm ds_read_b64); 1 builtin packed fma and
// min/max; 2 form 1 with plain LDS loads (ds_read2_b64); 4 form 0 with the slab min/max as
// non-volatile asm (schedulable); 5 form 0 with builtin min/max.
#if RTZIG_WALK_FORM == 4 || RTZIG_WALK_FORM == 5
#define RTK_PK_ASM 1
#else
#define RTK_PK_ASM (RTZIG_WALK_FORM == 0)
#endif
__device__ __forceinline__ f2 pk_fma_lo(f2 b, f2 m, f2 a) {
#if !RTK_PK_ASM
    const f2 mm = {m.x, m.x}, aa = {a.x, a.x};
    return __builtin_elementwise_fma(b, mm, aa);
#else
    f2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(b), "v"(m), "v"(a));
    return r;
#endif
}

}  // namespace rtk

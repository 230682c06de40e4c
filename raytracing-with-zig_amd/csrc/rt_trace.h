// rt_trace.h — the domain rule of rt_trace_rays (rt.h): may the f32 slab walk of
// BvhWalker (rt_kernel.hip) cull for this ray, or must the ray take the reference's own list scan?
//
// The walk's certificate (rt_bvh.cpp "Padding rules", rt_kernel.hip run_f64) is written for the
// renderer's rays: directions of order 1, t_min = 1e-3, origins inside the tree's origin bound.  A
// ray query receives any six doubles and any interval, so the certificate's premises are checked per
// ray, in f64, on the ray as given.  A ray that fails is still answered exactly, by world_hit.
//
// The rule, and what each clause buys (the full argument: DESIGN.md §5.12):
//   1. all six components finite                 — no NaN / inf reaches the slab arithmetic;
//   2. max|o_k| <= origin_bound                  — the |o| part of the box padding (2^-21 x bound);
//   3. 2^-kTraceDirLog2 <= max|d_k| <= 2^kTraceDirLog2
//        — every accepted root obeys |t| <= 2 x bound / max|d_k| < 2^127, so a slab plane that
//          overflows f32 to +-inf still orders correctly against it; the f32 direction does not
//          overflow; and an axis whose reciprocal is clamped to +-1e30 moves the ray by less than
//          2^-78 x bound over that t range, far inside the padding;
//   4. 0 <= t_min < +inf                         — the renderer's side of the interval.  (t_max needs
//          no clause: its f32 cast is widened outward, a cast that underflows moves the bound by less
//          than 2^-106 in position, inside the padding's 2^-60, and an empty or NaN interval has no
//          hit to lose.);
//   5. |o_k| <= 2^126 x max(|d_k|, 2^-100) per axis — the f32 product o x (1 / d), reciprocal
//          clamped to 1e30 < 2^100, stays finite: an infinite -(o x inv) would put BOTH planes of the
//          axis at the same infinity and cull a box the origin lies inside.  With a component below
//          2^-100 this asks |o_k| <= 2^26: it never fires for a tree whose origin bound is at most
//          2^26 (6.7e7), i.e. clauses 1-4 alone decide there.
// The range of clause 3 is the narrowest the contract allows (every ordinary ray is inside it); the
// bounds above would hold up to 2^26, and nothing is gained by going there: the scan is always right.
#pragma once

#if defined(__HIPCC__)
#define RT_TRACE_HD __host__ __device__ __forceinline__
#else
#define RT_TRACE_HD inline
#endif

namespace rtk {

constexpr int kTraceDirLog2 = 20;

// |x| without <cmath> (one v_and on the device); -0.0 gives +0.0, a NaN stays a NaN
RT_TRACE_HD double trace_abs(double x) { return __builtin_fabs(x); }
// max that returns NaN when either operand is NaN (every later compare is then false)
RT_TRACE_HD double trace_max_nan(double a, double b) { return a != a ? a : (b > a || b != b ? b : a); }

// o, d: the ray as given (f64); [t_min, t_max]: its interval; origin_bound: BvhArgs::origin_bound of
// the tree that would be walked (rt_context_origin_bound).  Every comparison is written so that a
// NaN makes the result false.
RT_TRACE_HD bool trace_tree_ok(const double o[3], const double d[3], double t_min, double t_max, double origin_bound) {
    (void)t_max;  // no clause (see above)
    constexpr double kMaxFinite = 0x1.fffffffffffffp1023;
    const double ox = trace_abs(o[0]), oy = trace_abs(o[1]), oz = trace_abs(o[2]);
    const double dx = trace_abs(d[0]), dy = trace_abs(d[1]), dz = trace_abs(d[2]);
    const double om = trace_max_nan(trace_max_nan(ox, oy), oz);
    const double dm = trace_max_nan(trace_max_nan(dx, dy), dz);
    // clause 3 bounds dm; dx, dy, dz <= dm are then finite, and a NaN among them made dm NaN
    const bool dir_ok = dm >= 0x1p-20 && dm <= 0x1p20;
    static_assert(kTraceDirLog2 == 20, "the literals above");
    const bool org_ok = om <= origin_bound && om <= kMaxFinite;
    const bool tmin_ok = t_min >= 0 && t_min <= kMaxFinite;
    const bool prod_ok = ox <= 0x1p126 * (dx > 0x1p-100 ? dx : 0x1p-100) &&
                         oy <= 0x1p126 * (dy > 0x1p-100 ? dy : 0x1p-100) &&
                         oz <= 0x1p126 * (dz > 0x1p-100 ? dz : 0x1p-100);
    return dir_ok && org_ok && tmin_ok && prod_ok;
}

}  // namespace rtk

// rt_leaf_filter.h — the leaf round's exact candidate filter, host and device: fma, fabs and
// compares only, so the host evaluates the very same expression (tests/cpp/test_leaf_filter.cpp
// checks its soundness on the CPU, tests/hip/rt_probe.hip that the device answers the same).
#pragma once

#if defined(__HIPCC__)
#define RT_LF_HD __host__ __device__ __forceinline__
#else
#define RT_LF_HD inline
#endif

namespace rtk {

// Exact candidate filter for the leaf round.  With s = fl(sqrt(disc)), the reference's roots are
// root1 = fl(fl(h - s) / a) <= root2 = fl(fl(h + s) / a), and the candidate of a sphere is root1 if
// t_min < root1, else root2 if t_min < root2 (sphere.zig:35-41).  behind(h, disc) proves
// root2 <= t_min, so the sphere yields no candidate.  It is evaluated with explicit fma and margins
// of 2^-30 relative (plus a * 2^-600 absolute) that dominate every rounding error of the comparison
// (a few ulps), so it never rejects a sphere the exact candidate() would accept; NaN or inf operands
// make the test false (keep the sphere).  Proof: Z = (t_min*a - margins) - h - 2^-30|h|;
// Z > 0 and Z*Z > disc*(1 + 2^-30) give s < Z, hence h + s < t_min*a by more than the rounding of
// fl(h + s), so fl(h + s) / a < t_min and root1 <= root2 <= t_min.  The filter needs a within
// [2^-400, 2^400] (else it never rejects).  Typical catch: the sphere a secondary ray starts on
// (c ~ 0, h < 0), whose candidate otherwise costs a sqrt and two divisions for the whole wave.
struct LeafFilter {
    double a_tiny;  // a * 2^-600
    double tm_lim;  // t_min * a lowered by the margins
    bool on;
    RT_LF_HD static LeafFilter make(double a, double t_min) {
        LeafFilter f;
        f.on = a > 0x1p-400 && a < 0x1p400;
        f.a_tiny = a * 0x1p-600;
        const double pm = t_min * a;
        f.tm_lim = __builtin_fma(-__builtin_fabs(pm), 0x1p-30, pm) - f.a_tiny;
        return f;
    }
    RT_LF_HD bool behind(double h, double disc) const {
        const double z = __builtin_fma(-__builtin_fabs(h), 0x1p-30, tm_lim - h);
        return on && z > 0 && __builtin_fma(z, z, -(disc * (1 + 0x1p-30))) > 0;
    }
};

}  // namespace rtk

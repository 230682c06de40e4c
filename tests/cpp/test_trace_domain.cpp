// CPU test of rt_trace.h: trace_tree_ok on the sets the contract names.
//   must be FALSE: any non-finite origin or direction component; max|o_k| > origin_bound; a largest
//     direction component outside [2^-20, 2^20];
//   must be TRUE: six finite components, max|o_k| <= origin_bound, 2^-20 <= max|d_k| <= 2^20 and
//     0 <= t_min < +inf — whatever t_max is.
// The header's own choices are pinned too: negative and NaN t_min go to the scan, and the product
// guard |o_k| <= 2^126 max(|d_k|, 2^-100) fires only beyond an origin bound of 2^26.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../raytracing-with-zig_amd/csrc/rt_trace.h"

namespace {
long fails = 0, checks = 0;
const double kInf = std::numeric_limits<double>::infinity();
const double kNan = std::numeric_limits<double>::quiet_NaN();

void expect(bool want, const double* o, const double* d, double t_min, double t_max, double bound, const char* what) {
    ++checks;
    if (rtk::trace_tree_ok(o, d, t_min, t_max, bound) != want) {
        if (fails++ < 20)
            std::printf("FAIL (%s): want %d for o=(%a %a %a) d=(%a %a %a) t=(%a, %a) bound=%a\n", what, (int)want, o[0], o[1],
                        o[2], d[0], d[1], d[2], t_min, t_max, bound);
    }
}
}  // namespace

int main() {
    const double bound = 1000.0009765625;  // the final scene's, about
    const double o0[3] = {13.0, 2.0, -3.0}, d0[3] = {-0.7, 0.1, 0.5};
    const double t_maxes[] = {kInf, -kInf, kNan, 0.0, -1.0, 1e-300, 1e300, 2.0, 5e-324};
    const double t_mins_ok[] = {0.0, -0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1e-3, 1.0, 1e300,
                                std::numeric_limits<double>::max()};

    // the base ray, every interval of the must-be-true set (subnormal t_min included)
    for (double t_min : t_mins_ok)
        for (double t_max : t_maxes) expect(true, o0, d0, t_min, t_max, bound, "base");
    // t_min outside [0, inf): this header sends them to the scan
    for (double t_min : {-5e-324, -1e-3, -5.0, -kInf, kInf, kNan}) expect(false, o0, d0, t_min, kInf, bound, "t_min placed on the scan");

    // each component in turn NaN, +-inf (false) and +-0 (true: the other components carry the ray)
    for (int k = 0; k < 3; k++) {
        for (double bad : {kNan, kInf, -kInf}) {
            double o[3] = {o0[0], o0[1], o0[2]}, d[3] = {d0[0], d0[1], d0[2]};
            o[k] = bad;
            expect(false, o, d0, 1e-3, kInf, bound, "non-finite origin");
            expect(false, o, d0, 1e-3, kInf, kInf, "non-finite origin, infinite bound");
            d[k] = bad;
            expect(false, o0, d, 1e-3, kInf, bound, "non-finite direction");
        }
        for (double z : {0.0, -0.0}) {
            double o[3] = {o0[0], o0[1], o0[2]}, d[3] = {d0[0], d0[1], d0[2]};
            o[k] = z;
            expect(true, o, d0, 1e-3, kInf, bound, "zero origin component");
            d[k] = z;
            expect(true, o0, d, 1e-3, kInf, bound, "zero direction component");
        }
    }
    const double zero[3] = {0, 0, 0};
    expect(false, o0, zero, 1e-3, kInf, bound, "zero direction");
    expect(true, zero, d0, 1e-3, kInf, bound, "zero origin");

    // origins at the bound and one ulp beyond, on every axis and sign
    for (int k = 0; k < 3; k++)
        for (double s : {1.0, -1.0}) {
            double o[3] = {1.0, -2.0, 3.0};
            o[k] = s * bound;
            expect(true, o, d0, 1e-3, kInf, bound, "origin at the bound");
            o[k] = s * std::nextafter(bound, kInf);
            expect(false, o, d0, 1e-3, kInf, bound, "origin one ulp beyond the bound");
            o[k] = s * std::nextafter(bound, 0.0);
            expect(true, o, d0, 1e-3, kInf, bound, "origin one ulp inside the bound");
        }
    expect(false, o0, d0, 1e-3, kInf, 0.0, "bound 0 (list walk)");
    expect(false, o0, d0, 1e-3, kInf, kNan, "NaN bound");

    // direction scales 2^e, e = -1074 .. 1023: the largest component decides
    for (int e = -1074; e <= 1023; e++) {
        const double s = std::ldexp(1.0, e);
        for (int k = 0; k < 3; k++)
            for (double sg : {1.0, -1.0}) {
                double d[3] = {0.0, 0.0, 0.0};
                d[k] = sg * s;
                d[(k + 1) % 3] = sg * s * 0.25;
                const bool in_must_true = e >= -20 && e <= 20;
                expect(in_must_true, o0, d, 1e-3, kInf, bound, "direction scale (this header's range is the contract's)");
            }
    }
    // just outside the range, by one ulp
    {
        const double d_hi[3] = {std::nextafter(0x1p20, kInf), 0, 0}, d_lo[3] = {0, std::nextafter(0x1p-20, 0.0), 0};
        expect(false, o0, d_hi, 1e-3, kInf, bound, "2^20 + ulp");
        expect(false, o0, d_lo, 1e-3, kInf, bound, "2^-20 - ulp");
    }

    // random rays of the must-be-true set, for every origin bound a scene can have up to 2^26 (the
    // product guard is silent there), tiny other components included
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (double b : {1e-300, 1.0, 1000.0009765625, 6060.0, 0x1p26}) {
        for (int n = 0; n < 20000; n++) {
            double o[3], d[3];
            for (int k = 0; k < 3; k++) o[k] = u(rng) * b;
            const int major = (int)(rng() % 3);
            const double m = std::ldexp(1.0 + 0.999 * std::fabs(u(rng)), (int)(rng() % 40) - 20);  // [2^-20, 2^20)
            for (int k = 0; k < 3; k++) {
                const int kind = (int)(rng() % 4);
                d[k] = kind == 0 ? 0.0 : kind == 1 ? u(rng) * m : kind == 2 ? std::ldexp(u(rng), -1000) : u(rng) * 1e-35;
            }
            d[major] = (rng() & 1) ? m : -m;
            if (std::fabs(d[major]) > 0x1p20) d[major] = 0x1p20;
            expect(true, o, d, t_mins_ok[rng() % 10], t_maxes[rng() % 9], b, "random must-be-true ray");
        }
    }
    // beyond 2^26 the guard may refuse an origin component whose direction component is tiny: the f32
    // product o x 1e30 would overflow.  Pinned: refused, and accepted again with a component of order 1.
    {
        const double o[3] = {1e9, 1e9, 1e9}, d_tiny[3] = {1.0, 0.0, 0.0}, d_full[3] = {1.0, -1.0, 0.5};
        expect(false, o, d_tiny, 1e-3, kInf, 1e10, "f32 overflow of o x inv");
        expect(true, o, d_full, 1e-3, kInf, 1e10, "far origin, direction of order 1 on every axis");
    }

    std::printf("%ld checks, %ld fails\n%s\n", checks, fails, fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}

// rt_temporal.h — launch interface of the temporal accumulation (rt.h rt_temporal_accumulate; DESIGN.md
// §5.11), shared by the kernel (rt_temporal.hip) and the runtime (rt_runtime.cpp).  No workspace: the
// kernel reads the two frames' buffers and writes the current frame's in place.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtk {

// the block: 32 x 8 pixels, so the four-tap footprints of a block overlap in both directions
constexpr uint32_t kTpTileW = 32, kTpTileH = 8;

struct TemporalFrame {  // rt_temporal_frame with typed pointers and fi = 1.0 / feature_samples
    double* accum;          // [P][3]
    double* m2;             // [P]
    uint32_t* counts;       // [P]
    const double* albedo;   // [P][3] or null
    const double* normal;   // [P][3] or null
    const double* depth;    // [P]
    const uint32_t* hits;   // [P]
    double fi;
};

struct TemporalArgs {
    TemporalFrame cur, prev;  // prev is only read
    // the current camera (getRay's terms) and the per-call values of the previous one (rt.h):
    // pc = center', A = pixel0' - center', n = cross(du', dv'), an = dot(A, n), rnn = 1.0 / dot(n, n)
    double pixel0[3], du[3], dv[3], center[3];
    double pc[3], A[3], n[3], pdu[3], pdv[3], an, rnn;
    double sigma_z, tau_n, tau_a, tau_h, min_weight;
    uint32_t max_history;
    uint32_t W, H;
    uint32_t tx;            // tiles along x (set by the launcher)
    uint32_t* history;      // [P] or null
};

}  // namespace rtk

// one thread per pixel in 32 x 8 tiles; hipErrorInvalidConfiguration if the tiles do not fit a launch
extern "C" hipError_t rtk_launch_temporal(rtk::TemporalArgs* a, hipStream_t stream);

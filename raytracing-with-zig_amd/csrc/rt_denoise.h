// rt_denoise.h — launch interface of the denoiser (rt.h rt_denoise), shared by the
// kernels (rt_denoise.hip) and the runtime (rt_runtime.cpp).
//
// Workspace, 128 B per pixel, in three planes of P records each:
//   cv[0], cv[1]  {c0, c1, c2, v}: colour + variance of the mean luminance, 32 B; the levels ping-pong
//   g             {N0, N1, N2, A0, A1, A2, cov, z}: the guides, 64 B; written once by the prepare pass
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtk {

constexpr uint32_t kDenoiseBytesPerPixel = 128;
constexpr uint32_t kDenoiseMaxLevels = 16;
// the tile form's block: 32 x 8 pixels of one lattice (a wave's half is one row of 32 pixels, so its
// 8-byte LDS reads of one plane are 256 contiguous bytes: no bank conflict) plus a 2-pixel halo
constexpr uint32_t kDnTileW = 32, kDnTileH = 8, kDnHalo = 2;
constexpr uint32_t kDnPitch = kDnTileW + 2 * kDnHalo;                  // 36
constexpr uint32_t kDnRecords = kDnPitch * (kDnTileH + 2 * kDnHalo);   // 432
constexpr uint32_t kDnPlanes = 12;                                     // doubles per pixel: cv + g
// steps up to this one run the tile form by default, larger ones the direct form
constexpr uint32_t kDnTileMaxStep = 32;

struct DenoiseParams {  // rt_denoise_params without the level count
    double sigma_l, sigma_n, sigma_a, sigma_z, sigma_h, epsilon;
};

struct DenoisePrepareArgs {
    const double* accum;    // [P][3]
    const double* m2;       // [P]
    const uint32_t* counts; // [P]
    const double* albedo;   // [P][3] or null
    const double* normal;   // [P][3] or null
    const double* depth;    // [P] or null
    const uint32_t* hits;   // [P] or null
    double fi;              // 1.0 / feature_samples (0 when there are no guides)
    double* cv;             // out [P][4]
    double* g;              // out [P][8]
    uint32_t P;
};

// Where a pass puts its result: the next pass's cv plane, or — the last pass — the caller's buffers.
struct DenoiseSink {
    double* cv;         // [P][4], or null for the last pass
    void* out;          // the caller's image (last pass only)
    double* var_out;    // the caller's variance, may be null (last pass only)
    uint32_t format;    // rt_output_format of `out`
};

struct DenoiseLevelArgs {
    const double* cv;   // [P][4] of the previous pass
    const double* g;    // [P][8]
    DenoiseSink sink;
    DenoiseParams p;
    uint32_t W, H, step;
    // tile form: tiles per lattice along x / y and lattices along x / y (min(step, W), min(step, H))
    uint32_t tx, ty, lx, ly;
};

}  // namespace rtk

extern "C" hipError_t rtk_launch_denoise_prepare(const rtk::DenoisePrepareArgs* a, hipStream_t stream);
// the 3x3 variance prefilter: cv -> sink (colour copied, variance filtered)
extern "C" hipError_t rtk_launch_denoise_prefilter(const double* cv, uint32_t W, uint32_t H,
                                                   const rtk::DenoiseSink* sink, hipStream_t stream);
// one à-trous level; tile != 0: the LDS tile form, else the direct form (same bits)
extern "C" hipError_t rtk_launch_denoise_level(rtk::DenoiseLevelArgs* a, int tile, hipStream_t stream);
// can the tile form run this step on this image (its grid fits a launch)?
extern "C" int rtk_denoise_tile_ok(uint32_t W, uint32_t H, uint32_t step);

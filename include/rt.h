/*
 * rt.h — C ABI of the MI355X path tracer (drop-in for the reference's Camera.render()).
 *
 * The reference (AndrewJarrett/raytracing-with-zig, Zig 0.14) has no FFI of its own.  The cut is
 * `Camera.render(self: Camera) !void` (src/camera.zig:123-145), called from src/main.zig:35.  A Zig
 * shim marshals the Camera fields (camera.zig:82-103), the Hittable list
 * (hittable.zig:43-44, Sphere sphere.zig:13-16, Material material.zig:126-143) and the scene
 * interval/seed (Scene.zig:19-21) into the plain structs below and calls rt_render(), then keeps
 * its own PPM.saveBinary (ppm.zig:42-60, camera.zig:144).
 *
 * Everything is plain C: pointers + sizes, no torch / HIP types in the signatures (device pointers
 * and streams are passed as void*).  All functions return 0 on success and a negative rt_status on
 * failure; rt_last_error() returns a thread-local message for the last failure.
 *
 * Arithmetic contract: IEEE f64, no FMA contraction, correctly-rounded sqrt/div, in the exact
 * operation order of the reference.  The only deviation from the reference is the
 * RNG stream layout: the reference draws every random number from ONE sequential Xoshiro256++
 * stream (Scene.zig:29-38), which cannot be parallelised; here every (pixel, sample) owns its own
 * Xoshiro256++ stream (same generator, same Random.float(f64) conversion) keyed by
 * rt_sample_key(seed, pixel, sample).  See DESIGN.md "RNG".
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3
/* uint64 words of the d_stats buffer of an instrumented render (rt_context_enable_profile) */
#define RT_PROFILE_STATS_WORDS 72

/* ---- status codes ---------------------------------------------------------------------------- */
typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,   /* bad argument (n==0, W/H/spp==0, bad material, non-finite camera...) */
    RT_ERR_HIP = -2,       /* HIP runtime error (message in rt_last_error) */
    RT_ERR_NO_DEVICE = -3, /* no gfx950 device visible / extension not built for it */
    RT_ERR_CAPACITY = -4,  /* too large: > 2^24 spheres, or a launch with >= 2^32 work units */
    RT_ERR_IO = -5         /* file I/O (PPM writer) */
} rt_status;

/* ---- materials: tag of the reference's `Material` union (material.zig:113-117) ---------------- */
typedef enum rt_material_kind {
    RT_LAMBERTIAN = 0, /* Lambertian.scatter  material.zig:27-39 */
    RT_METAL = 1,      /* Metal.scatter       material.zig:55-68 */
    RT_DIELECTRIC = 2  /* Dielectric.scatter  material.zig:82-103 */
} rt_material_kind;

/* One Hittable (only `.sphere` exists, hittable.zig:22-27).  Replaces Sphere{center, radius, mat}
 * (sphere.zig:13-16).  The Material's `*DefaultPrng` pointer does not cross the boundary.
 * `radius` is stored as given; like Sphere.init (sphere.zig:21) the library clamps it to >= 0. */
typedef struct rt_sphere {
    double center[3];
    double radius;
    uint32_t material;        /* rt_material_kind */
    uint32_t reserved;        /* must be 0 */
    double albedo[3];         /* Lambertian/Metal albedo (material.zig:17,43) */
    double fuzz;              /* Metal.fuzz (material.zig:45) */
    double refraction_index;  /* Dielectric.refractionIndex (material.zig:72) */
} rt_sphere;                  /* 80 bytes */

/* The built Camera (camera.zig:82-103 after CameraBuilder.build camera.zig:300-345) plus the scene
 * fields render() reads (Scene.interval Scene.zig:21, Scene.seed Scene.zig:19). */
typedef struct rt_camera {
    uint32_t image_width;        /* Image.width  (camera.zig:27) */
    uint32_t image_height;       /* Image.height (camera.zig:28), already trunc(W/ratio), >= 1 */
    uint32_t samples_per_pixel;  /* Camera.samplesPerPixel (camera.zig:88) */
    uint32_t bounce_max;         /* Camera.bounceMax (camera.zig:90) */
    double pixel_samples_scale;  /* Camera.pixelSamplesScale = 1.0/spp (camera.zig:89,284) */
    double center[3];            /* Camera.center */
    double pixel0[3];            /* Camera.pixel0 */
    double du[3];                /* Camera.du */
    double dv[3];                /* Camera.dv */
    double defocus_disk_u[3];    /* Camera.defocusDiskU */
    double defocus_disk_v[3];    /* Camera.defocusDiskV */
    double defocus_angle;        /* Camera.defocusAngle (degrees; <= 0 disables the disk) */
    double t_min;                /* Scene.interval.min (1e-3) */
    double t_max;                /* Scene.interval.max (+inf) */
    uint64_t seed;               /* Scene.seed (the shim draws one from scene.prng when null) */
} rt_camera;

/* Options for one render call. */
typedef enum rt_output_format {
    RT_OUT_LINEAR_F64 = 0, /* ppm.pixels: linear Color per pixel (camera.zig:137-138) */
    RT_OUT_RGB8 = 1        /* fused Color.toRgb (color.zig:63-80): 3 bytes per pixel */
} rt_output_format;

/* Arithmetic of the sampling kernel. */
typedef enum rt_precision {
    RT_PRECISION_F64 = 0,  /* parity: the reference's f64 arithmetic bit for bit (default) */
    RT_PRECISION_F32 = 1   /* fast: f32 shading / sampling / intersection (huge spheres in f64);
                              statistical parity only (DESIGN.md "Fast mode") */
} rt_precision;

typedef struct rt_options {
    int32_t n_gpus;        /* 0 => all visible devices; rows are interleaved j mod n_gpus */
    int32_t device;        /* first device ordinal used */
    uint32_t pixel_stride; /* LINEAR_F64 only: doubles between pixels; 0 => 3. Zig's
                              @Vector(3,f64) has stride 4 (32 bytes), so the shim passes 4 */
    uint32_t output_format;/* rt_output_format */
    uint32_t precision;    /* rt_precision (0 = parity) */
    uint32_t reserved;     /* must be 0 */
    uint64_t* stats_out;   /* optional: [0] = rays traced (world.hit calls), [1] = samples */
} rt_options;

/* ---- the drop-in: Camera.render() ------------------------------------------------------------ */
/* Renders the whole image into host memory `out` (row-major, j*W+i).  LINEAR_F64: W*H pixels of
 * `pixel_stride` doubles (first 3 are r,g,b); RGB8: W*H*3 bytes.  Blocks the calling thread.
 * The library keeps one device context per GPU for the life of the process (created on first use,
 * on parallel host threads): a later call on the same sphere list re-uploads and rebuilds nothing.
 * Calls are serialised by an internal lock.
 *
 * Workspace (per device, held by the cached context; rt_context_workspace_bytes reports it).  A
 * context holds the buffers of ONE of two modes at a time (switching frees the other's):
 *   ring mode (launches whose samples need more than 2 GiB, e.g. config 4's full 1200x800x500
 *   frame on one GPU): one 144-KiB ring per resident wave of the launched kernel (the BVH kernels
 *   run 16 waves per CU: 576 MiB on a 256-CU MI355X) + 24 B of running sum per pixel + 4 B of flag
 *   per 64 pixels — config 4: 576 MiB + 22 MiB;
 *   direct mode (smaller launches: a rank's rows of a multi-GPU job, the 400x225 book scenes): every
 *   sample's colour, P x spp x 24 B (at most 2 GiB; a rank's 100 rows of config 4 at N = 8:
 *   1.34 GiB), summed in order by a second pass.
 * A buffer more than 25% larger than the current launch needs is given back and reallocated.
 * Plus the framebuffer rows (W x rows x 24 B) and the scene (≈ 100 KB for 485 spheres). */
int rt_render(const rt_camera* cam, const rt_sphere* spheres, size_t n_spheres,
              const rt_options* opts, void* out);
/* Frees rt_render's cached device contexts (optional; the next rt_render creates them again). */
int rt_release_cached_contexts(void);

/* ---- device-resident path (bench / multi-process drivers) ------------------------------------ */
typedef struct rt_context rt_context;

int rt_context_create(int device, rt_context** out_ctx);
/* Runs a pending deferred reduce pass, waits for every launch and pass of the context, then frees
 * it.  Returns the flush's status (the context is freed either way). */
int rt_context_destroy(rt_context* ctx);
/* Uploads the Hittable list to the context's device (once per scene). */
int rt_context_set_scene(rt_context* ctx, const rt_sphere* spheres, size_t n_spheres);
/* Renders rows j = row0 + k*row_step, k in [0, n_rows), into DEVICE memory `d_out`
 * (n_rows*W pixels; LINEAR_F64 stride 3 doubles, or RGB8) on HIP stream `stream` (NULL = default).
 * Asynchronous: returns after the launches; the output is complete when `stream` reaches the point
 * of the call.  `d_stats` (device, 2 x uint64, may be NULL) is atomically incremented with
 * {rays, samples}.  One kernel launch per call.  A context is not re-entrant: calls on one context
 * must come from one host thread at a time; a call on a different stream than the previous one
 * waits for the previous call's work, and scene changes / buffer growth wait for it on the host.
 * A call of at least 2^25 samples on a scene of at least 32 spheres with a camera the context's
 * tree was not built for first rebuilds the BVH from sample rays of that camera (host work,
 * ≈16 ms for the final scene, memoised per process; it waits for the previous call on the host).
 * Any tree gives the same bits; this one only walks faster for that camera. */
int rt_render_rows_async(rt_context* ctx, const rt_camera* cam, uint32_t output_format,
                         uint32_t row0, uint32_t row_step, uint32_t n_rows,
                         void* d_out, void* d_stats, void* stream);
/* The same render with the output completed on a second stream `out_stream` instead of `stream`
 * (frame pipelining for multi-frame drivers, e.g. bench.py's N > 1 path, which gathers each frame
 * on its collective stream): the sample kernel runs on `stream`; `out_stream` waits for it, and a
 * direct-mode call (small launches: a rank's rows of a multi-GPU job) runs its reduce pass there.
 * The context then alternates two per-sample buffers, so the next call's sample kernel on `stream`
 * does not wait for this call's reduce pass — the pass (HBM-bound, ≈0.25 ms at rank 0 of 8 on
 * config 4) overlaps the next sample kernel.  The output, and `d_stats`, are complete when
 * `out_stream` reaches the point of the call.  Either stream may be NULL (the HIP null stream);
 * out_stream == stream: rt_render_rows_async.
 * Workspace: twice direct mode's per-sample buffer. */
int rt_render_rows_async_split(rt_context* ctx, const rt_camera* cam, uint32_t output_format,
                               uint32_t row0, uint32_t row_step, uint32_t n_rows,
                               void* d_out, void* d_stats, void* stream, void* out_stream);
/* Deferred variant for frame pipelines (bench.py's N > 1 loop): like the split call, but a
 * direct-mode call's reduce pass is left PENDING — the next deferred call's sample kernel folds it
 * (one wave per block starts on it before tracing; the waves that run out of items while a few long
 * paths finish take the rest) and completes it before the kernel ends; with profiling enabled the
 * instrumented kernel does not fold, and a pass on that call's out_stream runs it after the kernel.
 * So the output of call k is complete on ITS out_stream once call k+1 has been issued and its
 * out_stream reaches that point, or after rt_context_flush(ctx) / rt_context_sync(ctx), which run a
 * pending pass whole.  A call that cannot fold the pending pass (a plain or ring-mode call, another
 * launch size, or another out_stream than the pending call's) runs it first.  Ring-mode calls behave
 * as rt_render_rows_async_split.  out_stream (NULL: the HIP null stream) must differ from stream.
 * rt_context_destroy runs a pending pass and waits for it before freeing anything: the output of
 * the last deferred call is complete when destroy returns (RT_OK), never dropped. */
int rt_render_rows_async_deferred(rt_context* ctx, const rt_camera* cam, uint32_t output_format,
                                  uint32_t row0, uint32_t row_step, uint32_t n_rows,
                                  void* d_out, void* d_stats, void* stream, void* out_stream);
/* ---- progressive rendering: sample ranges accumulated bit-exactly ------------------------------
 * Renders samples [sample_begin, sample_begin + sample_count) of rows row0 + k*row_step, k < n_rows,
 * and adds each pixel's colours, in sample order, to the UNSCALED running sums in DEVICE memory
 * d_accum (n_rows*W pixels x 3 doubles).  sample_begin == 0 starts a new image: d_accum's previous
 * contents are ignored and overwritten (it need not be initialised).  sample_begin > 0 continues
 * from the sums a previous call left there.  cam->samples_per_pixel and pixel_samples_scale are
 * not used.  Asynchronous on `stream`; d_stats as rt_render_rows_async.  One sample-kernel launch.
 *
 * Bits: the reference adds a pixel's samples strictly in sample order and scales once at the end
 * (camera.zig:133-137), and a sample's stream key (seed, pixel, sample) does not depend on the
 * sample count.  So for ANY split of [0, n) into consecutive calls on one d_accum, in either unit
 * mode and in any mix of them, rt_accum_resolve(n) is bit-identical to rt_render_rows_async at
 * samples_per_pixel = n (RT_PRECISION_F32 contexts: to the one-pass fast render at n), and the
 * {rays, samples} the passes add to d_stats sum to the one-pass counts.  The accumulator is plain
 * data: copied to the host and back (or into another buffer) it resumes exactly.  Passes on one
 * d_accum must be ordered (one stream, or events); the caller keeps track of the samples done.
 *
 * sample_count == 0 or n_rows == 0: RT_OK, nothing is touched.  RT_ERR_INVALID: null ctx, cam or
 * d_accum; a row range past the image; sample_begin + sample_count > 2^32 - 1.  RT_ERR_CAPACITY:
 * too many work units, as rt_render_rows_async.
 *
 * Launch: a plain one-stream call — a pending deferred reduce pass runs first.  The unit mode is
 * chosen from the pass's own size (P x sample_count x 24 B; RTZIG_UNIT_MODE forces it), and the BVH
 * training from the pass's sample count (any tree gives the same bits).  In ring mode d_accum is
 * the kernel's running-sum buffer itself; in direct mode the reduce pass adds to it.  Timing
 * (rt_context_kernel_times*) and instrumented contexts (rt_context_enable_profile, 72-word d_stats)
 * work as for rt_render_rows_async.  Every pass pays a launch's ramp and tail. */
int rt_render_rows_accumulate(rt_context* ctx, const rt_camera* cam,
                              uint32_t row0, uint32_t row_step, uint32_t n_rows,
                              uint32_t sample_begin, uint32_t sample_count,
                              void* d_accum, void* d_stats, void* stream);
/* d_out[q] = d_accum[q] * (1.0 / n_samples) (camera.zig:284,137) for n_pixels pixels, linear f64
 * (3 doubles per pixel) or the fused Color.toRgb (3 bytes); asynchronous on `stream`.  d_accum is
 * not modified, so a caller can resolve a preview and go on accumulating.  n_pixels == 0: RT_OK.
 * RT_ERR_INVALID: null ctx, d_accum or d_out; n_samples == 0; a bad output_format;
 * n_pixels >= 2^32. */
int rt_accum_resolve(rt_context* ctx, const void* d_accum, uint64_t n_pixels, uint32_t n_samples,
                     uint32_t output_format, void* d_out, void* stream);
/* ---- adaptive sampling: samples added to chosen pixels, bit-exactly -----------
 * A gather pass.  d_pixels: n_pixels image-global pixel indices j*W + i in DEVICE memory, in any
 * order, each < W*H and pairwise distinct (a caller contract, like the validity of a pointer); NULL
 * means every pixel, and then n_pixels must be W*H.  d_accum: [W*H][3] f64 unscaled sums, the buffer
 * (meaning and bits) of rt_render_rows_accumulate for the whole image.  d_counts: [W*H] u32 samples
 * done per pixel; the caller zeroes it for a new image.  d_m2: [W*H] f64, may be NULL: the per-pixel
 * sum of squared sample luminance.
 * Per listed pixel p, with b = counts[p]: samples [b, b + sample_count) are rendered with their usual
 * stream keys and their colours added, in sample order, to accum[p]; if d_m2 is given, y*y with
 * y = (r + g) + b is added to m2[p] in the same order (no weights, no fused multiply-add); then
 * counts[p] = b + sample_count.  A pixel with b == 0 starts from 0: its accum and m2 entries are
 * overwritten, not read, and need not be initialised.  Pixels not listed are not touched in any buffer.
 * So after any sequence of passes every pixel's sums are those of a one-pass render at that pixel's
 * own count: rt_accum_resolve_counts gives, per pixel, the bits of rt_render_rows_async at
 * samples_per_pixel = counts[p] (RT_PRECISION_F32 contexts: of the one-pass fast render).  An
 * accumulator that row passes brought to n samples continues here once counts is filled with n.
 *
 * Asynchronous on `stream`; d_stats (2 x uint64) as elsewhere.  A plain one-stream call: a pending
 * deferred reduce pass runs first.  Always direct mode: the pass's sample buffer is
 * n_pixels x sample_count x 24 B, and a pass above the 2-GiB cap (RTZIG_GATHER_BYTES, read per call,
 * lowers it) is split by the library into consecutive sub-passes over the same list; counts carries
 * the position between them.  The buffer is not given back when a later pass needs less (an adaptive
 * loop's lists shrink; the next row render applies the workspace rule).  BVH training and tree choice follow n_pixels x sample_count; timing
 * (rt_context_kernel_times*) covers every sub-pass.  cam->samples_per_pixel and pixel_samples_scale
 * are unused.  sample_count == 0 or n_pixels == 0: RT_OK, nothing is touched.
 * RT_ERR_INVALID: null ctx, cam, d_accum or d_counts; a NULL list with n_pixels != W*H;
 * n_pixels > W*H; an instrumented context (rt_context_enable_profile: gather passes have no
 * instrumented kernel).  RT_ERR_CAPACITY: one sample of the list alone does not fit the buffer. */
int rt_render_pixels_accumulate(rt_context* ctx, const rt_camera* cam,
                                const uint32_t* d_pixels, uint32_t n_pixels,
                                uint32_t sample_count,
                                void* d_accum, void* d_m2, uint32_t* d_counts,
                                void* d_stats, void* stream);
/* The noise estimate and the ordered selection.  Per pixel, in f64, in exactly this order:
 *   n = (double)counts[p];  S = (a0 + a1) + a2;  mean = S / n;  v = m2 - S * mean;
 *   v = v < 0 ? 0 : v;  sem = sqrt((v / (n - 1)) / n);  err = sem / (mean > floor ? mean : floor)
 * A pixel is selected when counts < min_count, or when counts < max_count && !(err <= tolerance)
 * (a NaN error keeps sampling until max_count).  The selected indices go to d_list (capacity
 * n_pixels) in ASCENDING order and their number to *d_n; entries of d_list past *d_n are
 * unspecified.  d_err (may be NULL) receives err for every pixel, 0 where counts < 2.
 * Asynchronous on `stream`; three small launches, none waiting on another block.  n_pixels == 0:
 * *d_n = 0.
 * RT_ERR_INVALID: null ctx, d_accum, d_m2, d_counts, d_list or d_n; min_count < 2;
 * max_count < min_count; n_pixels >= 2^32; floor not > 0; tolerance NaN. */
int rt_accum_select(rt_context* ctx, const void* d_accum, const void* d_m2,
                    const uint32_t* d_counts, uint64_t n_pixels,
                    uint32_t min_count, uint32_t max_count,
                    double tolerance, double floor,
                    uint32_t* d_list, uint32_t* d_n, double* d_err, void* stream);
/* d_out[p] = d_accum[p] * (1.0 / (double)counts[p]) (camera.zig:284,137), 0 for a pixel with
 * counts[p] == 0; linear f64 or the fused Color.toRgb.  Errors as rt_accum_resolve (and null
 * d_counts). */
int rt_accum_resolve_counts(rt_context* ctx, const void* d_accum, const uint32_t* d_counts,
                            uint64_t n_pixels, uint32_t output_format, void* d_out, void* stream);
/* ---- feature buffers: first-hit albedo, normal, depth and coverage per pixel ---
 * The auxiliary buffers a denoiser or compositor is guided by, accumulated like colour.  For pixel
 * p = j*W + i and sample s the feature ray is the ray getRay (camera.zig:187-215) produces from the
 * stream rt_sample_key(seed, p, s): two sampleSquare draws, then the defocus disk's rejection draws
 * when defocus_angle > 0 — bit for bit the camera ray of colour sample s in a parity (f64) render.
 * Its closest hit in (t_min, t_max) is HittableList.hit's (ties: the lower sphere index).  A sample
 * that hits contributes
 *   albedo: the attenuation scatter would apply — the sphere's albedo for Lambertian and Metal
 *           (material.zig:27-39, 55-68), (1, 1, 1) for Dielectric (:82-110); no random draw is made;
 *   normal: the hit record's normal after setFaceNormal (sphere.zig:44-53):
 *           outward = (point - center) * inv_r, negated when dot(dir, outward) >= 0;
 *   depth:  the Euclidean distance t * sqrt(lenSquared(dir)), lenSquared = (x*x + y*y) + z*z, a
 *           correctly rounded sqrt, no fused multiply-add;
 *   hit:    1.
 * A sample that misses contributes exactly nothing (the sky is an analytic function of the ray; a
 * colour render at bounce_max = 1 gives its per-pixel mean).  Per pixel the samples' values are
 * added, in sample order, to UNSCALED sums in DEVICE memory, indexed by the local pixel k*W + i of
 * rows j = row0 + k*row_step, k < n_rows: d_albedo [P][3] f64, d_normal [P][3] f64, d_depth [P] f64,
 * d_hits [P] u32.  d_albedo and d_normal have the layout of the colour accumulator:
 * rt_accum_resolve scales them or packs them to RGB8.  Mean depth is depth / hits, coverage
 * hits / samples.
 *
 * sample_begin == 0 starts a new image: the buffers are overwritten, not read, and need not be
 * initialised.  sample_begin > 0 continues from the stored sums.  Any split of [0, n) into
 * consecutive calls leaves, in all four buffers, the bits of the one call [0, n); the result does
 * not depend on row_step, on which walk ran or on which tree the context holds.  Each of the four
 * pointers may be NULL: that buffer is skipped.  All four NULL: RT_OK, no launch.
 * sample_count == 0 or n_rows == 0: RT_OK, nothing is touched.  RT_ERR_INVALID: null ctx or cam; a
 * row range past the image; sample_begin + sample_count > 2^32 - 1.  cam->samples_per_pixel,
 * pixel_samples_scale and bounce_max are not used.
 *
 * Precision: the pass always uses parity arithmetic and the parity stream, whatever
 * rt_context_set_precision says — on an RT_PRECISION_F32 context the feature rays are those of the
 * f64 render, not of the fast render's own stream.  Instrumented contexts are accepted; the pass
 * has no instrumented form and writes no stats.
 *
 * Launch: asynchronous on `stream`, one kernel, a plain one-stream call (a pending deferred reduce
 * pass runs first).  It walks the structure the context holds now (rt_context_tree_info) and never
 * rebuilds or retrains the BVH; it uses no per-sample workspace.  rt_context_kernel_times reports
 * the pass as sample_ms, with reduce_ms 0.  Passes on one set of buffers must be ordered. */
int rt_render_rows_features(rt_context* ctx, const rt_camera* cam,
                            uint32_t row0, uint32_t row_step, uint32_t n_rows,
                            uint32_t sample_begin, uint32_t sample_count,
                            void* d_albedo, void* d_normal, void* d_depth, uint32_t* d_hits,
                            void* stream);
/* ---- denoise: a variance- and feature-guided à-trous filter, bit-exact to its spec
 * Turns the buffers of an every-pixel gather pass (rt_render_pixels_accumulate with a NULL list: the
 * unscaled colour sums, the squared-luminance sums m2, the counts) and of a feature pass over all rows
 * (rt_render_rows_features) into a clean image.  Every operation below is IEEE f64, correctly rounded,
 * with no fused multiply-add and no transcendental function, in exactly this order, so the result
 * depends on nothing but the buffers and the parameters — not on tile shape, launch shape or which
 * kernel form ran a level.  P = W*H, pixel p = j*W + i.
 *
 * Prepare, per pixel, n = (double)counts[p]:
 *   colour    c_k = accum[p][k] * (1.0 / n), 0 when counts[p] == 0 (rt_accum_resolve_counts' bits);
 *   variance  of the mean luminance: S = (a0 + a1) + a2; mean = S / n; v = m2[p] - S * mean;
 *             var = v > 0 ? (v / (n - 1)) / n : 0; var = 0 when counts[p] < 2;
 *   guides    fi = 1.0 / (double)feature_samples: A_k = albedo[p][k] * fi; N_k = normal[p][k] * fi (not
 *             renormalised); h = (double)hits[p]; cov = h * fi; z = hits[p] ? depth[p] / h : 0.
 *             A guide whose pointer is NULL is 0 everywhere: its term vanishes.
 * Variance prefilter, once: 3x3, taps ty = -1..1 outer, tx = -1..1 inner, only taps inside the image:
 *   g = G[ty] * G[tx], G = {0.25, 0.5, 0.25}; sv += g * var_q; sg += g; then v0 = sv / sg.
 * Level k = 0 .. levels - 1, step s = 2^k, reads (c, v) of the previous level and writes (c', v'):
 *   l_p = (c0 + c1) + c2 (likewise l_q); isd = 1.0 / (sigma_l * sqrt(v_p) + epsilon);
 *   sw = 0; sc[3] = 0; sv = 0;
 *   for ty = -2..2 (outer), tx = -2..2 (inner), q = (i + tx*s, j + ty*s), skipped outside the image:
 *     dl = |l_p - l_q| * isd
 *     dn = sigma_n * (((Np0-Nq0)^2 + (Np1-Nq1)^2) + (Np2-Nq2)^2)          x^2 is x * x
 *     da = sigma_a * (((Ap0-Aq0)^2 + (Ap1-Aq1)^2) + (Ap2-Aq2)^2)
 *     dh = sigma_h * |cov_p - cov_q|
 *     r  = (double)(max(|tx|, |ty|) * s)
 *     dz = (r > 0 && z_p > 0 && z_q > 0) ? |z_p - z_q| / ((sigma_z * r) * (z_p + z_q) + epsilon) : 0
 *     d  = ((dl + dn) + da) + (dh + dz)
 *     x  = 1.0 - d * 0.125; t = x > 0 ? x : 0; t = t*t; t = t*t; t = t*t     (1 - d/8)^8 for exp(-d)
 *     w  = t * (K[ty] * K[tx]), K = {1, 4, 6, 4, 1} / 16 (the product is exact)
 *     sw += w; sc_k += w * c_q,k; sv += (w * w) * v_q
 *   rs = 1.0 / sw; c'_k = sc_k * rs; v' = sv * (rs * rs)
 * The centre tap has d = 0, so sw >= 36/256.  d_out receives the last level's c, linear f64 (3 doubles
 * per pixel) or the fused Color.toRgb (3 bytes); d_var_out (P doubles, may be NULL) the last level's v.
 * levels == 0: the prepared colour and the prefiltered variance.
 *
 * params == NULL: rt_denoise_default_params' values (levels 2, sigma_l 4, sigma_n 32, sigma_a 32,
 * sigma_z 0.05, sigma_h 4, epsilon 1e-6).  Finite sums are a caller contract: with a NaN or infinite
 * input the output is unspecified, but the call neither faults nor hangs.  The inputs are not
 * modified; d_out and d_var_out must not alias them.
 *
 * Launch: asynchronous on `stream`; a plain one-stream call (a pending deferred reduce pass runs
 * first): a prepare pass, the prefilter and one kernel per level.  Workspace: 128 B per pixel, held by
 * the context (rt_context_workspace_bytes counts it; the 25% give-back rule applies).
 * rt_context_kernel_times reports the whole call as sample_ms, with reduce_ms 0.  Instrumented
 * contexts are accepted; the call writes no stats.
 * RT_ERR_INVALID, each answered before any device is touched: null ctx, d_accum, d_m2, d_counts or
 * d_out; width or height 0, or W*H >= 2^32; d_depth without d_hits; a guide pointer with
 * feature_samples == 0; levels > 16; a sigma that is negative or NaN; epsilon not > 0;
 * reserved != 0; a bad output_format. */
typedef struct rt_denoise_params {
    uint32_t levels;     /* à-trous levels, step 2^k at level k; at most 16 */
    uint32_t reserved;   /* must be 0 */
    double sigma_l;      /* luminance, in standard deviations of the pixel's mean */
    double sigma_n;      /* squared normal distance */
    double sigma_a;      /* squared albedo distance */
    double sigma_z;      /* relative depth difference per pixel of tap distance */
    double sigma_h;      /* coverage difference */
    double epsilon;      /* added to both denominators; > 0 */
} rt_denoise_params;     /* 56 bytes */
int rt_denoise_default_params(rt_denoise_params* out);
int rt_denoise(rt_context* ctx, uint32_t width, uint32_t height,
               const void* d_accum, const void* d_m2, const uint32_t* d_counts,
               const void* d_albedo, const void* d_normal, const void* d_depth,
               const uint32_t* d_hits, uint32_t feature_samples,
               const rt_denoise_params* params, uint32_t output_format,
               void* d_out, void* d_var_out, void* stream);
/* ---- temporal accumulation: the previous frame's sums reprojected into the next ---
 * For a static scene seen by a moving camera.  `prev` holds the previous frame's buffers — the unscaled
 * colour sums, m2 and counts of an every-pixel gather pass (rt_render_pixels_accumulate, NULL list) and
 * the sums of a feature pass over all rows (rt_render_rows_features) at prev->feature_samples samples,
 * rendered with cam_prev — and `cur` the current frame's, freshly rendered with cam.  For every pixel the
 * call finds where the pixel's first-hit point was in the previous image, checks that the previous image
 * saw the same surface there, and if so adds the previous frame's per-sample means to the current sums
 * as nh pseudo-samples.  The merged (accum, m2, counts) are at once rt_denoise's input and the next
 * frame's history: there is no separate history format.  Only the first frame of a sequence is
 * bit-identical to a one-pass render at its counts; a merged pixel's sums are an estimate that mixes
 * two frames, and rt_accum_resolve_counts gives its blended mean.
 *
 * Every operation below is IEEE f64, correctly rounded, with no fused multiply-add and no
 * transcendental function, in exactly this order; every comparison is written so that a NaN makes it
 * false.  dot(x,y) = (x0*y0 + x1*y1) + x2*y2; cross(a,b) = (a1*b2 - a2*b1, a2*b0 - a0*b2,
 * a0*b1 - a1*b0); x^2 is x*x.  Primed names belong to cam_prev / prev.  P = W*H, pixel p = j*W + i.
 *
 * Per call, from cam_prev:  A = pixel0' - center';  n = cross(du', dv');  an = dot(A, n);
 *   nn = dot(n, n);  rnn = 1.0 / nn.
 * Per pixel p = (i, j), c = counts[p], h = hits[p]:
 *  1. h == 0: no history (the sky is an analytic function of the ray; there is no point to reproject).
 *  2. The first-hit point.  z = depth[p] / (double)h;
 *     D_k = ((pixel0_k + du_k*(double)i) + dv_k*(double)j) - center_k   (getRay's order, camera.zig:189,198,
 *     with a zero offset; pixel centres lie at integer coordinates, camera.zig:318);
 *     L = sqrt(dot(D,D));  g = z / L;  X_k = center_k + D_k*g.
 *  3. Its place in the previous image.  E = X - center';  en = dot(E,n);  s = an / en; the point lies in
 *     front of the previous camera iff s > 0 && s < +inf, else no history.  Q_k = s*E_k - A_k;
 *     u = dot(cross(Q, dv'), n) * rnn;  v = dot(cross(du', Q), n) * rnn;  r = sqrt(dot(E,E)).
 *  4. The taps.  fu = floor(u), fv = floor(v); in range iff fu >= -1 && fu <= W-1 && fv >= -1 &&
 *     fv <= H-1, else no history; only then are they converted to integers i0, j0.  fx = u - fu, fy = v - fv.
 *  5. For b = 0,1 (outer), a = 0,1 (inner): q = (i0+a, j0+b), skipped outside the image;
 *     bw = (a ? fx : 1.0 - fx) * (b ? fy : 1.0 - fy); the tap is skipped when bw == 0.  It is VALID iff
 *       counts'[q] > 0 && hits'[q] > 0;
 *       |z_q - r| <= sigma_z * r, with z_q = depth'[q] / (double)hits'[q];
 *       dn <= tau_n, dn = ((Np0-Nq0)^2 + (Np1-Nq1)^2) + (Np2-Nq2)^2, N = normal * fi,
 *         fi = 1.0 / (double)feature_samples (each frame its own);
 *       da <= tau_a, the same on albedo;
 *       |cov_p - cov_q| <= tau_h, cov = (double)hits * fi.
 *     A guide that is NULL contributes no test.  A valid tap adds, with rn = 1.0 / (double)counts'[q]:
 *       sw += bw;  sc_k += bw * (accum'[q][k] * rn);  sq += bw * (m2'[q] * rn);  nmin = min(nmin, counts'[q]).
 *  6. History is taken iff at least one tap was valid and sw >= min_weight.  Then
 *     nh = min(nmin, max_history, 2^32 - 1 - c); nh == 0: no history.  rs = 1.0 / sw; hd = (double)nh;
 *       accum[p][k] = (c ? accum[p][k] : 0) + (sc_k*rs)*hd;   m2[p] = (c ? m2[p] : 0) + (sq*rs)*hd;
 *       counts[p] = c + nh;   d_history[p] = nh.
 *     Without history d_history[p] = 0 and no byte of `cur` at that pixel is written.  A pixel with
 *     c == 0 starts from 0: its accum and m2 entries are not read.
 * m2 is a sum of squared sample luminances, and the history's mean second moment times nh is the same
 * kind of quantity: the variance estimates of rt_accum_select and rt_denoise keep their meaning on merged
 * buffers.  In the steady state a pixel carries n + max_history samples, so max_history is the blend
 * factor: alpha = n / (n + max_history).
 *
 * params == NULL: rt_temporal_default_params' values (max_history 64, sigma_z 0.05, tau_n 0.1,
 * tau_a 0.05, tau_h 0.5, min_weight 0.25).  d_history ([P] u32) may be NULL.  `prev` is only read.
 *
 * Launch: asynchronous on `stream`, one kernel, a plain one-stream call (a pending deferred reduce pass
 * runs first).  No workspace, no stats.  rt_context_kernel_times reports it as sample_ms, with reduce_ms
 * 0.  The context's precision setting has no effect.
 * RT_ERR_INVALID, each answered before any device is touched: null ctx, cam, cam_prev, cur or prev; a
 * null accum, m2, counts, depth or hits in either frame; albedo or normal given in one frame and NULL
 * in the other; feature_samples == 0 in either frame; image sizes that differ, are 0, or have
 * W*H >= 2^32; reserved != 0 (frames or params); max_history outside 1 .. 2^24; a negative or NaN
 * tolerance; min_weight outside (0, 1]; nn not positive and finite, or an == 0; cur and prev sharing
 * any buffer pointer. */
typedef struct rt_temporal_frame {  /* device pointers of one whole image */
    void* accum;                    /* [P][3] f64 */
    void* m2;                       /* [P] f64 */
    uint32_t* counts;               /* [P] u32 */
    const void* albedo;             /* [P][3] f64, may be NULL */
    const void* normal;             /* [P][3] f64, may be NULL */
    const void* depth;              /* [P] f64 */
    const uint32_t* hits;           /* [P] u32 */
    uint32_t feature_samples;       /* samples of the feature pass; > 0 */
    uint32_t reserved;              /* must be 0 */
} rt_temporal_frame;                /* 64 bytes */
typedef struct rt_temporal_params {
    uint32_t max_history;  /* cap on the pseudo-samples a pixel takes over; 1 .. 2^24 */
    uint32_t reserved;     /* must be 0 */
    double sigma_z;        /* relative depth tolerance, >= 0 */
    double tau_n;          /* max squared distance of the mean normals, >= 0 */
    double tau_a;          /* max squared distance of the mean albedos, >= 0 */
    double tau_h;          /* max coverage difference, >= 0 */
    double min_weight;     /* least sum of valid bilinear weights, in (0, 1] */
} rt_temporal_params;      /* 48 bytes */
int rt_temporal_default_params(rt_temporal_params* out);
int rt_temporal_accumulate(rt_context* ctx,
                           const rt_camera* cam, const rt_temporal_frame* cur,
                           const rt_camera* cam_prev, const rt_temporal_frame* prev,
                           const rt_temporal_params* params, uint32_t* d_history, void* stream);
/* ---- ray queries: the closest hit of caller-supplied rays, bit-exact --------------
 * HittableList.hit(ray, Interval(t_min, t_max)) (hittable.zig:64-77 over Sphere.hit, sphere.zig:26-54)
 * for n_rays rays in DEVICE memory, in the reference's f64 arithmetic, bit for bit.
 * d_origins, d_directions: f64, ray q at [q * ray_stride + 0..2]; ray_stride is in doubles, 0 means 3,
 * 4 is Zig's @Vector(3, f64); 1 and 2 are invalid.  Directions are used as given, not normalised.
 * d_intervals: NULL, or [n][2] f64 — ray q then uses (intervals[q][0], intervals[q][1]) in place of
 * (t_min, t_max).
 *
 * Per ray: the sphere with the smallest accepted root wins, the lowest index among equal roots;
 * Interval.surrounds is strict at both ends; a sphere's root is root1, else root2 (sphere.zig:38-42).
 * The record follows sphere.zig:44-53: point = orig + dir * t; outward = (point - center) * inv_r;
 * front = dot(dir, outward) < 0; normal = front ? outward : -outward.  Every non-NULL output is written
 * for every ray, so the buffers need not be initialised.  NaN and infinite components and intervals
 * are legal: the result is what the reference's comparisons give (a miss wherever a NaN decides), and
 * the call neither faults nor hangs.  Inputs and outputs must not alias.
 *
 * The arithmetic is always parity, whatever rt_context_set_precision says.  Instrumented contexts are
 * accepted.  The call walks the structure the context holds now (rt_context_tree_info) and never
 * rebuilds or trains it.  The tree's f32 boxes are used only for rays inside the domain they are
 * certified for (finite components, max|o_k| <= rt_context_origin_bound, max|d_k| in [2^-20, 2^20],
 * 0 <= t_min < +inf; csrc/rt_trace.h); every other ray is answered by the reference's own scan of the
 * whole list: the same bits, at the list's cost.
 *
 * d_stats (DEVICE, 2 x uint64, may be NULL) is atomically incremented: [0] by the number of rays, [1]
 * by the number of rays the list scan resolved (every ray when the context walks the list).
 *
 * Launch: asynchronous on `stream`, one kernel, a plain one-stream call (a pending deferred reduce pass
 * runs first).  No workspace.  rt_context_kernel_times reports it as sample_ms, with reduce_ms 0.
 * n_rays == 0: RT_OK, nothing is touched.  All five outputs NULL and d_stats NULL: RT_OK, no launch.
 * RT_ERR_INVALID, each answered before any device is touched: null d_origins, d_directions or out;
 * ray_stride 1 or 2; n_rays >= 2^32; null ctx; no scene uploaded. */
typedef struct rt_ray_hits {   /* DEVICE pointers; each may be NULL: that output is skipped */
    int32_t* index;            /* [n]    sphere index in rt_context_set_scene's list; -1: miss */
    double*  t;                /* [n]    the accepted root; +inf on a miss */
    double*  point;            /* [n][3] ray.at(t);            +0.0 on a miss */
    double*  normal;           /* [n][3] after setFaceNormal;  +0.0 on a miss */
    uint8_t* front;            /* [n]    1 iff dot(dir, outward) < 0; 0 on a miss */
} rt_ray_hits;                 /* 40 bytes */
int rt_trace_rays(rt_context* ctx, const void* d_origins, const void* d_directions,
                  uint32_t ray_stride, uint64_t n_rays, double t_min, double t_max,
                  const void* d_intervals, const rt_ray_hits* out, void* d_stats, void* stream);
/* ---- occlusion queries: any hit of caller-supplied rays, bit-exact ----------------
 * Ray q is OCCLUDED iff HittableList.hit(ray_q, Interval(t_min_q, t_max_q)) returns true in the
 * reference's f64 arithmetic — equivalently, iff some sphere's own Sphere.hit(ray, (t_min, t_max)) is
 * true (a sphere that the shrinking `closest` rejects is rejected only after another was accepted, and
 * an accepted root lies in (t_min, t_max) by the reference's strict comparisons).  So the answer equals
 * rt_trace_rays' index >= 0 for every input that call accepts — NaN, infinities, zero directions,
 * negative or inverted intervals, duplicate spheres and zero radii included — and no sphere order,
 * tree or early exit changes it.  The walk stops at the first accepted root, its interval never
 * shrinks, and it writes 1 byte and / or 1 bit per ray.
 *
 * d_origins, d_ends, ray_stride, d_intervals, t_min, t_max: exactly as rt_trace_rays (stride in doubles,
 * 0 means 3, 1 and 2 are invalid).  Without a flag d_ends holds directions, used as given.  With
 * RT_OCCLUSION_TARGETS it holds end points: the direction is end - origin, computed on the device with
 * one f64 subtraction per component, and the natural interval is (eps, 1.0), the open segment.
 * Interval.surrounds is strict, so an occluder whose root is exactly 1.0 — exactly at the end point —
 * does not count.  Any other flag bit: RT_ERR_INVALID (the message names `flags`).
 *
 * d_occluded ([n] uint8, may be NULL): 1 or 0 for every ray.
 * d_mask ([ceil(n / 64)] uint64, may be NULL): bit q & 63 of word q >> 6 is set iff ray q is occluded.
 *   Every word is written whole; the bits past n in the last word are 0; words past ceil(n / 64) are
 *   not touched.
 * d_stats (DEVICE, 3 x uint64, may be NULL) is atomically incremented: [0] rays, [1] rays the list scan
 *   resolved, [2] occluded rays.
 *
 * Always parity arithmetic; instrumented and RT_PRECISION_F32 contexts are accepted; the structure the
 * context holds is walked as it is, never rebuilt or trained.  The tree's domain rule is
 * rt_trace_rays' (csrc/rt_trace.h), applied to the ray as used: after the subtraction in targets mode.
 * Rays outside it are answered by an early-exit scan of the whole list: the same answer.
 *
 * Launch: asynchronous on `stream`, one kernel, a plain one-stream call, no workspace;
 * rt_context_kernel_times reports it as sample_ms, with reduce_ms 0.  n_rays == 0: RT_OK, nothing is
 * touched.  Both outputs NULL and d_stats NULL: RT_OK, no launch.
 * RT_ERR_INVALID, each answered before any device is touched: null d_origins or d_ends; ray_stride 1
 * or 2; n_rays >= 2^32; unknown flags; null ctx; no scene uploaded. */
#define RT_OCCLUSION_TARGETS 1u   /* d_ends holds end points: dir_k = end_k - origin_k, one f64 subtraction per component */
int rt_occluded_rays(rt_context* ctx, const void* d_origins, const void* d_ends,
                     uint32_t ray_stride, uint64_t n_rays, double t_min, double t_max,
                     const void* d_intervals, uint32_t flags,
                     uint8_t* d_occluded, uint64_t* d_mask, void* d_stats, void* stream);
/* ---- radiance queries: rayColor of caller-supplied rays, bit-exact ----------------
 * Camera.rayColor (camera.zig:148-183) — the bounce loop over HittableList.hit, Material.scatter and the
 * sky — for n_rays rays in DEVICE memory, in the reference's f64 arithmetic and draw order, bit for bit.
 * d_origins, d_directions, ray_stride: exactly as rt_trace_rays (f64, stride in doubles, 0 means 3, 1
 * and 2 invalid; directions used as given, not normalised).
 *
 * Per ray q and sample s in [sample_begin, sample_begin + sample_count): a fresh Xoshiro256++ stream is
 * seeded from rt_sample_key(seed, ray_base + q, s) — the renderer's key with the ray's id in the pixel's
 * place — and the colour is rayColor(ray_q) with bounceMax = bounce_max and Scene.interval = (t_min,
 * t_max) for every segment.  No draw is made before the first world.hit: the caller made the ray.
 * bounce_max == 0 gives black.  bounce_max is any uint32_t; the cost is proportional to it.
 *
 * d_sum ([n][3] f64, the colour accumulator's layout, may be NULL): the colours are added in sample
 * order to the unscaled sums, sum = sum + colour, one addition per component and sample.  sample_begin
 * == 0 starts a ray: its entry is overwritten and not read.  sample_begin > 0 continues from the stored
 * sums.  rt_accum_resolve scales the buffer or packs it to RGB8.  So
 *   - any split of [0, n) into consecutive calls leaves the bits of the one call;
 *   - any split of a batch into consecutive sub-batches with matching ray_base leaves the bits of the
 *     one batch;
 *   - no result depends on the grid, the tree, the kernel form or which lane ran a ray.
 *
 * d_states (DEVICE, [n][4] uint64, may be NULL): ray q's one sample uses these four words as its
 * Xoshiro256++ state in place of seeding from the key — how a caller who drew from a stream before the
 * ray existed hands the stream on, as the reference's getRay does to rayColor.  sample_count must be 1;
 * seed and ray_base are unused; sample_begin still decides overwrite or add.  Fed getRay's rays and the
 * states after getRay's draws, the call returns the renderer's own 1-spp image, bit for bit.  (An
 * all-zero state never leaves randomUnitVec's rejection loop, in the reference as here.)
 *
 * NaN and infinite components, zero directions and empty, negative or NaN intervals are legal: the
 * result is what the reference's operations give (a zero direction misses everything and its sky
 * colour is NaN), and the call neither faults nor hangs.
 *
 * d_stats (DEVICE, 3 x uint64, may be NULL) is atomically incremented: [0] paths (n_rays x
 * sample_count), [1] segments (the world.hit calls: exact and deterministic), [2] segments the list scan
 * resolved (every segment when the context walks the list).
 *
 * Always parity arithmetic, whatever rt_context_set_precision says; instrumented contexts are accepted;
 * the structure the context holds is walked as it is, never rebuilt or trained.  The tree's domain rule
 * is rt_trace_rays' (csrc/rt_trace.h), applied to every segment as used.
 *
 * Launch: asynchronous on `stream`, one kernel, a plain one-stream call (a pending deferred reduce pass
 * runs first), no workspace; rt_context_kernel_times reports it as sample_ms, with reduce_ms 0.
 * n_rays == 0 or sample_count == 0: RT_OK, nothing is touched.  d_sum and d_stats both NULL: RT_OK, no
 * launch.
 * RT_ERR_INVALID, each answered before any device is touched: null d_origins, d_directions or params;
 * ray_stride 1 or 2; reserved != 0; ray_base + n_rays > 2^32; sample_begin + sample_count > 2^32 - 1;
 * d_states with sample_count != 1; null ctx; no scene uploaded. */
typedef struct rt_radiance_params {
    uint64_t seed;          /* Scene.seed of the streams */
    uint64_t ray_base;      /* stream id of ray 0: ray q uses id ray_base + q */
    uint32_t sample_begin;  /* first sample of this call */
    uint32_t sample_count;  /* samples per ray in this call */
    uint32_t bounce_max;    /* Camera.bounceMax */
    uint32_t reserved;      /* must be 0 */
    double   t_min, t_max;  /* Scene.interval, used for every segment */
} rt_radiance_params;       /* 48 bytes */
int rt_radiance_rays(rt_context* ctx, const void* d_origins, const void* d_directions,
                     uint32_t ray_stride, uint64_t n_rays, const rt_radiance_params* params,
                     const void* d_states, void* d_sum, void* d_stats, void* stream);
/* The origin bound of the tree the context holds: rays starting within it (max|o_k| <= bound) may use
 * the tree; rays starting beyond it are exact but cost a scan of the whole list.  0 when the list walk
 * runs. */
int rt_context_origin_bound(rt_context* ctx, double* bound);
/* The remedy for that cost: with a finite bound greater than the current one, waits for the context's
 * work and rebuilds the tree for origins up to bound * 1.01 (host work; the path a far camera takes).
 * A smaller or equal bound, or a context without a tree, is a no-op.  It changes no result bit of any
 * call.  It drops a trained tree: the next large render retrains.  RT_ERR_INVALID: a non-finite or
 * non-positive bound; null ctx; no scene uploaded. */
int rt_context_reserve_origin_bound(rt_context* ctx, double bound);
/* Runs a pending deferred reduce pass (on the out_stream of the call that deferred it); no-op otherwise. */
int rt_context_flush(rt_context* ctx);
/* *pending = 1 if the last deferred call left its output pending (direct mode), else 0. */
int rt_context_fold_pending(rt_context* ctx, int* pending);
/* Waits for the context's last render (running a pending deferred reduce pass first) and reports a
 * failure the kernel recorded (RT_ERR_HIP: a wave gave up waiting for a running-sum hand-off — a bug
 * guard, never expected). */
int rt_context_sync(rt_context* ctx);
/* Arithmetic of the context's later renders: rt_precision (default RT_PRECISION_F64).  F32 needs
 * the BVH walk (any scene whose BVH builds); otherwise the parity kernel runs. */
int rt_context_set_precision(rt_context* ctx, int precision);
/* Name of the kernel variant the context launches (for profiling / logs). */
const char* rt_kernel_name(rt_context* ctx);
/* The closest-hit structure the context's next render walks (diagnostics / tests), info[6]:
 * {1 if the BVH walk runs (else the reference's list walk), tree nodes, leaves, depth, always-list
 * spheres, 1 if the tree was trained on the rays of the last large launch's camera (DESIGN.md §5.4:
 * same bits as any tree, fewer node visits)}. */
int rt_context_tree_info(rt_context* ctx, uint32_t* info);
/* Device bytes the context's render workspace holds now (rings, sums, flags, direct-mode samples,
 * schedule, counters, rt_accum_select's scratch, rt_denoise's planes; not the scene or caller buffers): see rt_render
 * "Workspace". */
int rt_context_workspace_bytes(rt_context* ctx, uint64_t* bytes);
/* Optional kernel timing with HIP events recorded on the launch stream around the kernels of every
 * render call.  rt_context_kernel_times waits for the last event and returns the durations (ms) of
 * the most recent rt_render_rows_async call: the sample kernel, and the reduce pass of direct mode
 * (small launches, see rt_render; ~0 when the sample kernel accumulated in order itself; for a split
 * call, from the point `out_stream` reaches the pass to its end). */
int rt_context_enable_timing(rt_context* ctx, int enable);
int rt_context_kernel_times(rt_context* ctx, double* sample_ms, double* reduce_ms);
/* The same summed over every call since timing was (re)enabled (at most 1024 calls; beyond that the
 * totals restart), so a caller can time many frames without a host sync per frame.
 * *n_launches = the number of sample-kernel launches summed. */
int rt_context_kernel_times_total(rt_context* ctx, double* sample_ms, double* reduce_ms, uint32_t* n_launches);
/* Instrumented kernels (diagnostics): when enabled, `d_stats` of rt_render_rows_async must hold
 * RT_PROFILE_STATS_WORDS (72) uint64: {rays, samples, sphere tests executed, BVH node visits, wave-cycles in queue refill,
 * wave-cycles in the closest-hit walk, wave-cycles in shading, wave-iterations of the BVH inner
 * (internal-node) loop, wave-iterations of BVH leaf rounds, wave-level candidate blocks (sqrt +
 * root division), wave-level second-root divisions, node visits of camera rays, sphere tests of
 * camera rays, [13..15] kernel timeline stamps, [16] wave-cycles in the rejection-trip loop,
 * [17] idle sleeps of waves waiting on a hand-off, [18] deferred unit finalisations (previous chunk
 * of the tile not yet finalised), [19] refills that found no free ring slot, [20] / [21] sum / max over
 * waves of (wave end - the wave's first empty claim), [22] the last wave's first empty claim, [23..25]
 * the parts of [4]: wave-cycles finalising units, handing out items (claims), seeding + getRay;
 * [26..31] wave-level executions: loop iterations, rejection trips, seeding blocks, walks started
 * (always-list tests), shading blocks, unit finalisations; then lane-level executions (the active
 * lanes summed over every wave-level execution of a block) and the wave-level executions they pair
 * with: [32] seeding lanes, [33] rejection-trip lanes, [34] / [35] scatter-finish waves / lanes,
 * [36] / [37] defocus camera-finish waves / lanes, [38] / [39] walk waves / lanes (resumed walks
 * included), [40] walk-start lanes, [41] shading lanes, [42..47] waves / lanes of the sky, Lambertian
 * + metal and dielectric shading branches, [48] / [49] store waves / lanes, [50] lanes holding a path
 * after the hand-out (per iteration), [51] leaf-round lanes, [52] candidate-block lanes, [53]
 * second-root lanes, [54..57] / [58..61] always-list candidate blocks per always-list slot 0..3, waves
 * / lanes, [62] / [63] always-list second-root waves / lanes, [64] / [65] seed-window fills / take
 * passes (RTZIG_SEED_WIN builds), [66..71] unused}.  Counts 0-3 are exact and
 * deterministic; the cycles, wave-level and lane-level counts are diagnostics. */
int rt_context_enable_profile(rt_context* ctx, int enable);

/* ---- host mirror of the reference's Scene / CameraBuilder / Color / PPM ---------------------- */
/* Scene.generateWorld (Scene.zig:48-134) driven by DefaultPrng.init(seed) (Scene.zig:30).
 * Writes up to `cap` spheres, stores the count in *n (485 for seed 0xdeadbeef).  If `prng_state`
 * is non-NULL it receives the 4 Xoshiro256++ words after generation (the reference's render()
 * continues that stream). */
int rt_scene_final(uint64_t seed, rt_sphere* out, size_t cap, size_t* n, uint64_t* prng_state);
/* Scene.generateChapter13 (Scene.zig:136-182): 5 spheres, no RNG. */
int rt_scene_chapter13(rt_sphere* out, size_t cap, size_t* n);

/* CameraBuilder inputs (camera.zig:233-251).  rt_camera_build applies them in the order main.zig
 * uses (setDefocusAngle, setFocusDist, setViewport, setSamplesPerPixel, setBounceMax): the viewport
 * is computed from focus_dist (camera.zig:277) and everything else as in build() (:300-345). */
typedef struct rt_camera_params {
    uint32_t image_width;
    uint32_t samples_per_pixel;
    uint32_t bounce_max;
    uint32_t reserved;
    double aspect_ratio;
    double look_from[3];
    double look_at[3];
    double v_up[3];
    double vfov;           /* degrees */
    double defocus_angle;  /* degrees */
    double focus_dist;
    double t_min, t_max;
    uint64_t seed;
} rt_camera_params;

int rt_camera_build(const rt_camera_params* params, rt_camera* out);
/* Color.toRgb (color.zig:63-76) for n linear pixels with the given stride (doubles). */
int rt_color_to_rgb8(const double* linear, size_t n_pixels, uint32_t pixel_stride, uint8_t* rgb);
/* PPM.saveBinary byte stream (ppm.zig:42-60): "P6\nW H\n255\n" + W*H*3 bytes + "\n".
 * rt_ppm_p6_size gives the byte count; rt_ppm_encode_p6 writes it into `buf`. */
size_t rt_ppm_p6_size(uint32_t width, uint32_t height);
int rt_ppm_encode_p6(const uint8_t* rgb, uint32_t width, uint32_t height, uint8_t* buf, size_t cap);
int rt_ppm_save_p6(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height);
/* PPM.save ASCII byte stream (ppm.zig:25-39, Color.format color.zig:82-87 -> RGB.format :13-18):
 * "P3\nW H\n255\n" then one "r g b\n" line per pixel, decimal, no padding.
 * rt_ppm_p3_size gives the exact byte count for these pixels; rt_ppm_encode_p3 writes the stream
 * into `buf` (cap >= that size). */
size_t rt_ppm_p3_size(const uint8_t* rgb, uint32_t width, uint32_t height);
int rt_ppm_encode_p3(const uint8_t* rgb, uint32_t width, uint32_t height, uint8_t* buf, size_t cap);
int rt_ppm_save_p3(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height);

/* Per-(pixel, sample) stream key (DESIGN.md "RNG"); exposed so host tools can reproduce it. */
uint64_t rt_sample_key(uint64_t seed, uint64_t pixel, uint64_t sample);

const char* rt_last_error(void);
int rt_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_MI355X_H */

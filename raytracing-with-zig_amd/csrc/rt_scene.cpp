// rt_scene.cpp — host scene records, the device tree and its training (rt_scene.hpp).
#include "rt_scene.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <mutex>

namespace rtscene {

// Ray-driven tree (rtbvh::build with sample rays): trained for launches of at least
// kTrainMinSamples samples on scenes of at least kTrainMinSpheres spheres, from the paths of
// kTrainSamples camera samples.  Config 4: node visits per ray 6.97 -> 6.2.
constexpr uint64_t kTrainMinSamples = 1ull << 25;
constexpr size_t kTrainMinSpheres = 32;
#ifndef RTZIG_TRAIN_SAMPLES
#define RTZIG_TRAIN_SAMPLES 6000
#endif
constexpr size_t kTrainSamples = RTZIG_TRAIN_SAMPLES;  // build knob
constexpr uint64_t kTrainSeed = 0x7261792d74726565ull;

int32_t device_ref(int32_t ref) {
    if (ref >= 0) return (int32_t)((int64_t)ref * (int64_t)sizeof(rtk::BvhNode));
    return ~(int32_t)((int64_t)(~ref) * (int64_t)sizeof(rtk::BvhLeaf));
}

rtk::GeoRec geo_of(const rt_sphere* s) {
    rtk::GeoRec g;
    if (!s) {  // never-hit sentinel (rt_kernel.h)
        g.cx = g.cy = g.cz = 0.0;
        g.r2 = -std::numeric_limits<double>::infinity();
        return g;
    }
    const double r = s->radius > 0 ? s->radius : 0.0;  // Sphere.init clamps (sphere.zig:21)
    g.cx = s->center[0];
    g.cy = s->center[1];
    g.cz = s->center[2];
    g.r2 = r * r;
    return g;
}

void set_tree(SceneData& sd, const rtbvh::Bvh& bvh, double bound) {
    sd.trained = false;
    sd.train_tried = false;
    // byte-offset refs must fit int32 (and stay clear of the walk's INT32_MIN "done" marker)
    const bool fits = bvh.nodes.size() * sizeof(rtk::BvhNode) < (1ull << 30) &&
                      bvh.slot_to_sphere.size() / rtk::kLeafBvh * sizeof(rtk::BvhLeaf) < (1ull << 30);
    sd.bvh_ok = bvh.ok && fits;
    sd.origin_bound = bound;
    if (!sd.bvh_ok) return;
    static_assert(rtbvh::kLeafMax == rtk::kLeafBvh && rtbvh::kMaxDepth == rtk::kMaxDepthBvh, "BVH constants differ");
    const size_t nn = bvh.nodes.size();
    const size_t na = bvh.n_always;
    const size_t nl = (bvh.slot_to_sphere.size() - na) / rtk::kLeafBvh;
    auto sphere = [&](uint32_t k) { return k == rtbvh::kSentinel ? nullptr : &sd.spheres[k]; };
    sd.nodes.assign(nn, rtk::BvhNode{});
    for (size_t i = 0; i < nn; i++) {
        const rtbvh::Node& src = bvh.nodes[i];
        rtk::BvhNode& d = sd.nodes[i];
        for (int a = 0; a < 3; a++) {  // {lo, hi, hi, lo}: see rtk::BvhNode
            d.c0[a][0] = d.c0[a][3] = src.lo0[a];
            d.c0[a][1] = d.c0[a][2] = src.hi0[a];
            d.c1[a][0] = d.c1[a][3] = src.lo1[a];
            d.c1[a][1] = d.c1[a][2] = src.hi1[a];
        }
        // device refs are BYTE offsets (node: ref * 104 >= 0, leaf: ~(leaf * sizeof(BvhLeaf))) so the
        // walk forms LDS/global addresses with an add instead of a quarter-rate v_mul_lo_u32
        d.ref0 = device_ref(src.ref0);
        d.ref1 = device_ref(src.ref1);
    }
    sd.leaves.assign(nl ? nl : 1, rtk::BvhLeaf{});
    for (size_t l = 0; l < nl; l++)
        for (int u = 0; u < rtk::kLeafBvh; u++) {
            const uint32_t k = bvh.slot_to_sphere[na + l * rtk::kLeafBvh + u];
            const rtk::GeoRec g = geo_of(sphere(k));
            sd.leaves[l].g[u] = rtk::LeafGeo{g.cx, g.cy, g.cz, g.r2};
            sd.leaves[l].sid[u] = k;
        }
    sd.ageo.assign(na ? na : 1, geo_of(nullptr));
    sd.asid.assign(na ? na : 1, 0);
    for (size_t q = 0; q < na; q++) {
        sd.ageo[q] = geo_of(sphere(bvh.slot_to_sphere[q]));
        sd.asid[q] = bvh.slot_to_sphere[q];
    }
    sd.n_nodes = (uint32_t)nn;
    sd.n_leaves = (uint32_t)nl;
    sd.n_always = (uint32_t)na;
    sd.depth = (uint32_t)std::max(2, std::min(bvh.depth, rtk::kMaxDepthBvh));
}

void build_bvh(SceneData& sd, double bound) {
    rtbvh::Bvh bvh;  // ok = false: the linear walk
    try {            // the builder uses host threads for the top of the tree
        bvh = rtbvh::build(sd.spheres.data(), sd.spheres.size(), bound);
    } catch (const std::exception&) {
        bvh = rtbvh::Bvh{};
    }
    set_tree(sd, bvh, bound);
}

bool same_view(const rt_camera& a, const rt_camera& b) {
    rt_camera x = a, y = b;
    x.samples_per_pixel = y.samples_per_pixel = 0;
    x.pixel_samples_scale = y.pixel_samples_scale = 0;
    x.seed = y.seed = 0;
    return std::memcmp(&x, &y, sizeof x) == 0;
}

// Should a launch of `samples` samples train the tree for its camera?  RTZIG_BVH_TRAIN=0|1 forces
// it off / on (test hook: trained trees on small launches).
bool want_train(const SceneData& sd, uint64_t samples) {
    if (const char* e = std::getenv("RTZIG_BVH_TRAIN")) {
        if (std::strcmp(e, "0") == 0) return false;
        if (std::strcmp(e, "1") == 0) return sd.bvh_ok;
    }
    return sd.bvh_ok && samples >= kTrainMinSamples && sd.spheres.size() >= kTrainMinSpheres;
}

// Rebuilds sd's tree from sample rays of `cam` (rtbvh::sample_rays over the SAH tree, then the
// ray-driven build).  The result depends only on (spheres, origin bound, view), so it is memoised
// process-wide: rt_render's devices and later calls reuse it.  Any valid tree returns the same
// bits (rt_bvh.hpp); this one only visits fewer nodes for this camera's rays.  A training that
// fails or is rejected (builder exception, no tree, LDS budget) keeps the current tree and is
// memoised too (train_tried), so later launches of the same view do not quiesce and retry it.
bool try_train(SceneData& sd, const rt_camera& cam) {
    const double bound = sd.origin_bound;
    rtbvh::Bvh sah, tree;
    try {  // the trained build runs on host threads; if they cannot be had, keep the current tree
        sah = rtbvh::build(sd.spheres.data(), sd.spheres.size(), bound);
        if (!sah.ok) return false;
        const std::vector<rtbvh::TrainRay> rays =
            rtbvh::sample_rays(sd.spheres.data(), sd.spheres.size(), cam, sah, kTrainSamples, kTrainSeed);
        tree = rtbvh::build(sd.spheres.data(), sd.spheres.size(), bound, &rays);
    } catch (const std::exception&) {
        return false;
    }
    if (!tree.ok) return false;
    // a trained tree that the launchers would not stage in LDS where they do stage the SAH tree (or
    // that does not build) is not used: the launchers' own rule (rtk::bvh_lds_plan)
    auto in_lds = [](const SceneData& t) {
        return rtk::bvh_lds_plan(t.n_nodes, t.n_leaves, t.depth, rtk::kBlockBvh, rtk::kLdsSceneBudget).lds_scene;
    };
    SceneData sah_sd = sd;
    set_tree(sah_sd, sah, bound);
    SceneData tr = sd;
    set_tree(tr, tree, bound);
    if (!tr.bvh_ok || (!in_lds(tr) && in_lds(sah_sd))) {
        if (sah_sd.bvh_ok) sd = sah_sd;
        return false;
    }
    sd = tr;
    return true;
}

double cam_origin_bound(const rt_camera& cam) {
    double b = 0;
    for (int a = 0; a < 3; a++)
        b = std::max(b, std::fabs(cam.center[a]) + std::fabs(cam.defocus_disk_u[a]) + std::fabs(cam.defocus_disk_v[a]));
    return b;
}
bool needs_far_rebuild(const SceneData& sd, const rt_camera& cam) {
    return sd.bvh_ok && !(cam_origin_bound(cam) <= sd.origin_bound);
}
double far_bound(const SceneData& sd, const rt_camera& cam) {
    return std::max(cam_origin_bound(cam), sd.origin_bound) * 1.01;
}
bool needs_training(const SceneData& sd, const rt_camera& cam, uint64_t samples) {
    return want_train(sd, samples) && !(sd.train_tried && same_view(sd.view, cam));
}

void train_bvh(SceneData& sd, const rt_camera& cam) {
    static std::mutex mu;
    static SceneData memo;
    static bool memo_valid = false;
    std::lock_guard<std::mutex> lock(mu);
    if (memo_valid && same_view(memo.view, cam) && memo.origin_bound == sd.origin_bound &&
        memo.spheres.size() == sd.spheres.size() &&
        std::memcmp(memo.spheres.data(), sd.spheres.data(), sd.spheres.size() * sizeof(rt_sphere)) == 0) {
        sd = memo;
        return;
    }
    const bool ok = try_train(sd, cam);
    sd.trained = ok;
    sd.train_tried = true;
    sd.view = cam;
    memo = sd;
    memo_valid = true;
}

void build_scene(const rt_sphere* spheres, size_t n, SceneData& sd) {
    sd = SceneData{};
    sd.spheres.assign(spheres, spheres + n);
    const size_t n_pad = (n + rtk::kPad - 1) / rtk::kPad * rtk::kPad;
    sd.geo.assign(n_pad, geo_of(nullptr));
    sd.mat.assign(n, rtk::MatRec{});
    for (size_t k = 0; k < n; k++) {
        sd.geo[k] = geo_of(&spheres[k]);
        rtk::MatRec& m = sd.mat[k];
        const double r = spheres[k].radius > 0 ? spheres[k].radius : 0.0;
        for (int c = 0; c < 3; c++) m.albedo[c] = spheres[k].albedo[c];
        m.fuzz = spheres[k].fuzz;
        m.ior = spheres[k].refraction_index;
        m.inv_r = 1.0 / r;
        const double ior = spheres[k].refraction_index;
        m.inv_ior = 1.0 / ior;
        for (int face = 0; face < 2; face++) {  // reflectance()'s r0 (material.zig:106-108) per face
            const double ri = face == 0 ? m.inv_ior : ior;
            double r0 = (1 - ri) / (1 + ri);
            r0 = r0 * r0;
            (face == 0 ? m.r0_front : m.r0_back) = r0;
        }
        m.kind = spheres[k].material;
    }
    const double extent = rtbvh::scene_extent(spheres, n);
    build_bvh(sd, extent * (1.0 + 0x1p-20) + 1e-300);
}

bool same_spheres(const SceneData& sd, const rt_sphere* s, size_t n) {
    return sd.spheres.size() == n && n && std::memcmp(sd.spheres.data(), s, n * sizeof(rt_sphere)) == 0;
}

}  // namespace rtscene

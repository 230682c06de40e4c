// Host check of the scene code (csrc/rt_scene.cpp over rt_bvh.cpp): the padded records, the device
// tree's refs and sphere slots, the far-camera rebuild rule and the memoised training.  Sphere lists
// of 1, 9 (one past the list walk's 8) and 40 (past the training's 32).  No GPU, no HIP runtime call.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../raytracing-with-zig_amd/csrc/rt_scene.hpp"

using namespace rtscene;

static int g_bad = 0;
#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            g_bad++;                  \
        }                             \
    } while (0)

static std::vector<rt_sphere> spheres_of(size_t n) {
    std::vector<rt_sphere> v(n);
    uint64_t x = 0x9e3779b97f4a7c15ull + n;
    auto u = [&]() {  // [0, 1)
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(x >> 11) * 0x1p-53;
    };
    for (size_t k = 0; k < n; k++) {
        rt_sphere& s = v[k];
        std::memset(&s, 0, sizeof s);
        for (int a = 0; a < 3; a++) s.center[a] = 6.0 * u() - 3.0;
        s.radius = 0.2 + 0.3 * u();
        s.material = (uint32_t)(k % 3);
        s.albedo[0] = s.albedo[1] = s.albedo[2] = 0.5;
        s.refraction_index = 1.5;
    }
    if (n > 1) {  // the book's ground: an always-list sphere
        v[0].center[0] = v[0].center[2] = 0;
        v[0].center[1] = -1000.5;
        v[0].radius = 1000;
    }
    return v;
}

static rt_camera camera_at(double cx, double cy, double cz) {
    rt_camera c;
    std::memset(&c, 0, sizeof c);
    c.image_width = 32;
    c.image_height = 16;
    c.samples_per_pixel = 4;
    c.bounce_max = 8;
    c.pixel_samples_scale = 0.25;
    const double center[3] = {cx, cy, cz}, p0[3] = {cx - 1.55, cy + 0.75, cz - 1.0};
    for (int a = 0; a < 3; a++) c.center[a] = center[a], c.pixel0[a] = p0[a];
    c.du[0] = 0.1;
    c.dv[1] = -0.1;
    c.t_min = 1e-3;
    c.t_max = INFINITY;
    c.seed = 7;
    return c;
}

static void check_tree(const SceneData& sd, size_t n) {
    CHECK(sd.nodes.size() == sd.n_nodes && sd.leaves.size() == (sd.n_leaves ? sd.n_leaves : 1), "n %zu: array sizes", n);
    CHECK(sd.depth >= 2 && sd.depth <= (uint32_t)rtk::kMaxDepthBvh, "n %zu: depth %u", n, sd.depth);
    // every device ref decodes back through device_ref to a node or leaf inside the arrays
    for (const rtk::BvhNode& nd : sd.nodes)
        for (int32_t ref : {nd.ref0, nd.ref1}) {
            if (ref >= 0) {
                const int32_t i = ref / (int32_t)sizeof(rtk::BvhNode);
                CHECK(device_ref(i) == ref && (uint32_t)i < sd.n_nodes, "n %zu: node ref %d", n, ref);
            } else {
                const int32_t l = ~ref / (int32_t)sizeof(rtk::BvhLeaf);
                CHECK(device_ref(~l) == ref && (uint32_t)l < sd.n_leaves, "n %zu: leaf ref %d", n, ref);
            }
        }
    // every sphere index appears in exactly one leaf slot or in the always list
    std::vector<int> seen(n, 0);
    for (uint32_t l = 0; l < sd.n_leaves; l++)
        for (int u = 0; u < rtk::kLeafBvh; u++) {
            const uint32_t k = sd.leaves[l].sid[u];
            if (k == rtbvh::kSentinel) continue;
            CHECK(k < n, "n %zu: leaf %u holds sphere %u", n, l, k);
            if (k < n) seen[k]++;
        }
    for (uint32_t q = 0; q < sd.n_always; q++) {
        CHECK(sd.asid[q] < n, "n %zu: always slot %u holds sphere %u", n, q, sd.asid[q]);
        if (sd.asid[q] < n) seen[sd.asid[q]]++;
    }
    for (size_t k = 0; k < n; k++) CHECK(seen[k] == 1, "n %zu: sphere %zu appears %d times", n, k, seen[k]);
}

static bool same_tree(const SceneData& a, const SceneData& b) {
    auto eq = [](const auto& x, const auto& y) {
        return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0;
    };
    return a.bvh_ok == b.bvh_ok && a.trained == b.trained && a.train_tried == b.train_tried && a.n_nodes == b.n_nodes &&
           a.n_leaves == b.n_leaves && a.n_always == b.n_always && a.depth == b.depth &&
           a.origin_bound == b.origin_bound && eq(a.nodes, b.nodes) && eq(a.leaves, b.leaves) && eq(a.ageo, b.ageo) &&
           eq(a.asid, b.asid);
}

int main() {
    setenv("RTZIG_BVH_TRAIN", "1", 1);  // trained trees on small launches (want_train's hook)
    for (size_t n : {(size_t)1, (size_t)9, (size_t)40}) {
        const std::vector<rt_sphere> sp = spheres_of(n);
        SceneData sd;
        build_scene(sp.data(), n, sd);
        // geo is padded to kPad with never-hit sentinels {0, 0, 0, -inf}
        const size_t n_pad = (n + rtk::kPad - 1) / rtk::kPad * rtk::kPad;
        CHECK(sd.geo.size() == n_pad && sd.mat.size() == n && same_spheres(sd, sp.data(), n), "n %zu: record counts", n);
        for (size_t k = 0; k < sd.geo.size(); k++) {
            const rtk::GeoRec& g = sd.geo[k];
            if (k < n)
                CHECK(g.cx == sp[k].center[0] && g.r2 == sp[k].radius * sp[k].radius, "n %zu: record %zu", n, k);
            else
                CHECK(g.cx == 0 && g.cy == 0 && g.cz == 0 && g.r2 == -INFINITY, "n %zu: sentinel %zu", n, k);
        }
        CHECK(sd.bvh_ok || n == 1, "n %zu: no tree", n);
        if (!sd.bvh_ok) continue;
        check_tree(sd, n);

        // the far-camera rule: false at the bound, true just past it
        rt_camera at = camera_at(sd.origin_bound, 0, 0);
        CHECK(cam_origin_bound(at) == sd.origin_bound && !needs_far_rebuild(sd, at), "n %zu: rebuild at the bound", n);
        at.center[0] = std::nextafter(sd.origin_bound, INFINITY);
        CHECK(needs_far_rebuild(sd, at), "n %zu: no rebuild just past the bound", n);
        const rt_camera far = camera_at(1e6, -2e6, 3.0);
        CHECK(needs_far_rebuild(sd, far) && far_bound(sd, far) > cam_origin_bound(far), "n %zu: far_bound", n);
        SceneData fr = sd;
        build_bvh(fr, far_bound(sd, far));
        CHECK(fr.bvh_ok && !needs_far_rebuild(fr, far), "n %zu: still far after the rebuild", n);
        if (fr.bvh_ok) check_tree(fr, n);

        // training: tried once per (scene, view), memoised process-wide
        const rt_camera cam = camera_at(0, 0.5, 6.0);
        CHECK(needs_training(sd, cam, 1), "n %zu: training not wanted", n);
        SceneData a = sd, b = sd;
        train_bvh(a, cam);
        CHECK(a.train_tried && a.bvh_ok, "n %zu: train_tried not set", n);
        check_tree(a, n);
        train_bvh(b, cam);
        CHECK(same_tree(a, b), "n %zu: the second training differs", n);
        rt_camera again = cam;  // the same rays: sample count and seed play no part
        again.samples_per_pixel = 100;
        again.pixel_samples_scale = 0.01;
        again.seed = 99;
        CHECK(!needs_training(a, again, 1), "n %zu: the same view trains again", n);
        CHECK(needs_training(a, camera_at(0.25, 0.5, 6.0), 1), "n %zu: a moved camera does not train", n);
    }
    if (g_bad) return 1;
    std::printf("OK\n");
    return 0;
}

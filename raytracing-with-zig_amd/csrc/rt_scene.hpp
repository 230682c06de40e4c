// rt_scene.hpp — the host side of a scene: the device records of a Hittable list, its BVH in the
// device layout (rt_kernel.h), and the rules for rebuilding and training that tree.  Host arithmetic
// only: no HIP runtime call (rt_scene.cpp), so it links into CPU tests as it is.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/rt.h"
#include "rt_bvh.hpp"
#include "rt_kernel.h"

namespace rtscene {

// Host-side scene: device records of the Hittable list plus its BVH, built once per sphere list and
// uploaded to every device that renders it.
struct SceneData {
    std::vector<rt_sphere> spheres;
    std::vector<rtk::GeoRec> geo;  // padded to kPad with never-hit sentinels
    std::vector<rtk::MatRec> mat;
    bool bvh_ok = false;
    double origin_bound = 0;
    std::vector<rtk::BvhNode> nodes;
    std::vector<rtk::BvhLeaf> leaves;
    std::vector<rtk::GeoRec> ageo;
    std::vector<uint32_t> asid;
    uint32_t n_nodes = 0, n_leaves = 0, n_always = 0, depth = 0;
    bool trained = false;      // the tree was built from sample rays of camera `view` (train_bvh)
    bool train_tried = false;  // train_bvh ran for `view` (trained or not: a failure is not retried)
    rt_camera view{};
};

// Builder ref (node index >= 0, ~leaf index < 0) -> device ref (byte offsets, see set_tree).
int32_t device_ref(int32_t ref);
rtk::GeoRec geo_of(const rt_sphere* s);  // nullptr: the never-hit sentinel
// Sets sd's device tree from `bvh` (built for ray origins with |o_i| <= bound; rt_kernel.h layout).
void set_tree(SceneData& sd, const rtbvh::Bvh& bvh, double bound);
// The SAH BVH of sd.spheres, valid for ray origins with |o_i| <= bound.
void build_bvh(SceneData& sd, double bound);
// Device records + BVH of a sphere list (validated by the caller).
void build_scene(const rt_sphere* spheres, size_t n, SceneData& sd);
// Do two cameras shoot the same rays (every field getRay / rayColor read except spp and seed)?
bool same_view(const rt_camera& a, const rt_camera& b);
bool same_spheres(const SceneData& sd, const rt_sphere* s, size_t n);

// The tree preparation a launch of `samples` samples with camera `cam` does before it runs: a
// rebuild with a larger origin bound (far_bound) when the camera's ray origins lie beyond it, then
// the ray-driven training (train_bvh).  rt_render runs it on a host thread beside HIP's start-up.
double cam_origin_bound(const rt_camera& cam);
bool needs_far_rebuild(const SceneData& sd, const rt_camera& cam);
double far_bound(const SceneData& sd, const rt_camera& cam);
bool want_train(const SceneData& sd, uint64_t samples);
bool needs_training(const SceneData& sd, const rt_camera& cam, uint64_t samples);
bool try_train(SceneData& sd, const rt_camera& cam);
void train_bvh(SceneData& sd, const rt_camera& cam);

}  // namespace rtscene

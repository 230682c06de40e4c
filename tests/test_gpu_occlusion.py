"""Occlusion queries on the GPU (include/rt.h rt_occluded_rays): one boolean per
caller-supplied ray, equal to HittableList.hit's return value.

The reference is computed on the CPU from oracle.world_hit(...)[0] >= 0 per ray (occlusion_support).
Every comparison is np.array_equal; the mask is compared against np.packbits(..., bitorder="little")
viewed as u64.  The counts and shares asserted on the reference are input conditions — they say that a
case exercises what it is meant to — not tolerances."""
import numpy as np
import pytest
import torch

import fast_scenes
import rtzig
from gpu_support import DEV, cached
from gpu_support import module_renderers, renderers  # noqa: F401 (fixtures)
from occlusion_support import (INF, MASK_SENTINEL, N, NAN, U8_SENTINEL, assert_answers, base_rays, base_ref,
                               edge_intervals, final_cam, ground_rays, intervals_of, mask_of, non_finite_rays, query,
                               ref_occluded, sphere_hits, targets, trace_hit)
from rtzig.lib import RtError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def final_renderer(module_renderers):
    return module_renderers(final_cam().scene.world)


def world():
    return final_cam().scene.world


# ---- 1. base -----------------------------------------------------------------------------------------
def test_base_rays_u8_mask_stats_bvh_in_lds(oracle, renderers):
    O, D = base_rays()
    occ, _ = base_ref(oracle)
    assert int(occ.sum()) == 2042  # input condition
    r = renderers(world())
    assert r.tree_info()["bvh"] == 1
    got = query(r, O, D)
    assert r.kernel_name() == "bvh_lds(occlusion)"
    assert got["stats"] == [N, 0, 2042]
    assert_answers(got, occ, label="base")
    for n in (1, 63, 64, 65, 127):
        got = query(r, O[:128], D[:128], n=n)
        assert got["stats"] == [n, 0, int(occ[:n].sum())]
        assert_answers(got, occ, n=n, label="prefix %d" % n)  # nothing past n, the last word's high bits 0
        assert int(got["mask"][(n - 1) // 64]) >> ((n - 1) % 64 + 1) == 0
    r.close()


# ---- 2. outputs one at a time ------------------------------------------------------------------------
def test_outputs_one_at_a_time(oracle, final_renderer):
    O, D = base_rays()
    O, D = O[:1000], D[:1000]
    occ, _ = base_ref(oracle)
    occ = occ[:1000]
    r = final_renderer
    got = query(r, O, D, outputs=("u8", "stats"))
    assert np.array_equal(got["u8"], occ.astype(np.uint8)) and (got["mask"] == np.uint64(MASK_SENTINEL)).all()
    assert got["stats"] == [1000, 0, int(occ.sum())]
    got = query(r, O, D, outputs=("mask",))
    assert np.array_equal(got["mask"], mask_of(occ)) and (got["u8"] == U8_SENTINEL).all()
    assert got["stats"] == [0, 0, 0]
    got = query(r, O, D, outputs=("stats",))  # d_stats alone still launches
    assert got["stats"] == [1000, 0, int(occ.sum())]
    assert (got["u8"] == U8_SENTINEL).all() and (got["mask"] == np.uint64(MASK_SENTINEL)).all()
    assert r.kernel_name() == "bvh_lds(occlusion)"
    img = torch.empty((final_cam().height, final_cam().width, 3), dtype=torch.float64, device=DEV)
    r.render_rows_async(final_cam().cam, img.data_ptr())
    torch.cuda.synchronize()
    name = r.kernel_name()
    assert "occlusion" not in name
    got = query(r, O, D, outputs=())  # nothing asked for: no launch
    assert got["stats"] == [0, 0, 0] and (got["u8"] == U8_SENTINEL).all() and (got["mask"] == np.uint64(MASK_SENTINEL)).all()
    assert r.kernel_name() == name


# ---- 3. intervals ------------------------------------------------------------------------------------
def test_interval_edge_cases_interleaved_lane_by_lane(oracle, final_renderer):
    O, D = base_rays()
    O, D = O[:1024], D[:1024]
    iv = edge_intervals(1024)
    occ, _ = cached("occ_iv_mixed", lambda: ref_occluded(oracle, world(), O, D, iv))
    assert 0.2 < occ.mean() < 0.8
    got = query(final_renderer, O, D, t_min=NAN, t_max=NAN, iv=iv)  # the scalars are not used
    assert got["stats"][0] == 1024 and 0 < got["stats"][1] < 1024  # both routes in every wave
    assert got["stats"][2] == int(occ.sum())
    assert_answers(got, occ, label="mixed")
    assert np.array_equal(trace_hit(final_renderer, O, D, iv=iv), occ)  # 10. cross-check on the device


def test_per_ray_t_max_and_peeling_past_the_closest_root(oracle, final_renderer):
    O, D = base_rays()
    base, first = base_ref(oracle)
    iv = intervals_of(N, 1e-3, np.random.default_rng(2).uniform(.5, 20, N))
    occ, _ = cached("occ_iv_tmax", lambda: ref_occluded(oracle, world(), O, D, iv))
    assert 0 < occ.sum() < base.sum() and not (occ & ~base).any()  # a shorter interval only loses hits
    got = query(final_renderer, O, D, iv=iv)
    assert got["stats"] == [N, 0, int(occ.sum())]
    assert_answers(got, occ, label="per-ray t_max")
    # peel: t_min = the closest root, which the strict comparison excludes; a later root may remain
    iv = intervals_of(N, first, INF)
    occ, _ = cached("occ_iv_peel", lambda: ref_occluded(oracle, world(), O, D, iv))
    assert not occ[~base].any() and 0.9 < occ[base].mean() < 1.0
    got = query(final_renderer, O, D, iv=iv)
    assert got["stats"][0] == N and got["stats"][1] == int((~base).sum())  # t_min = +inf leaves the tree's domain
    assert_answers(got, occ, label="peel")
    # the closest root as t_max: nothing is closer, and the comparison is strict
    got = query(final_renderer, O, D, iv=intervals_of(N, 1e-3, first))
    assert_answers(got, np.zeros(N, bool), label="strict t_max")


# ---- 4. non-finite and zero components ---------------------------------------------------------------
def test_non_finite_and_zero_components_are_unoccluded_and_scanned(oracle, final_renderer):
    O, D = non_finite_rays()
    occ, _ = cached("occ_non_finite", lambda: ref_occluded(oracle, world(), O, D, intervals_of(640, 1e-3, INF)))
    assert not occ.any()
    got = query(final_renderer, O, D)
    assert got["stats"] == [640, 640, 0]
    assert_answers(got, occ, label="non-finite")
    # interleaved with ordinary rays, which stay on the tree and keep their answers
    O2, D2 = base_rays()
    O2, D2 = O2[:640].copy(), D2[:640].copy()
    O2[::2], D2[::2] = O[::2], D[::2]
    want = base_ref(oracle)[0][:640].copy()
    want[::2] = False
    got = query(final_renderer, O2, D2)
    assert got["stats"] == [640, 320, int(want.sum())]
    assert_answers(got, want, label="interleaved")


# ---- 5. the direction scale ladder -------------------------------------------------------------------
@pytest.mark.parametrize("e", [-140, 60, 140])
def test_direction_scale_ladder(oracle, final_renderer, e):
    O, D = base_rays()
    O, D = O[:1024], D[:1024]
    Ds = D * 2.0 ** e  # a power of two: exact
    t_min = 1e-3 * 2.0 ** -e
    occ, _ = cached("occ_scale_%d" % e, lambda: ref_occluded(oracle, world(), O, Ds, intervals_of(1024, t_min, INF)))
    assert np.array_equal(occ, base_ref(oracle)[0][:1024])
    got = query(final_renderer, O, Ds, t_min=t_min)
    assert_answers(got, occ, label="2^%d" % e)
    assert got["stats"][0] == 1024 and got["stats"][2] == int(occ.sum())
    if abs(e) == 140:
        assert got["stats"][1] == 1024  # outside any f32 range the slab walk could be trusted in


# ---- 6. far origins ----------------------------------------------------------------------------------
def test_far_origins_scan_then_tree_after_reserve(oracle, renderers):
    O, D = base_rays()
    Of = O * 400
    Df = -Of + D
    occ, _ = cached("occ_far", lambda: ref_occluded(oracle, world(), Of, Df, intervals_of(N, 1e-3, INF)))
    assert 0.9 < occ.mean() < 1.0
    r = renderers(world())
    bound = r.origin_bound()
    beyond = np.abs(Of).max(axis=1) > bound
    assert 0 < beyond.sum() < N
    got = query(r, Of, Df)
    assert got["stats"] == [N, int(beyond.sum()), int(occ.sum())]
    assert_answers(got, occ, label="far, scanned")
    assert np.array_equal(trace_hit(r, Of, Df), occ)  # 10. cross-check on the device
    r.reserve_origin_bound(6000)
    got = query(r, Of, Df)
    assert got["stats"] == [N, 0, int(occ.sum())]
    assert_answers(got, occ, label="far, tree")
    r.close()


# ---- 7. which structure answers ----------------------------------------------------------------------
def test_rays_pointing_down_are_occluded_by_the_ground(oracle, final_renderer):
    """The ground is a sphere of radius 1000: 19 of the 4096 downward rays are so shallow that they pass
    over its horizon, and nothing else stops them.  Every occluded ray is occluded by the ground, the
    always-list's sphere; the sub-batch of those rays is occluded ray for ray."""
    O, D = base_rays()
    D = D.copy()
    D[:, 1] = -np.abs(D[:, 1]) - 0.1
    by_ground = cached("occ_down_ground", lambda: sphere_hits(oracle, world()[0], O, D, 1e-3, INF))
    occ, _ = cached("occ_down", lambda: ref_occluded(oracle, world(), O, D, intervals_of(N, 1e-3, INF)))
    assert int(by_ground.sum()) == 4077 and np.array_equal(occ, by_ground)  # input conditions
    got = query(final_renderer, O, D)
    assert got["stats"] == [N, 0, 4077]
    assert_answers(got, occ, label="down")
    got = query(final_renderer, O[by_ground], D[by_ground])
    assert got["stats"] == [4077, 0, 4077]
    assert_answers(got, np.ones(4077, bool), label="down, all occluded")


def test_rays_leaving_the_ground_are_occluded_by_the_tree_only(oracle, final_renderer):
    O, D = ground_rays()
    occ, _ = cached("occ_ground", lambda: ref_occluded(oracle, world(), O, D, intervals_of(N, 1e-3, INF)))
    assert int(occ.sum()) == 663  # input conditions: and none of them by the ground
    assert not cached("occ_ground_ground", lambda: sphere_hits(oracle, world()[0], O, D, 1e-3, INF)).any()
    got = query(final_renderer, O, D)
    assert got["stats"] == [N, 0, 663]
    assert_answers(got, occ, label="tree only")


# ---- 8. targets mode ---------------------------------------------------------------------------------
def test_targets_mode_equals_directions_mode_fed_the_difference(oracle, final_renderer):
    O, _ = base_rays()
    B = targets()
    Dn = B - O  # one f64 subtraction per component, as the device does
    occ, _ = cached("occ_targets_ref", lambda: ref_occluded(oracle, world(), O, Dn, intervals_of(N, 1e-3, 1.0)))
    assert int(occ.sum()) == 981  # input condition
    r = final_renderer
    got = query(r, O, B, t_max=1.0, targets=True)
    assert got["stats"] == [N, 0, 981]
    assert_answers(got, occ, label="targets")
    got_d = query(r, O, Dn, t_max=1.0)
    assert np.array_equal(got_d["u8"], got["u8"]) and np.array_equal(got_d["mask"], got["mask"])
    assert np.array_equal(trace_hit(r, O, Dn, t_max=1.0), occ)  # 10. cross-check on the device
    assert_answers(query(r, O[:1000], B[:1000], t_max=1.0, targets=True, stride=4), occ, n=1000, label="targets, stride 4")
    assert_answers(query(r, O[:1000], B[:1000], t_max=1.0, targets=True, stride=0), occ, n=1000, label="targets, stride 0")
    assert_answers(query(r, O[:1000], Dn[:1000], t_max=1.0, stride=4), occ, n=1000, label="directions, stride 4")
    # the same end points read as directions are another question
    assert not np.array_equal(query(r, O, B, t_max=1.0)["u8"], got["u8"])


def test_an_occluder_exactly_at_the_end_point_does_not_count(renderers):
    """A unit sphere at the origin (and, to have a tree, eight more far off): the segment from (0, 0, 4)
    to (0, 0, 1) ends on the sphere with root exactly 1.0; to (0, 0, 0.5) it ends inside."""
    scene = rtzig.Scene(1).add((0, 0, 0), 1.0, rtzig.RT_LAMBERTIAN)
    for k in range(8):
        scene.add((40.0 + 3 * k, 0, 0), 1.0, rtzig.RT_LAMBERTIAN)
    A = np.array([[0, 0, 4.0], [0, 0, 4.0], [0, 0, 4.0]])
    B = np.array([[0, 0, 1.0], [0, 0, 0.5], [0, 0, 1.5]])
    for r in (renderers(scene.world), renderers(scene.world, "f32")):
        got = query(r, A, B, t_max=1.0, targets=True)
        assert got["u8"].tolist() == [0, 1, 0]
        assert query(r, A, B, t_max=1.0 + 2.0 ** -52, targets=True)["u8"].tolist() == [1, 1, 0]
        r.close()


# ---- 9. other structures -----------------------------------------------------------------------------
def test_chapter13_list_walk_scans_every_ray(oracle, renderers):
    cam = cached("occ_ch13", lambda: rtzig.chapter13_camera(width=37))
    g = np.random.default_rng(5)
    O = g.uniform([-3, -0.4, -3], [3, 2, 1], (1000, 3))
    D = g.standard_normal((1000, 3))
    occ, _ = cached("occ_ch13_ref", lambda: ref_occluded(oracle, cam.scene.world, O, D, intervals_of(1000, 1e-3, INF)))
    assert 0.3 < occ.mean() < 0.9
    r = renderers(cam.scene.world)
    assert r.tree_info()["bvh"] == 0
    got = query(r, O, D)
    assert r.kernel_name() in ("lds_u4(occlusion)", "smem_u4(occlusion)")
    assert got["stats"] == [1000, 1000, int(occ.sum())]
    assert_answers(got, occ, label="chapter 13")
    r.close()


def test_large_scene_global_memory_tree(oracle, renderers):
    cam = cached("occ_large", fast_scenes.large)
    O, D = base_rays()
    O, D = O[:1024] * 2.5, D[:1024]
    occ, _ = cached("occ_large_ref", lambda: ref_occluded(oracle, cam.scene.world, O, D, intervals_of(1024, 1e-3, INF)))
    assert 0.4 < occ.mean() < 0.9
    r = renderers(cam.scene.world)
    assert r.tree_info()["bvh"] == 1
    got = query(r, O, D)
    assert r.kernel_name() == "bvh_global(occlusion)"
    assert got["stats"] == [1024, 0, int(occ.sum())]
    assert_answers(got, occ, label="large")
    r.close()


@pytest.mark.parametrize("precision, bvh", [("f64", 0), ("f32", 1)])
def test_exact_duplicate_and_zero_radius_sphere(oracle, precision, bvh, renderers):
    """fast_scenes.materials(): sphere 5 is an exact copy of sphere 4, sphere 6 has radius 0.  Seven
    spheres walk the list on a parity context and the tree on an RT_PRECISION_F32 one (the query itself is
    always parity arithmetic)."""
    cam = cached("occ_materials", fast_scenes.materials)
    g = np.random.default_rng(9)
    O = g.uniform([-3, 0.6, -3], [3, 3, 2], (1024, 3))
    D = np.array([1.0, 0.0, -1.0]) - O
    D[512:] += g.standard_normal((512, 3)) * 0.3  # around the target too: every sphere, and misses
    O[1000:] = [0.0, 2.0, -1.0]                   # straight down through the zero-radius sphere
    D[1000:] = [0.0, -1.0, 0.0]
    occ, _ = cached("occ_materials_ref", lambda: ref_occluded(oracle, cam.scene.world, O, D, intervals_of(1024, 1e-3, INF)))
    assert 0 < occ.sum() and occ[:512].mean() > 0.9
    r = renderers(cam.scene.world, precision)
    assert r.tree_info()["bvh"] == bvh
    got = query(r, O, D)
    assert got["stats"] == [1024, 1024 * (1 - bvh), int(occ.sum())]
    assert_answers(got, occ, label="materials " + precision)
    r.close()


def test_trained_tree_gives_the_same_answers(oracle, monkeypatch, renderers):
    O, D = base_rays()
    occ, _ = base_ref(oracle)
    cam = final_cam()
    monkeypatch.setenv("RTZIG_BVH_TRAIN", "1")
    r = renderers(cam.scene.world)
    img = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device=DEV)
    r.render_rows_async(cam.cam, img.data_ptr())
    torch.cuda.synchronize()
    assert r.tree_info()["trained"] == 1
    got = query(r, O, D)
    assert r.tree_info()["trained"] == 1  # walked as it is
    assert got["stats"] == [N, 0, 2042]
    assert_answers(got, occ, label="trained tree")
    r.close()


@pytest.mark.parametrize("kind", ["instrumented", "f32"])
def test_instrumented_and_f32_contexts_give_the_same_answers(oracle, kind, renderers):
    O, D = base_rays()
    occ, _ = base_ref(oracle)
    r = renderers(world(), "f32" if kind == "f32" else "f64")
    if kind == "instrumented":
        r.enable_profile(True)
    got = query(r, O, D)
    assert got["stats"] == [N, 0, 2042] and r.kernel_name() == "bvh_lds(occlusion)"
    assert_answers(got, occ, label=kind)
    r.close()


# ---- 10. cross-check on the device (cases 3, 6 and 8 carry theirs) -----------------------------------
def test_base_rays_equal_the_closest_hit_call(oracle, final_renderer):
    O, D = base_rays()
    got = query(final_renderer, O, D)
    assert np.array_equal(got["u8"].astype(bool), trace_hit(final_renderer, O, D))


# ---- 11. plumbing ------------------------------------------------------------------------------------
def test_non_default_stream_needs_no_host_sync(oracle, final_renderer):
    O, D = base_rays()
    occ, _ = base_ref(oracle)
    h_o, h_d = torch.from_numpy(O.copy()).pin_memory(), torch.from_numpy(D.copy()).pin_memory()  # the shared rays are read-only
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        u8 = torch.full((N,), U8_SENTINEL, dtype=torch.uint8, device=DEV)  # the fills run on the stream too
        mask = torch.full((N // 64,), -1, dtype=torch.int64, device=DEV)
        # the inputs are produced on the stream: copies, then arithmetic that leaves the bits alone
        d_o = h_o.to(DEV, non_blocking=True) * 1.0
        d_d = h_d.to(DEV, non_blocking=True) + 0.0
        final_renderer.occluded_rays(d_o.data_ptr(), d_d.data_ptr(), N, d_occluded_ptr=u8.data_ptr(),
                                     d_mask_ptr=mask.data_ptr(), stream_ptr=s.cuda_stream)
        total = u8.sum(dtype=torch.int64)  # consumed on the stream
        got_u8, got_mask = u8.to("cpu", non_blocking=True), mask.to("cpu", non_blocking=True)
    s.synchronize()
    assert np.array_equal(got_u8.numpy(), occ.astype(np.uint8))
    assert np.array_equal(got_mask.numpy().view(np.uint64), mask_of(occ))
    assert int(total.cpu()) == 2042


def test_kernel_times_empty_calls_and_no_scene(oracle, renderers):
    O, D = base_rays()
    r = renderers(world())
    r.enable_timing(True)
    query(r, O[:256], D[:256])
    sample_ms, reduce_ms = r.kernel_times()
    assert sample_ms > 0 and reduce_ms == 0
    name = r.kernel_name()
    assert name == "bvh_lds(occlusion)"
    # n_rays == 0 and "nothing asked for" return RT_OK and launch nothing
    u8 = torch.full((4,), U8_SENTINEL, dtype=torch.uint8, device=DEV)
    mask = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    stats = torch.zeros(3, dtype=torch.int64, device=DEV)
    r.occluded_rays(1, 1, 0, d_occluded_ptr=u8.data_ptr(), d_mask_ptr=mask.data_ptr(), d_stats_ptr=stats.data_ptr())
    r.occluded_rays(1, 1, 4)  # the pointers are never read
    torch.cuda.synchronize()
    assert (u8.cpu().numpy() == U8_SENTINEL).all() and int(mask.cpu()[0]) == -1 and stats.cpu().tolist() == [0, 0, 0]
    assert r.kernel_name() == name
    r.close()
    r = renderers()
    with pytest.raises(RtError, match="no scene"):
        r.occluded_rays(1, 1, 4, d_occluded_ptr=1)
    r.close()


# ---- 12. Python --------------------------------------------------------------------------------------
def test_python_wrappers_equal_the_reference(oracle):
    O, D = base_rays()
    O, D = O[:777], D[:777]
    occ, _ = base_ref(oracle)
    scene = final_cam().scene
    for got in (rtzig.occluded(scene.world, O, D), scene.occluded(O, D)):
        assert got.dtype == bool and got.shape == (777,)
        assert np.array_equal(got, occ[:777])
    iv = edge_intervals(777)
    mixed, _ = cached("occ_iv_mixed", lambda: ref_occluded(oracle, scene.world, *[a[:1024] for a in base_rays()],
                                                          edge_intervals(1024)))
    assert np.array_equal(scene.occluded(O, D, intervals=iv), mixed[:777])
    B = targets()[:777]
    seg, _ = cached("occ_targets_ref", lambda: ref_occluded(oracle, scene.world, base_rays()[0], targets() - base_rays()[0],
                                                           intervals_of(N, 1e-3, 1.0)))
    assert np.array_equal(scene.occluded(O, B, t_max=1.0, targets=True), seg[:777])
    vis = scene.visible(O, B)
    assert vis.dtype == bool and np.array_equal(vis, ~seg[:777])
    assert rtzig.occluded(scene.world, np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    assert scene.occluded(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    assert scene.visible(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)

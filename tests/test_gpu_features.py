"""Feature buffers on the GPU (include/rt.h rt_render_rows_features): per pixel, the
unscaled sums over samples [0, n) of the camera ray's first-hit albedo, shading normal and Euclidean
depth, and the number of samples that hit.

The reference (tests/gpu_support.py) is computed on the CPU from the oracle's helpers alone: per (pixel, sample) the
draws of the stream oracle.sample_key(seed, pixel, sample), getRay restated in Python floats (IEEE
f64, no fused multiply-add, the operation order of oracle/rt_oracle.c get_ray / random_in_unit_disk),
oracle.world_hit for the winning sphere and its root, oracle.sphere_hit for the normal, the albedo
from the sphere, the depth as rt.h states it, all added in sample order from 0.0.  Every comparison is
np.array_equal on the raw sums."""
import numpy as np
import pytest
import torch

import fast_scenes
import rtzig
from gpu_support import DEV, Buffers, assert_equal, cached, reference
from gpu_support import renderers  # noqa: F401 (fixture)
from rtzig.abi import D3, RT_LAMBERTIAN, RtCamera, RtSphere

pytestmark = pytest.mark.gpu


def materials48():
    scene = fast_scenes.materials().scene
    return (rtzig.Camera.builder(48, 16 / 9).setScene(scene).setDefocusAngle(2.0).setFocusDist(1.5)
            .setViewport((0, 0.3, 0.5), (0, 0, -1), 70).setSamplesPerPixel(1).build())


def straddle48():
    scene = fast_scenes.c1_straddle().scene
    return (rtzig.Camera.builder(48, 1.5).setScene(scene).setDefocusAngle(0.0).setFocusDist(10)
            .setViewport((0, 0, 0), (0, 0, -1), 3).setSamplesPerPixel(1).build())


SCENES = {
    # name: (camera factory, samples)
    "final37": (lambda: rtzig.final_scene_camera(width=37, aspect_ratio=16 / 9, spp=1), 8),
    "chapter13": (lambda: rtzig.chapter13_camera(width=37), 8),
    "materials48": (materials48, 4),
    "straddle48": (straddle48, 2),
    "large": (fast_scenes.large, 2),
}


def scene_ref(oracle, name):
    """(camera, reference prefix sums) of a scene, computed once and left unchanged."""
    def make():
        factory, n = SCENES[name]
        cam = factory()
        ref = reference(oracle, cam.cam, cam.scene.world, n)
        for arrs in ref:
            for a in arrs:
                a.setflags(write=False)
        return cam, ref
    return cached(("features", name), make)


def run_split(r, cam, buf, split, ref=None, **rows):
    done = 0
    for count in split:
        r.features(cam.cam, done, count, **buf.ptrs(), **rows)
        done += count
        if ref is not None:
            assert_equal(buf.host(), ref[done], (split, done))
    return done


# ---- the final scene: LDS tree, ground on the always-list, a partial last wave ------------------------
@pytest.mark.parametrize("split", [[8], [1, 7], [3, 5], [2, 2, 2, 2]], ids=lambda s: "-".join(map(str, s)))
def test_final_scene_every_prefix_of_every_split_equals_the_reference(oracle, split, renderers):
    cam, ref = scene_ref(oracle, "final37")
    assert (cam.height, cam.width) == (20, 37) and len(cam.scene.world) == 485
    r = renderers(cam)
    info = r.tree_info()
    assert info["bvh"] == 1 and info["always"] >= 1
    buf = Buffers(740)
    assert run_split(r, cam, buf, split, ref) == 8
    assert r.kernel_name() == "bvh_lds(features)"
    r.sync()
    r.close()
    assert ref[8][3].max() == 8 and ref[8][3].min() == 0  # the image has both covered and open pixels


def test_new_image_overwrites_poisoned_buffers(oracle, renderers):
    """sample_begin = 0 neither reads nor keeps what the buffers held (NaN / 0xFFFFFFFF here)."""
    cam, ref = scene_ref(oracle, "final37")
    r = renderers(cam)
    buf = Buffers(740, poison=True)
    run_split(r, cam, buf, [3, 5])
    got = buf.host()
    r.sync()
    r.close()
    assert_equal(got, ref[8])


# ---- the other closest-hit structures and edge cases ---------------------------------------------------
def test_chapter13_list_walk_nested_dielectric(oracle, renderers):
    cam, ref = scene_ref(oracle, "chapter13")
    assert len(cam.scene.world) == 5
    r = renderers(cam)
    assert r.tree_info()["bvh"] == 0
    buf = Buffers(cam.width * cam.height)
    run_split(r, cam, buf, [8], ref)
    assert r.kernel_name() == "lds_u4(features)"
    r.sync()
    r.close()


def test_materials_duplicate_sphere_zero_radius_defocus(oracle, renderers):
    """The exact duplicate (spheres 4 and 5) must give the lower index's albedo; the scene also holds a
    zero-radius sphere and a defocus disk."""
    cam, ref = scene_ref(oracle, "materials48")
    w = cam.scene.world
    assert (cam.width, cam.cam.defocus_angle) == (48, 2.0)
    assert list(w[4].center) == list(w[5].center) and w[4].radius == w[5].radius and w[6].radius == 0.0
    assert tuple(w[4].albedo) != tuple(w[5].albedo)
    r = renderers(cam)
    buf = Buffers(cam.width * cam.height)
    run_split(r, cam, buf, [1, 3], ref)
    r.sync()
    r.close()


def test_straddle_huge_far_spheres_on_the_always_list(oracle, monkeypatch, renderers):
    """Five spheres walk the list by default; RTZIG_KERNEL=bvh walks the tree, whose always-list holds
    the two huge far spheres.  Both equal the reference."""
    cam, ref = scene_ref(oracle, "straddle48")
    assert cam.cam.defocus_angle == 0.0
    r = renderers(cam)
    buf = Buffers(cam.width * cam.height)
    run_split(r, cam, buf, [2], ref)
    r.close()
    monkeypatch.setenv("RTZIG_KERNEL", "bvh")
    r = renderers(cam)
    info = r.tree_info()
    assert info["bvh"] == 1 and info["always"] >= 2
    buf = Buffers(cam.width * cam.height, poison=True)
    run_split(r, cam, buf, [1, 1], ref)
    assert r.kernel_name().startswith("bvh_")
    r.sync()
    r.close()
    assert ref[2][3].max() > 0


def test_large_scene_global_memory_tree(oracle, renderers):
    cam, ref = scene_ref(oracle, "large")
    assert len(cam.scene.world) == 2600 and (cam.width, cam.height) == (96, 54)
    r = renderers(cam)
    assert r.tree_info()["bvh"] == 1
    buf = Buffers(96 * 54)
    run_split(r, cam, buf, [1, 1], ref)
    assert r.kernel_name() == "bvh_global(features)"
    r.sync()
    r.close()


# ---- partition independence ------------------------------------------------------------------------------
@pytest.mark.parametrize("row0, row_step", [(1, 3), (0, 3), (19, 1)])
def test_row_interleave_equals_the_matching_rows(oracle, row0, row_step, renderers):
    cam, ref = scene_ref(oracle, "final37")
    rows = list(range(row0, 20, row_step))
    r = renderers(cam)
    buf = Buffers(len(rows) * 37)
    run_split(r, cam, buf, [5, 3], row0=row0, row_step=row_step)
    got = buf.host()
    r.sync()
    r.close()
    want = tuple(a.reshape((20, 37) + a.shape[1:])[rows].reshape((len(rows) * 37,) + a.shape[1:]) for a in ref[8])
    assert_equal(got, want)


@pytest.mark.parametrize("only", ["albedo", "normal", "depth", "hits"])
def test_each_buffer_alone_equals_its_part_of_the_full_call(oracle, only, renderers):
    cam, ref = scene_ref(oracle, "final37")
    r = renderers(cam)
    buf = Buffers(740, poison=True)
    keep = [t.clone() for t in (buf.albedo, buf.normal, buf.depth, buf.hits)]
    ptr = {k: v for k, v in buf.ptrs().items() if k == f"d_{only}_ptr"}
    r.features(cam.cam, 0, 3, **ptr)
    r.features(cam.cam, 3, 5, **ptr)
    got = buf.host()
    r.sync()
    r.close()
    for name, g, w, k in zip(("albedo", "normal", "depth", "hits"), got, ref[8], keep):
        if name == only:
            assert np.array_equal(g, w), name
        else:  # untouched: still the poison
            assert np.array_equal(g.view(np.uint8), k.cpu().numpy().view(np.uint8)), name


def test_all_null_buffers_and_empty_calls_touch_nothing(oracle, renderers):
    cam, _ = scene_ref(oracle, "final37")
    r = renderers(cam)
    buf = Buffers(740, poison=True)
    keep = [t.clone() for t in (buf.albedo, buf.normal, buf.depth, buf.hits)]
    name = r.kernel_name()
    r.features(cam.cam, 0, 4)                          # all four NULL: no launch
    r.features(cam.cam, 0, 0, **buf.ptrs())            # no samples
    r.features(cam.cam, 0, 4, n_rows=0, **buf.ptrs())  # no rows
    assert r.kernel_name() == name
    torch.cuda.synchronize()
    r.sync()
    r.close()
    for t, k in zip((buf.albedo, buf.normal, buf.depth, buf.hits), keep):
        assert np.array_equal(t.cpu().numpy().view(np.uint8), k.cpu().numpy().view(np.uint8))


def test_f32_context_gives_the_f64_contexts_bits(oracle, renderers):
    """The pass is always parity arithmetic on the parity stream; on chapter 13 an F32 context also
    holds another structure (fast mode walks the tree of tiny scenes), which changes nothing."""
    for name, n in (("final37", 8), ("chapter13", 8)):
        cam, ref = scene_ref(oracle, name)
        r = renderers(cam, precision="f32")
        assert r.tree_info()["bvh"] == 1
        buf = Buffers(cam.width * cam.height)
        run_split(r, cam, buf, [3, n - 3])
        got = buf.host()
        assert r.kernel_name().startswith("bvh_")
        r.sync()
        r.close()
        assert_equal(got, ref[n], name)


def test_forced_list_walk_on_the_final_scene(oracle, monkeypatch, renderers):
    monkeypatch.setenv("RTZIG_KERNEL", "smem_u4")
    cam, ref = scene_ref(oracle, "final37")
    r = renderers(cam)
    assert r.tree_info()["bvh"] == 0
    buf = Buffers(740)
    run_split(r, cam, buf, [8])
    got = buf.host()
    assert r.kernel_name() == "smem_u4(features)"
    r.sync()
    r.close()
    assert_equal(got, ref[8])


@pytest.mark.parametrize("spread", [0, 2, 4])
@pytest.mark.parametrize("name, kernel", [("final37", "bvh_lds"), ("chapter13", "lds_u4"), ("large", "bvh_global")])
def test_every_lanes_per_pixel_form_gives_the_same_bits(oracle, monkeypatch, name, kernel, spread, renderers):
    """1, 4 or 16 lanes per pixel (RTZIG_FEATURE_SPREAD forces the form a launch's size would pick):
    the additions are the same in the same order.  Passes of 3 and n - 3 samples: rounds with lanes
    past the pass's last sample, and more lanes than samples."""
    monkeypatch.setenv("RTZIG_FEATURE_SPREAD", str(spread))
    cam, ref = scene_ref(oracle, name)
    n = len(ref) - 1
    r = renderers(cam)
    buf = Buffers(cam.width * cam.height, poison=True)
    run_split(r, cam, buf, [n] if n < 4 else [3, n - 3], ref)
    assert r.kernel_name() == kernel + "(features)"
    r.sync()
    r.close()


def test_trained_tree_gives_the_same_bits(oracle, monkeypatch, renderers):
    """A feature pass never trains; it walks the tree a colour pass left trained (RTZIG_BVH_TRAIN=1
    trains on this small launch)."""
    monkeypatch.setenv("RTZIG_BVH_TRAIN", "1")
    cam, ref = scene_ref(oracle, "final37")
    r = renderers(cam)
    buf = Buffers(740)
    run_split(r, cam, buf, [4])
    assert r.tree_info()["trained"] == 0  # the feature pass did not train
    accum = torch.empty((740, 3), dtype=torch.float64, device=DEV)
    r.accumulate(cam.cam, accum.data_ptr(), 0, 1)
    assert r.tree_info()["trained"] == 1
    r.features(cam.cam, 4, 4, **buf.ptrs())
    got = buf.host()
    r.sync()
    r.close()
    assert_equal(got, ref[8])


# ---- against the existing colour path ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chapter13", "materials48"])
def test_hits_agree_with_the_bounce_max_1_colour_render(oracle, name, renderers):
    """At bounce_max = 1 a sample that hits is black and a sample that misses is the (positive) sky:
    a pixel of the colour render is all-zero exactly where all n samples hit, and equals the render of
    a scene no ray hits (oracle B, same camera) exactly where none did.  Chapter 13 at 8 samples (its
    ground fills the view: every sample hits); the materials scene at 4 has all three kinds of pixel."""
    cam, ref = scene_ref(oracle, name)
    n = len(ref) - 1
    r = renderers(cam)
    buf = Buffers(cam.width * cam.height)
    r.features(cam.cam, 0, n, d_hits_ptr=buf.hits.data_ptr())
    torch.cuda.synchronize()
    hits = buf.hits.cpu().numpy().view(np.uint32)
    r.sync()
    r.close()
    c1 = RtCamera.from_buffer_copy(cam.cam)
    c1.samples_per_pixel, c1.bounce_max, c1.pixel_samples_scale = n, 1, 1.0 / n
    colour = rtzig.render(c1, cam.scene.world, n_gpus=1).reshape(-1, 3)
    # one small sphere behind the camera, as far back as the image plane is ahead
    W, H = cam.width, cam.height
    back = [2 * c1.center[c] - (c1.pixel0[c] + c1.du[c] * (W / 2) + c1.dv[c] * (H / 2)) for c in range(3)]
    behind = (RtSphere * 1)(RtSphere(center=D3(*back), radius=0.01, material=RT_LAMBERTIAN, albedo=D3(1, 1, 1)))
    sky, _ = oracle.render_b(c1, behind, threads=16)
    c2 = RtCamera.from_buffer_copy(c1)
    c2.bounce_max = 2  # a hit would now scatter into the sky and show: equal images mean no ray hit
    assert np.array_equal(sky, oracle.render_b(c2, behind, threads=16)[0]) and (sky > 0).all()
    assert np.array_equal(hits, ref[n][3])
    assert np.array_equal(hits == n, (colour == 0).all(axis=1))
    assert np.array_equal(hits == 0, (colour == sky.reshape(-1, 3)).all(axis=1))
    if name == "materials48":
        assert (hits == n).any() and (hits == 0).any() and ((hits > 0) & (hits < n)).any()


def test_colour_pass_between_feature_passes_changes_neither(oracle, renderers):
    cam, ref = scene_ref(oracle, "final37")
    r = renderers(cam)
    alone = torch.empty((740, 3), dtype=torch.float64, device=DEV)
    r.accumulate(cam.cam, alone.data_ptr(), 0, 6)
    buf = Buffers(740)
    accum = torch.empty((740, 3), dtype=torch.float64, device=DEV)
    r.features(cam.cam, 0, 5, **buf.ptrs())
    r.accumulate(cam.cam, accum.data_ptr(), 0, 6)
    r.features(cam.cam, 5, 3, **buf.ptrs())
    got = buf.host()
    r.sync()
    r.close()
    assert_equal(got, ref[8])
    assert np.array_equal(accum.cpu().numpy(), alone.cpu().numpy())


# ---- the Python layer -------------------------------------------------------------------------------------
def test_render_features_agrees_with_the_raw_sums(oracle):
    cam, ref = scene_ref(oracle, "final37")
    alb, nrm, dep, hits = ref[8]
    out = cam.render_features(8)
    assert set(out) == {"albedo", "normal", "depth", "coverage", "hits"}
    scale = 1.0 / 8
    assert np.array_equal(out["albedo"], (alb * scale).reshape(20, 37, 3))
    assert np.array_equal(out["normal"], (nrm * scale).reshape(20, 37, 3))
    assert out["hits"].dtype == np.uint32 and np.array_equal(out["hits"], hits.reshape(20, 37))
    assert np.array_equal(out["coverage"], hits.reshape(20, 37) / 8.0)
    miss = hits.reshape(20, 37) == 0
    assert miss.any() and np.isinf(out["depth"][miss]).all() and (out["depth"][miss] > 0).all()
    assert np.array_equal(out["depth"][~miss], (dep.reshape(20, 37)[~miss] / hits.reshape(20, 37)[~miss]))
    again = rtzig.render_features(cam.cam, cam.scene.world, 8)
    assert all(np.array_equal(out[k], again[k]) for k in out)

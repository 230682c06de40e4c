"""Every BASELINE.json GPU config at its STATED spp (SURVEY §8(d) parity targets), through the C ABI.

* bit-exact against oracle B (the reference arithmetic with the GPU's per-(pixel, sample) streams),
  in both unit modes (ring: in-kernel ordered accumulation; direct: stored samples + reduce pass):
  config 2 whole image at 100 spp; configs 3 and 4 on 8 interleaved rows at 500 spp (config 4 on
  the SAH tree and on the bench's trained tree); config 4's whole frame as bench.py runs it (one
  launch, trained tree, ring mode) at 100 and at its stated 500 spp; config 5 on one
  row at 10000 spp (2439 sample chunks: the in-kernel ordered accumulation hands each pixel's running
  sum from unit to unit, camera.zig:133-136);
* statistical against the reference's OWN images (SURVEY §8(c) ladder 3) for configs 2 and 3, whose
  seeds are unknown: per-channel image-mean |delta| <= 1.0 (8-bit units) and 8x8 box RMSE <= 1.5x
  the A-vs-B RMSE (oracle A's sequential stream vs oracle B's per-sample streams, same scene).
"""
import os

import numpy as np
import pytest

import rtzig
from gpu_support import box_rmse
from gpu_support import renderers  # noqa: F401 (fixture)
from oracle_lib import read_ppm

pytestmark = pytest.mark.gpu


def _rows(make, cam, row0, step, n, info=None):
    """Renders rows row0 + k*step, k < n, in one launch; `info` (a dict) receives the kernel name and
    the walk the launch used (rt_context_tree_info)."""
    import torch
    r = make(cam, timing=True)
    buf = torch.zeros((n, cam.width, 3), dtype=torch.float64, device="cuda:0")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    r.render_rows_async(cam.cam, buf.data_ptr(), row0=row0, row_step=step, n_rows=n, d_stats_ptr=stats.data_ptr())
    r.sync()
    launches = r.kernel_times_total()[2]
    if info is not None:
        info.update(r.tree_info(), kernel=r.kernel_name(), workspace=r.workspace_bytes())
    r.close()
    return buf.cpu().numpy(), [int(x) for x in stats.cpu().tolist()], launches


@pytest.mark.parametrize("mode", ["ring", "direct"])
def test_config2_full_image_100spp_bit_exact(oracle, mode, monkeypatch):
    """Config 2: chapter 9 (two Lambertian spheres), 400x225, 100 spp, depth 50 — every pixel, in
    both unit modes (direct is the default at this size)."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = rtzig.chapter9_camera(spp=100)
    st = {}
    out = rtzig.render(cam.cam, cam.scene.world, n_gpus=1, stats=st)
    ref, rays = oracle.render_b(cam.cam, cam.scene.world, threads=16)
    assert np.array_equal(out, ref)
    assert st["rays"] == rays and st["samples"] == 400 * 225 * 100


@pytest.mark.parametrize("config", ["chapter9", "chapter13"])
def test_configs2_3_statistically_match_reference_images(oracle, golden_dir, config):
    """Configs 2 and 3 vs the reference's images/chapter9.ppm and images/chapter13.ppm (400x225,
    100 spp): the GPU's fused-toRgb output against the fixture, with the A-vs-B noise floor."""
    cam = rtzig.chapter9_camera(spp=100) if config == "chapter9" else rtzig.chapter13_camera(width=400, spp=100)
    gpu = rtzig.render(cam.cam, cam.scene.world, n_gpus=1, output="rgb8")
    a, _ = oracle.render_a(cam.cam, cam.scene.world)
    b, _ = oracle.render_b(cam.cam, cam.scene.world, threads=16)
    floor = box_rmse(oracle.to_rgb8(a), oracle.to_rgb8(b))
    _, _, gold = read_ppm(open(os.path.join(golden_dir, f"{config}.ppm"), "rb").read())
    assert np.abs(gpu.astype(np.float64).mean(axis=(0, 1)) - gold.astype(np.float64).mean(axis=(0, 1))).max() <= 1.0
    assert box_rmse(gpu, gold) <= 1.5 * floor, (box_rmse(gpu, gold), floor)


@pytest.mark.parametrize("mode", ["ring", "direct"])
def test_config3_rows_500spp_bit_exact(oracle, mode, monkeypatch, renderers):
    """Config 3: chapter 13 scene + camera, 1200x675, 500 spp — 8 rows spread over the image."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = rtzig.chapter13_camera(width=1200, spp=500)
    assert (cam.width, cam.height) == (1200, 675)
    out, st, _ = _rows(renderers, cam, 3, 83, 8)
    ref, rays = oracle.render_b(cam.cam, cam.scene.world, row0=3, row_step=83, n_rows=8, threads=16)
    assert np.array_equal(out, ref)
    assert st == [rays, 8 * 1200 * 500]


@pytest.mark.parametrize("train", ["sah", "trained"])
@pytest.mark.parametrize("mode", ["ring", "direct"])
def test_config4_rows_500spp_bit_exact(oracle, mode, train, monkeypatch, renderers):
    """Config 4 (the bench workload): final scene, 1200x800, 500 spp — 8 rows spread over the image,
    on the SAH tree an 8-row launch builds by itself (4.8e6 samples, below the 2^25 training
    threshold) and on the tree trained on the 1200x800 camera's rays — the bench frame's tree
    (RTZIG_BVH_TRAIN=1; the training depends on the camera, not on the rows or the spp)."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    monkeypatch.setenv("RTZIG_BVH_TRAIN", "1" if train == "trained" else "0")
    cam = rtzig.final_scene_camera(width=1200, aspect_ratio=1.5, spp=500)
    assert (cam.width, cam.height, len(cam.scene.world)) == (1200, 800, 485)
    info = {}
    out, st, _ = _rows(renderers, cam, 7, 99, 8, info)
    assert info["bvh"] == 1 and info["trained"] == (train == "trained"), info
    ref, rays = oracle.render_b(cam.cam, cam.scene.world, row0=7, row_step=99, n_rows=8, threads=16)
    assert np.array_equal(out, ref)
    assert st == [rays, 8 * 1200 * 500]


@pytest.mark.parametrize("spp", [100, 500])
def test_config4_full_frame_bench_state_bit_exact(oracle, spp, renderers):
    """The bench's exact kernel state against the oracle, every pixel (reference: the row loop of
    camera.zig:123-145, HittableList.hit's first-wins scan hittable.zig:64-77): the whole 1200x800
    frame in ONE launch with the library's own choices — 9.6e7 / 4.8e8 samples, so the tree is the
    one trained on this camera's rays and the launch runs ring mode (its samples exceed direct
    mode's 2 GiB): the in-kernel ordered accumulation over 15 000 tiles, the LDS tree kernel
    `bvh_lds`, the chunk schedule of the stated spp.  500 spp is BASELINE config 4 itself, the
    frame bench.py times; oracle B on 16 host threads takes ~10 / ~45 s."""
    assert "RTZIG_UNIT_MODE" not in os.environ and "RTZIG_BVH_TRAIN" not in os.environ
    cam = rtzig.final_scene_camera(width=1200, aspect_ratio=1.5, spp=spp)
    info = {}
    out, st, launches = _rows(renderers, cam, 0, 1, 800, info)
    assert launches == 1
    assert info["kernel"] == "bvh_lds" and info["bvh"] == 1 and info["trained"] == 1, info
    assert info["workspace"] < 1 << 30, info  # ring + sums (~0.6 GiB), not direct mode's per-sample store
    ref, rays = oracle.render_b(cam.cam, cam.scene.world, threads=16)
    assert np.array_equal(out, ref), int((out != ref).any(axis=2).sum())
    assert st == [rays, 1200 * 800 * spp]


@pytest.mark.parametrize("mode", ["ring", "direct"])
def test_config5_row_10000spp_bit_exact(oracle, mode, monkeypatch, renderers):
    """Config 5: final scene at 3840x2160 (16/9), 10000 spp — one row in one launch (60 tiles x 2439
    sample chunks of rt_schedule.hpp, every pixel's running sum handed along 2438 units in ring
    mode; direct mode stores the row's 3.84e7 samples, 0.92 GB, and reduces them)."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = rtzig.final_scene_camera(width=3840, aspect_ratio=16 / 9, spp=10000)
    assert (cam.width, cam.height) == (3840, 2160)
    out, st, launches = _rows(renderers, cam, 1333, 1, 1)
    assert launches == 1  # one sample-kernel launch (+ the reduce pass in direct mode)
    ref, rays = oracle.render_b(cam.cam, cam.scene.world, row0=1333, row_step=1, n_rows=1, threads=16)
    assert np.array_equal(out, ref)
    assert st == [rays, 3840 * 10000]

"""Fast mode (RT_PRECISION_F32) against oracle mode F, sample by sample.

Oracle F feeds fast mode's specified random stream to the reference's operations, once in double
(F64, the reference) and once in float (F32, the yardstick for what f32 rounding alone does).  At
1 spp a pixel is one sample's colour, so the GPU is compared with F64 pixel by pixel, and what it
may differ by is bounded by what F32 differs by in the same test run — never by a stored GPU number.
One helper (fast_scenes.check_against_pair) applies one rule to every render here:

  divergence  share_gpu(theta) <= 2 * share_F32(theta) + 0.001 for theta in 1e-3, 1e-4, 1e-5, where
              share_x(theta) is the share of pixels whose max-channel |x - F64| exceeds theta
  cap         share_gpu(1e-3) <= 0.02, on inputs with share_F32(1e-3) <= 0.01
  bias        per channel |mean(gpu - F64)| <= 2 * |mean(F32 - F64)| + 4 * se(gpu - F64), over all
              pixels, diverged ones included
  rays        |rays_gpu - rays_F64| <= 2 * |rays_F32 - rays_F64| + 0.002 * rays_F64
  finite      every output value is finite
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fast_scenes as fs
import rtzig
from gpu_support import renderers  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

_pairs = {}


def pair_of(oracle, name):
    """The F64 / F32 reference pair of a scene of fast_scenes.SCENES, computed once per run."""
    if name not in _pairs:
        cam = fs.SCENES[name]()
        _pairs[name] = (cam, fs.reference_pair(oracle, cam))
    return _pairs[name]


def render_fast(make, cam, profile=False):
    """One fast-mode render into an f64 device buffer: (image, rays, samples, kernel name, tree info)."""
    H, W = cam.height, cam.width
    r = make(cam, "f32", profile=profile)
    out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    st = torch.zeros(rtzig.abi.RT_PROFILE_STATS_WORDS if profile else 2, dtype=torch.int64, device="cuda:0")
    r.render_rows_async(cam.cam, out.data_ptr(), d_stats_ptr=st.data_ptr())
    r.sync()
    name, tree = r.kernel_name(), r.tree_info()
    r.close()
    st = st.cpu().tolist()
    return out.cpu().numpy(), st[0], st[1], name, tree


def check_scene(oracle, make, scene, label, kernel="fast_f32_lds", mode=None, profile=False):
    cam, pair = pair_of(oracle, scene)
    img, rays, samples, name, tree = render_fast(make, cam, profile)
    assert name.startswith(kernel), name
    if mode is not None:
        assert ("direct" in name) == (mode == "direct"), name
    assert ("prof" in name) == profile, name
    assert samples == cam.width * cam.height * cam.cam.samples_per_pixel
    sg, _ = fs.check_against_pair(img, rays, pair, f"{label} kernel={name} always={tree['always']}")
    return img, sg, tree


def test_camera_and_primary_visibility(oracle, renderers):
    """Final scene, depth 1: a pixel is the sky behind the first hit or black, so this isolates the
    fast camera_start / camera_finish, the fast seed-window branch, the disk sample and primary
    visibility.  F32 and F64 agree to 1e-6 on every sample here (tests/test_oracle.py), so beyond
    the rule: share_gpu(1e-5) <= 0.001."""
    _, sg, _ = check_scene(oracle, renderers, "final_d1", "final_d1")
    assert sg[2] <= 0.001, sg


@pytest.mark.parametrize("mode", ["ring", "direct"])
@pytest.mark.parametrize("depth", [2, 50])
def test_final_scene_per_sample(oracle, depth, mode, monkeypatch, renderers):
    """Final scene (485 spheres, defocus, all materials; r = 1000 ground on the f64 side of the
    always-list split) after one scatter and at full depth, in both unit modes."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    check_scene(oracle, renderers, f"final_d{depth}", f"final_d{depth}/{mode}", mode=mode)


@pytest.mark.parametrize("scene", ["chapter13", "chapter9", "materials"])
def test_materials_per_sample(oracle, scene, renderers):
    """Chapter 13: hollow glass, fuzz-1 metal, defocus 10, r = 100 ground (r^2 exactly 1e4: f64 side).
    Chapter 9: two Lambertian spheres, no defocus.  `materials`: fuzz > 1 absorption, a zero-radius
    sphere, an exact duplicate, inside-glass paths.
    Chapter 9 failed the rays rule (58 304 against 57 898) while its r = 100 ground sat in an f32 leaf;
    a Schlick term with x^2 for x^4 fails chapter 13 (share 2.29% at 1e-3) and `materials` (1.83%)."""
    check_scene(oracle, renderers, scene, scene)


@pytest.mark.parametrize("scene", ["final_d2_tmax1.2", "chapter13_tmax1.1", "final_d2_seed63"])
def test_finite_interval_max_and_a_64_bit_seed(oracle, scene, renderers):
    """A finite t_max (fast mode starts `closest` from its f32 cast) and a seed with bit 63 set, held to
    the same rule.  The references show the inputs are not the default ones: the finite interval or
    the other seed changes more than a tenth of oracle F64's pixels."""
    check_scene(oracle, renderers, scene, scene)
    base = "chapter13" if scene.startswith("chapter13") else "final_d2"
    moved = (pair_of(oracle, scene)[1][0] != pair_of(oracle, base)[1][0]).any(axis=-1).mean()
    assert moved > 0.10, moved


@pytest.mark.parametrize("scene", ["ground_99.9", "ground_100.1", "c1_straddle"])
def test_always_list_split(oracle, scene, renderers):
    """always_f32's f32 / f64 split at r^2 < 1e4 and |c|_1 < 1e4: the same scene on a ground of radius
    99.9 (f32 test) and 100.1 (f64 test), and two distant spheres whose |c|_1 is 9 990 and 10 010.
    The spheres in question must be always-list entries for the split to be what is exercised."""
    _, _, tree = check_scene(oracle, renderers, scene, scene)
    assert tree["always"] >= (2 if scene == "c1_straddle" else 1), tree


def test_everything_in_the_tree(oracle, monkeypatch, renderers):
    """No always-list (both builder criteria off): every sphere, the radius-99.9 ground included,
    is tested by leaf_f32, and held to the same rule."""
    monkeypatch.setenv("RTZIG_BVH_ALWAYS_AREA", "0")
    monkeypatch.setenv("RTZIG_BVH_ALWAYS_REL", "0")
    _, _, tree = check_scene(oracle, renderers, "ground_99.9", "ground_99.9/no-always")
    assert tree["always"] == 0, tree


def test_global_memory_kernel(oracle, renderers):
    """2600 spheres do not fit in LDS: a fast_f32_global kernel, never launched by another test."""
    check_scene(oracle, renderers, "large_2600", "large_2600", kernel="fast_f32_global")


@pytest.mark.parametrize("mode", ["ring", "direct"])
def test_profiled_kernels(oracle, mode, monkeypatch, renderers):
    """The instrumented fast instantiations with a 72-word stats buffer: a (prof) kernel, held to
    the rule, and bit-identical to the unprofiled fast render of the same call (in ring mode it was
    not, in 300 of 38 400 pixels, while fm::dot left the choice of the fused product to the compiler)."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam, _ = pair_of(oracle, "final_d50")
    plain, _, _, name, _ = render_fast(renderers, cam)
    assert "prof" not in name
    img, _, _ = check_scene(oracle, renderers, "final_d50", f"final_d50/prof/{mode}", mode=mode, profile=True)
    assert np.array_equal(img, plain)


@pytest.mark.parametrize("mode", ["ring", "direct"])
@pytest.mark.parametrize("scene", ["final_w64_spp3_d2", "final_w64_spp17_d1", "chapter13_w64_spp17"])
def test_more_than_one_sample_per_pixel(oracle, scene, mode, monkeypatch, renderers):
    """Per-pixel averages at spp 3 and 17 against F's averages (samples added in sample order), in
    both unit modes; theta applies to the pixel average.  The depths are those at which the input
    condition holds (fast_scenes.SCENES)."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    _, sg, _ = check_scene(oracle, renderers, scene, f"{scene}/{mode}", mode=mode)
    if scene.endswith("_d1"):  # as test_camera_and_primary_visibility: F32 == F64 to 1e-6 here
        assert sg[2] <= 0.001, sg


def test_rgb8_stride_and_device_map(oracle, monkeypatch, renderers):
    """Output plumbing of fast mode through rt_render: RT_OUT_RGB8 equals to_rgb8 of the f64-buffer
    render byte for byte; pixel_stride = 4 leaves the fourth lane untouched; three logical devices
    mapped onto GPU 0 (n_gpus = 0) are bit-identical to the single-device render."""
    cam, pair = pair_of(oracle, "final_d50")
    one = rtzig.render(cam.cam, cam.scene.world, n_gpus=1, precision="f32")
    dev, rays, _, _, _ = render_fast(renderers, cam)
    assert np.array_equal(one, dev)
    rgb = rtzig.render(cam.cam, cam.scene.world, n_gpus=1, output="rgb8", precision="f32")
    assert np.array_equal(rgb, rtzig.to_rgb8(one))
    assert np.array_equal(rgb, oracle.to_rgb8(one))

    monkeypatch.setenv("RTZIG_DEVICE_MAP", "0,0,0")
    lib = rtzig.load()
    out = np.full((cam.height, cam.width, 4), -7.0)
    st = (C.c_uint64 * 2)()
    opts = rtzig.RtOptions(n_gpus=0, pixel_stride=4, output_format=0, precision=rtzig.abi.RT_PRECISION_F32,
                           stats_out=C.cast(st, C.POINTER(C.c_uint64)))
    rc = lib.rt_render(C.byref(cam.cam), cam.scene.world, len(cam.scene.world), C.byref(opts),
                       out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.rt_last_error()
    assert np.array_equal(out[..., :3], one) and (out[..., 3] == -7.0).all()
    assert st[0] == rays and st[1] == cam.width * cam.height
    fs.check_against_pair(out[..., :3].copy(), st[0], pair, "final_d50/device-map")

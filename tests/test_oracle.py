"""Pins the CPU oracle against the reference's own fixtures and known-answer tests.

The only end-to-end golden in the reference is test "main" (src/main.zig:41-55): final scene,
seed 0xdeadbeef, width 400, 16/9, 10 spp, byte-exact vs test-files/chapter14.ppm.  The KATs below
restate the reference's unit tests (file:line cited per test).
"""
import math
import os

import numpy as np
import pytest

from fast_scenes import golden_params
from gpu_support import box_rmse
from oracle_lib import read_ppm
from rtzig.abi import D3, RT_DIELECTRIC, RT_LAMBERTIAN, RT_METAL, RtCameraParams, RtSphere

INF = math.inf


def test_golden_chapter14_byte_exact(oracle, golden_dir):
    """main.zig:41-55: render with the sequential stream == test-files/chapter14.ppm."""
    spheres, state = oracle.scene_final(0xDEADBEEF)
    assert len(spheres) == 485
    cam = oracle.camera_build(golden_params())
    assert (cam.image_width, cam.image_height) == (400, 225)
    lin, rays = oracle.render_a(cam, spheres, state)
    data = oracle.ppm_p6(oracle.to_rgb8(lin), 400, 225)
    gold = open(os.path.join(golden_dir, "chapter14.ppm"), "rb").read()
    assert len(data) == len(gold) == 270016
    assert data == gold
    assert rays == 2379984  # world.hit calls for this render (recorded by the pinned oracle)


def test_scene_counts(oracle):
    """Scene.zig:189-205: seed 0xabadcafe -> 1 + 3 + 22*22 - 3 objects."""
    spheres, _ = oracle.scene_final(0xABADCAFE)
    assert len(spheres) == 1 + 3 + 22 * 22 - 3
    spheres, _ = oracle.scene_final(0xDEADBEEF)
    kinds = np.array([s.material for s in spheres])
    assert len(spheres) == 485
    # 1 ground + 382 lambertian + 68 metal + 31 glass small spheres + 3 big
    assert (kinds == RT_LAMBERTIAN).sum() == 1 + 382 + 1
    assert (kinds == RT_METAL).sum() == 68 + 1
    assert (kinds == RT_DIELECTRIC).sum() == 31 + 1


def test_chapter13_scene(oracle):
    s = oracle.scene_chapter13()
    assert len(s) == 5
    assert list(s[3].center) == [-1, 0, -1] and s[3].radius == 0.4
    assert s[3].refraction_index == 1.0 / 1.5
    assert s[4].material == RT_METAL and s[4].fuzz == 1


def test_camera_kat(oracle):
    """camera.zig:516-535: 400 x 16/9, viewport((0,0,0),(0,0,-1),90), focus 10."""
    p = RtCameraParams(image_width=400, samples_per_pixel=100, bounce_max=50,
                       aspect_ratio=16.0 / 9.0, look_from=D3(0, 0, 0), look_at=D3(0, 0, -1),
                       v_up=D3(0, 1, 0), vfov=90, defocus_angle=0, focus_dist=10,
                       t_min=1e-3, t_max=INF, seed=1)
    cam = oracle.camera_build(p)
    assert cam.image_height == 225
    assert list(cam.du) == [8.888888888888888e-2, 0.0, 0.0]
    assert list(cam.dv) == [0.0, -8.888888888888888e-2, 0.0]
    assert list(cam.pixel0) == [-1.773333333333333e1, 9.955555555555554e0, -1e1]
    assert cam.pixel_samples_scale == 1 / 100
    assert list(cam.defocus_disk_u) == [0, 0, 0]


def test_color_kat(oracle):
    """color.zig:157-163 toRgb(0, 0.5, 0.75) = (0, 181, 221); color.zig:165-172 gamma."""
    rgb = oracle.to_rgb8(np.array([[0.0, 0.5, 0.75]]))
    assert rgb.tolist() == [[0, 181, 221]]
    rgb = oracle.to_rgb8(np.array([[1.0, 0.0, 1.0], [-1.0, 4.0, 1e9]]))
    assert rgb.tolist() == [[255, 0, 255], [0, 255, 255]]


def test_color_byte_boundaries_need_a_correctly_rounded_sqrt(oracle):
    """Byte k starts at (k/256)^2.  The neighbour just below it rounds back up to k/256 under a
    correctly rounded sqrt for 102 of the 255 boundaries and stays at byte k - 1 for the other 153:
    these inputs tell a sqrt that is one ulp off (tests/domain_values.py feeds them to the device)."""
    import domain_values as dv
    k = np.arange(1, 256)
    sq = (k / 256.0) ** 2
    byte = lambda x: oracle.to_rgb8(np.stack([x, x, x], 1))[:, 0]
    assert np.array_equal(byte(sq), k) and np.array_equal(byte(np.nextafter(sq, 2.0)), k)
    below = byte(np.nextafter(sq, 0.0))
    assert int((below == k).sum()) == 102 and int((below == k - 1).sum()) == 153
    assert np.array_equal(below == k, np.sqrt(np.nextafter(sq, 0.0)) == k / 256.0)
    x = 0.999 * 0.999  # the clamp's corner: 256 * 0.999 = 255.744
    assert byte(np.array([np.nextafter(x, 0.0), x, np.nextafter(x, 2.0), 1.0, 1.5, np.inf])).tolist() == [255] * 6
    assert byte(np.array([0.0, -0.0, -0.3, 5e-324, 1e-320, np.nan])).tolist() == [0] * 6
    import rtzig
    a = dv.pixels(len(dv.channel_values()))
    assert np.array_equal(rtzig.to_rgb8(a), oracle.to_rgb8(a))  # the product's host Color.toRgb too


def _sphere(center, radius, kind=RT_LAMBERTIAN, albedo=(1, 1, 1), fuzz=0.0, ior=1.0):
    return RtSphere(center=D3(*center), radius=radius, material=kind, albedo=D3(*albedo),
                    fuzz=fuzz, refraction_index=ior)


def test_sphere_hit_kat(oracle):
    """sphere.zig:76-98 hit() success; :100-117 out of range; :119-136 no hit."""
    s = _sphere((0, 0, -2), 1.0)
    rec = oracle.sphere_hit(s, (0, 0, 0), (0, 0, -1), 0.0, 3.0)
    assert rec is not None
    assert rec["t"] == 1 and rec["point"] == [0, 0, -1] and rec["normal"] == [0, 0, 1] and rec["front"]
    assert oracle.sphere_hit(s, (0, 0, 0), (0, 0, -1), 0.0, 0.0) is None
    assert oracle.sphere_hit(s, (0, 0, 0), (0, 0, 1), 0.0, 3.0) is None


def test_hittable_list_kat(oracle):
    """hittable.zig:185-209: 4 spheres on -z, interval (-6, 6) -> first sphere, t = 1."""
    arr = (RtSphere * 4)(*[_sphere((0, 0, -z), 1.0) for z in (2, 3, 4, 5)])
    k, t = oracle.world_hit(arr, (0, 0, 0), (0, 0, -1), -6, 6)
    assert k == 0 and t == 1
    # ties: a later sphere at exactly the same t never replaces the earlier one (strict <)
    arr = (RtSphere * 2)(_sphere((0, 0, -2), 1.0), _sphere((0, 0, -2), 1.0))
    k, t = oracle.world_hit(arr, (0, 0, 0), (0, 0, -1), 1e-3, INF)
    assert k == 0 and t == 1


def test_vec_kat(oracle):
    """material.zig:196-220 (metal fuzz 0 == reflect), :222-246 (dielectric refract eta 1/1.5)."""
    assert oracle.reflect((0, 0, -1), (0, 0, 1)) == [0, 0, 1]
    r = oracle.refract((0, 0, -1), (0, 0, 1), 1.0 / 1.5)
    assert r == [0, 0, -1]
    r = oracle.reflect((1, -1, 0), (0, 1, 0))
    assert r == [1, 1, 0]


def test_ppm_binary_fixture(oracle, golden_dir):
    """ppm.zig:92-105: 1x1 black P6 == test-files/test-binary.ppm."""
    data = oracle.ppm_p6(np.zeros((1, 1, 3), np.uint8), 1, 1)
    assert data == open(os.path.join(golden_dir, "test-binary.ppm"), "rb").read()
    assert data == b"P6\n1 1\n255\n\x00\x00\x00\n"


def test_rng_self_consistency(oracle):
    """util.zig:33-86: same seed -> same draws; draws in [0, 1)."""
    a = oracle.random_doubles(0xCAFEF00D, 1000)
    b = oracle.random_doubles(0xCAFEF00D, 1000)
    assert np.array_equal(a, b)
    assert a[0] != a[1]
    assert (a >= 0).all() and (a < 1).all()
    # Xoshiro256++ from SplitMix64(0): first word is a fixed published-algorithm value
    w = oracle.random_u64(0, 2)
    assert int(w[0]) == 0x53175D61490B23DF


def test_sample_key_bijective(oracle):
    keys = {oracle.sample_key(0xDEADBEEF, p, s) for p in range(64) for s in range(64)}
    assert len(keys) == 64 * 64


def test_oracle_b_statistically_matches_golden(oracle, golden_dir):
    """Parity ladder step 3: the per-sample-stream render (B) differs from the
    sequential-stream golden only by RNG noise.  Tolerance: |mean_B - mean_gold| <= 1.0 per channel
    (8-bit units); 8x8 box RMSE <= 2.0."""
    from oracle_lib import read_ppm
    spheres, _ = oracle.scene_final(0xDEADBEEF)
    cam = oracle.camera_build(golden_params())
    lin, _ = oracle.render_b(cam, spheres, threads=8)
    rgb = oracle.to_rgb8(lin).astype(np.float64)
    _, _, gold = read_ppm(open(os.path.join(golden_dir, "chapter14.ppm"), "rb").read())
    gold = gold.astype(np.float64)
    assert np.abs(rgb.mean(axis=(0, 1)) - gold.mean(axis=(0, 1))).max() <= 1.0
    box = lambda x: x[:224].reshape(28, 8, 50, 8, 3).mean(axis=(1, 3))
    assert np.sqrt(((box(rgb) - box(gold)) ** 2).mean()) <= 2.0


@pytest.mark.parametrize("chapter", [4, 5, 6])
def test_config1_book_chapter_byte_exact(oracle, golden_dir, chapter):
    """BASELINE config 1 (chapter5 single sphere, 400x225, 1 spp, CPU plumbing + PPM diff): the
    book renderer restated in the oracle + the P6 writer reproduce test-files/chapter{4,5}.ppm and
    the "normals" variant test-files/chapter6.ppm (sphere + ground, 0.5 * (normal + 1), walked by
    HittableList.hit / Sphere.hit on (0, inf))."""
    rgb = oracle.render_book(chapter)
    data = oracle.ppm_p6(rgb, 400, 225)
    assert data == open(os.path.join(golden_dir, f"chapter{chapter}.ppm"), "rb").read()
    import rtzig
    assert rtzig.encode_p6(rgb, 400, 225) == data  # the product's P6 writer too


def test_config1_normals_antialiased_statistical(oracle, golden_dir):
    """test-files/chapter7.ppm is the chapter-6 normals scene antialiased (jittered samples per
    pixel, Interval.clamp + 256 quantisation).  Its RNG stream is unknown, so it is compared
    statistically with the oracle's 100-spp render: per-channel mean |delta| <= 1.0 (8-bit units),
    mean absolute difference <= 0.6, 98% of pixels within 2 levels (the rest are silhouette pixels)."""
    rgb = oracle.render_book(7).astype(np.float64)
    _, _, gold = read_ppm(open(os.path.join(golden_dir, "chapter7.ppm"), "rb").read())
    gold = gold.astype(np.float64)
    assert np.abs(rgb.mean(axis=(0, 1)) - gold.mean(axis=(0, 1))).max() <= 1.0
    assert np.abs(rgb - gold).mean() <= 0.6
    assert (np.abs(rgb - gold).max(axis=2) <= 2).mean() >= 0.98


@pytest.mark.parametrize("config", ["chapter9", "chapter13"])
def test_presets_statistically_match_reference_images(oracle, golden_dir, config):
    """Configs 2 and 3 have no byte-exact pin: the reference's images/chapter9.ppm and
    images/chapter13.ppm come from the book-chapter code at an unknown seed.  The presets
    (rtzig.chapter9_camera / chapter13_camera at 400x225, 100 spp) are pinned statistically with the
    SURVEY §8(c) ladder-3 rule: per-channel image-mean |delta| <= 1.0 and 8x8 box RMSE <= 1.5x the
    A-vs-B RMSE (oracle A's sequential stream vs oracle B's per-sample streams, same scene)."""
    import rtzig
    cam = rtzig.chapter9_camera(spp=100) if config == "chapter9" else rtzig.chapter13_camera(width=400, spp=100)
    a, _ = oracle.render_a(cam.cam, cam.scene.world)
    b, _ = oracle.render_b(cam.cam, cam.scene.world, threads=8)
    A, B = oracle.to_rgb8(a), oracle.to_rgb8(b)
    _, _, gold = read_ppm(open(os.path.join(golden_dir, f"{config}.ppm"), "rb").read())
    floor = box_rmse(A, B)
    assert np.abs(B.astype(np.float64).mean(axis=(0, 1)) - gold.astype(np.float64).mean(axis=(0, 1))).max() <= 1.0
    assert box_rmse(B, gold) <= 1.5 * floor, (box_rmse(B, gold), floor)


# ---- oracle_accumulate_b: a sample range added onto stored sums ----------------------------------
def _cam37(spp, oracle):
    return oracle.camera_build(golden_params(width=37, spp=spp))


@pytest.mark.parametrize("split", [[12], [1, 11], [5, 7], [4, 1, 7], [3] * 4], ids=lambda s: "-".join(map(str, s)))
def test_accumulate_b_chained_splits_equal_render_b(oracle, split):
    """Chained calls over any split of [0, n), scaled once by 1.0 / n, have the bits of oracle_render_b
    at spp = n (camera.zig:133-137: samples added in order, one scale), and the calls' rays sum to its."""
    spheres, _ = oracle.scene_final(0xDEADBEEF)
    n = sum(split)
    cam = _cam37(n, oracle)
    ref, ref_rays = oracle.render_b(cam, spheres, threads=8)
    sums, rays, done = None, 0, 0
    for count in split:
        sums, r = oracle.accumulate_b(cam, spheres, done, count, sums, threads=8)
        rays += r
        done += count
    assert np.array_equal(sums * (1.0 / n), ref)
    assert rays == ref_rays
    # a row subset, and a thread count that must not matter
    sub, _ = oracle.accumulate_b(cam, spheres, 0, n, row0=1, row_step=3, n_rows=6, threads=1)
    assert np.array_equal(sub * (1.0 / n), ref[1:19:3])


def test_accumulate_b_keys_with_the_64_bit_sample_number(oracle):
    """A range that ends at 2^32 - 1 differs from the one 2^31 lower (bit 31 of the sample number
    reaches the key), and the additions start from `sums`."""
    spheres, _ = oracle.scene_final(0xDEADBEEF)
    cam = _cam37(1, oracle)
    k = 5
    hi, _ = oracle.accumulate_b(cam, spheres, 2 ** 32 - 1 - k, k, threads=8)
    lo, _ = oracle.accumulate_b(cam, spheres, 2 ** 31 - 1 - k, k, threads=8)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    assert (hi != lo).any(axis=-1).mean() > 0.9
    first, _ = oracle.accumulate_b(cam, spheres, 0, 1, threads=8)
    seeded = np.full((20, 37, 3), 0.375)
    got, _ = oracle.accumulate_b(cam, spheres, 0, 1, seeded, threads=8)
    assert np.array_equal(got, 0.375 + first) and (seeded == 0.375).all()


# ---- oracle mode F: the per-sample reference of the f32 fast mode ---------------
def test_mode_f_arithmetic_matches_mode_b_on_b_stream(oracle):
    """F's 64-bit instantiation fed mode B's stream (render_f_wide: one Random.float(f64) per
    uniform) restates the same operations as B from f32-rounded inputs, so the two agree within 1e-6
    on every pixel except those where the ~1e-7 input rounding moves a ray across a silhouette:
    none at depth 1, 0.03% at depth 2, 0.57% at depth 50 on the final scene (240x160, 1 spp),
    capped at 1%.  (On F's own stream the two cannot be compared per pixel: B draws the two
    sampleSquare offsets from two words, F from the halves of one.)"""
    import fast_scenes as fs
    for depth in (1, 2, 50):
        cam = fs.final(depth)
        b, rays_b = oracle.render_b(cam.cam, cam.scene.world, threads=8)
        f, rays_f = oracle.render_f_wide(cam.cam, cam.scene.world, threads=8)
        share = float((np.abs(b - f).max(axis=-1) > 1e-6).mean())
        assert share <= 0.01, (depth, share)
        assert abs(rays_b - rays_f) <= 0.002 * rays_b, (depth, rays_b, rays_f)


def test_mode_f_stream_layout(oracle):
    """§5.6's draw layout restated in numpy for the first draw of a sample: sampleSquare's x offset is
    the top 24 bits of the high half of word 0, its y offset the top 24 bits of the low half.
    Chapter 9's camera (no defocus) at depth 1 on sky pixels: the colour is the sky gradient
    (camera.zig:171-177) of the ray through that sample point."""
    import fast_scenes as fs
    cam = fs.chapter9()
    c = cam.cam
    c.bounce_max = 1
    f64, _ = oracle.render_f(c, cam.scene.world, 64)
    r32 = lambda v: np.array([np.float32(x) for x in v], np.float64)
    p0, du, dv, center = r32(c.pixel0), r32(c.du), r32(c.dv), r32(c.center)
    for i, j in ((0, 0), (17, 3), (239, 0), (120, 20)):
        w = int(oracle.random_u64(oracle.sample_key(c.seed, j * c.image_width + i, 0), 1)[0])
        ox = (w >> 40) * 2.0 ** -24 - 0.5
        oy = ((w & 0xFFFFFFFF) >> 8) * 2.0 ** -24 - 0.5
        d = (p0 + du * (i + ox)) + dv * (j + oy) - center
        a = 0.5 * (d[1] / np.sqrt(d @ d) + 1.0)
        sky = (1.0 - a) * np.ones(3) + a * np.array([0.5, 0.7, 1.0])
        assert np.abs(f64[j, i] - sky).max() < 1e-12, (i, j, f64[j, i], sky)


def test_mode_f_instantiations_consume_the_same_draws(oracle):
    """The 64- and 32-bit instantiations read the same stream: identical Xoshiro word and ray counts
    where no rejection or branch sits within f32 rounding of its boundary (final scene at depth 1;
    chapter 9, all Lambertian, at depth 50)."""
    import fast_scenes as fs
    for name in ("final_d1", "chapter9"):
        cam = fs.SCENES[name]()
        d64, d32 = {}, {}
        _, r64 = oracle.render_f(cam.cam, cam.scene.world, 64, threads=8, draws=d64)
        _, r32 = oracle.render_f(cam.cam, cam.scene.world, 32, threads=8, draws=d32)
        assert d64["words"] == d32["words"] > cam.width * cam.height and r64 == r32, (name, d64, d32, r64, r32)


def test_mode_f_inputs_stay_under_the_divergence_cap(oracle):
    """The input condition of tests/test_fast_oracle.py, checked where it can fail with a clear
    message: on every scene there, F32 differs from F64 by more than 1e-3 on at most 1% of the
    pixels (and both are finite).  A scene that drifts over it is replaced, not tolerated."""
    import fast_scenes as fs
    for name, make in fs.SCENES.items():
        cam = make()
        f64, _, f32, _ = fs.reference_pair(oracle, cam)
        assert np.isfinite(f64).all() and np.isfinite(f32).all(), name
        share = fs.shares(f32, f64)
        print(f"MODEF {name} {cam.width}x{cam.height} share_f32={share}")
        assert share[0] <= fs.INPUT_CAP, f"{name}: share_F32(1e-3) = {share[0]} > {fs.INPUT_CAP}"
    cam = fs.SCENES["final_d1"]()  # the depth-1 cases assert share_gpu(1e-5) directly: F32 == F64 here
    f64, _, f32, _ = fs.reference_pair(oracle, cam)
    assert np.abs(f32 - f64).max() <= 1e-6

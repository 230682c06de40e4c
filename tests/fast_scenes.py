"""Cameras and scenes of the fast-mode per-sample oracle tests, and the one rule they apply.

Shared by tests/test_oracle.py (CPU: oracle F's 32-bit instantiation against its 64-bit one) and
tests/test_fast_oracle.py (GPU: the f32 fast mode against the same pair).  Everything is rendered at
1 sample per pixel unless stated, so a pixel is one sample's colour.

Also the scene and parameter builders that more than one test file uses: always_list_scene and
far_origin_scene (tests/test_gpu_parity.py, tests/test_gpu_domain.py) and golden_params, the golden
test's camera preset (tests/test_oracle.py, tests/test_host.py, tests/test_gpu_parity.py); lattice and
skim_camera, the scene and the camera of the slab-certificate tests (tests/test_slab_inputs.py,
tests/test_gpu_slab.py).
"""
import math

import numpy as np

import rtzig
from rtzig.abi import D3, RT_DIELECTRIC, RT_LAMBERTIAN, RT_METAL, RtCamera, RtCameraParams, RtSphere

INF = math.inf
THETAS = (1e-3, 1e-4, 1e-5)
INPUT_CAP = 0.01  # share_F32(1e-3) every scene below must stay under (checked on the CPU)
GPU_CAP = 0.02    # share_gpu(1e-3), whatever F32 says


def final(depth, width=240, spp=1):
    return rtzig.final_scene_camera(width=width, aspect_ratio=1.5, spp=spp, bounce_max=depth)


def chapter13(width=240, spp=1):
    return rtzig.chapter13_camera(width=width, spp=spp)


def chapter9():
    return rtzig.chapter9_camera(width=240, spp=1)


def materials():
    """The scene of test_gpu_parity.test_materials_and_degenerate_spheres: fuzz > 1 absorption, a
    zero-radius sphere, an exact duplicate and inside-glass paths."""
    scene = rtzig.Scene.init(0x1234)
    scene.add((0, -100.5, -1), 100, RT_LAMBERTIAN, albedo=(0.8, 0.8, 0.0))
    scene.add((0, 0, -1.2), 0.5, RT_METAL, albedo=(0.9, 0.9, 0.9), fuzz=1.7)
    scene.add((-1, 0, -1), 0.5, RT_DIELECTRIC, refraction_index=1.5)
    scene.add((-1, 0, -1), 0.4, RT_DIELECTRIC, refraction_index=1.0 / 1.5)
    scene.add((1, 0, -1), 0.5, RT_METAL, albedo=(0.8, 0.6, 0.2), fuzz=0.0)
    scene.add((1, 0, -1), 0.5, RT_LAMBERTIAN, albedo=(0.1, 0.1, 0.9))  # exact duplicate: never wins
    scene.add((0, 1, -1), -0.3, RT_LAMBERTIAN)                          # radius clamps to 0
    return (rtzig.Camera.builder(240, 16 / 9).setScene(scene).setDefocusAngle(2.0).setFocusDist(1.5)
            .setViewport((0, 0.3, 0.5), (0, 0, -1), 70).setSamplesPerPixel(1).build())


def ground(radius):
    """Chapter 13's spheres on a ground of the given radius whose top stays at y = -0.5: at 99.9
    the ground's r^2 < 1e4 (f32 sphere test), at 100.1 it is on the f64 side of the split."""
    scene = rtzig.Scene.init(0xC0FFEE)
    scene.add((0, -0.5 - radius, -1), radius, RT_LAMBERTIAN, albedo=(0.8, 0.8, 0.0))
    scene.add((0, 0, -1.2), 0.5, RT_LAMBERTIAN, albedo=(0.1, 0.2, 0.5))
    scene.add((-1, 0, -1), 0.5, RT_DIELECTRIC, refraction_index=1.5)
    scene.add((-1, 0, -1), 0.4, RT_DIELECTRIC, refraction_index=1.0 / 1.5)
    scene.add((1, 0, -1), 0.5, RT_METAL, albedo=(0.8, 0.6, 0.2), fuzz=0.3)
    return (rtzig.Camera.builder(240, 16 / 9).setScene(scene).setDefocusAngle(1.0).setFocusDist(3.4)
            .setViewport((-2, 2, 1), (0, 0, -1), 25).setSamplesPerPixel(1).build())


def c1_straddle(depth=1):
    """Two radius-90 spheres 9 900 units away whose |c|_1 is 9 990 (f32 test) and 10 010 (f64
    test), behind three small spheres that make them always-list entries (10x the median box).
    Depth 1 (primary visibility through both sides of the split): a |c|_1 of 1e4 needs a coordinate
    of 3 333 or more, where an f32 hit point is known to 2.4e-4 or worse against t_min = 1e-3, so
    rays leaving such a sphere re-hit it in any f32 arithmetic and share_F32(1e-3) is 3.8% at depth 2."""
    scene = rtzig.Scene.init(0xFACADE)
    scene.add((-60, 30, -9900), 90, RT_LAMBERTIAN, albedo=(0.8, 0.3, 0.3))
    scene.add((60, 30, -9920), 90, RT_LAMBERTIAN, albedo=(0.3, 0.3, 0.8))
    scene.add((-1.1, -0.8, -60), 0.5, RT_DIELECTRIC, refraction_index=1.5)
    scene.add((0, -0.8, -60), 0.5, RT_METAL, albedo=(0.8, 0.8, 0.8), fuzz=0.1)
    scene.add((1.1, -0.8, -60), 0.5, RT_LAMBERTIAN, albedo=(0.2, 0.7, 0.2))
    return (rtzig.Camera.builder(240, 1.5).setScene(scene).setDefocusAngle(0.0).setFocusDist(10)
            .setViewport((0, 0, 0), (0, 0, -1), 3).setSamplesPerPixel(1).setBounceMax(depth).build())


def large():
    """The 2600-sphere scene of test_gpu_parity.test_large_scene_global_memory_variant (more
    spheres than the LDS holds), 96 wide at 2 spp.  Depth 3: its overlapping random spheres diverge
    more than any other scene here, share_F32(1e-3) = 0.54% at depth 3, 0.93% at 4, 1.6% at 50."""
    rng = np.random.default_rng(11)
    n = 2600
    arr = (RtSphere * n)()
    arr[0] = RtSphere(center=D3(0, -1000, 0), radius=1000, material=RT_LAMBERTIAN, albedo=D3(0.5, 0.5, 0.5))
    for k in range(1, n):
        arr[k] = RtSphere(center=D3(*rng.uniform([-30, 0.1, -30], [30, 3, 30])),
                          radius=float(rng.uniform(0.05, 0.3)), material=int(k % 3),
                          albedo=D3(*rng.uniform(0, 1, 3)), fuzz=float(rng.uniform(0, 0.5)),
                          refraction_index=1.5)
    scene = rtzig.Scene.init(77)
    scene.world = arr
    return (rtzig.Camera.builder(96, 16 / 9).setScene(scene).setDefocusAngle(0.6).setFocusDist(10)
            .setViewport((13, 2, 3), (0, 0, 0), 20).setSamplesPerPixel(2).setBounceMax(3).build())


def always_list_scene(n_big, ground, n_unbound):
    """The scene and camera of test_always_list_sizes_bit_exact (64 x 42, 4 spp): a grid of small
    spheres with n_big radius-1.2 spheres among them, an optional radius-1000 ground and n_unbound
    spheres centred at 2e30."""
    rng = np.random.default_rng(100 + 10 * n_big + n_unbound + (5 if ground else 0))
    sph = []
    for a in range(-4, 4):
        for b in range(-4, 4):
            sph.append(RtSphere(center=D3(a + 0.9 * rng.uniform(), 0.2, b + 0.9 * rng.uniform()), radius=0.2,
                                material=int(rng.integers(0, 3)), albedo=D3(*rng.uniform(0, 1, 3)),
                                fuzz=float(rng.uniform(0, 0.5)), refraction_index=1.5))
    for k in range(n_big):
        sph.append(RtSphere(center=D3(-3.0 + 2.0 * k, 1.2, 0.3 * k), radius=1.2, material=k % 3,
                            albedo=D3(0.7, 0.6, 0.5), fuzz=0.0, refraction_index=1.5))
    if ground:
        sph.insert(int(rng.integers(0, len(sph))), RtSphere(center=D3(0, -1000, 0), radius=1000.0, material=0,
                                                            albedo=D3(0.5, 0.5, 0.5)))
    for k in range(n_unbound):
        sph.insert(int(rng.integers(0, len(sph))), RtSphere(center=D3(2e30, 1.0 + k, 0), radius=1.0, material=0,
                                                            albedo=D3(0.5, 0.5, 0.5)))
    arr = (RtSphere * len(sph))(*sph)
    scene = rtzig.Scene.init(7)
    scene.world = arr
    cam = (rtzig.Camera.builder(64, 1.5).setScene(scene).setDefocusAngle(0.6).setFocusDist(10.0)
           .setViewport((13, 2, 3), (0, 0, 0), 20.0).setSamplesPerPixel(4).build())
    return arr, cam


def far_origin_scene(width=96):
    """The scene and camera of test_far_origin_lanes_walk_without_culling: the final scene of seed
    0xfa7 plus an unboundable radius-2e30 metal sphere."""
    scene = rtzig.Scene.init(0xfa7).generateWorld()
    huge = RtSphere(center=D3(0, -2e30, 0), radius=2e30, material=RT_METAL, albedo=D3(0.7, 0.7, 0.7), fuzz=0.3)
    arr = (RtSphere * (len(scene.world) + 1))(*scene.world, huge)
    scene.world = arr
    cam = (rtzig.Camera.builder(width, 1.5).setScene(scene).setDefocusAngle(0.6).setFocusDist(10)
           .setViewport((13, 2, 3), (0, 0, 0), 20).setSamplesPerPixel(4).build())
    return arr, cam


def lattice(T=0):
    """The scene of the slab-certificate tests (tests/slab_support.py): a 4 x 4 x 4 lattice of radius-0.25
    spheres at unit spacing, translated by (T, T / 2, -T).  Equal spheres: none is big against the
    median, so none goes to the always-list, and the poles of a layer share one plane, which is a face
    of every box on the way.  Materials by index: lambertian, metal, dielectric in turn."""
    sph = []
    for i in range(4):
        for j in range(4):
            for k in range(4):
                n = len(sph)
                sph.append(RtSphere(center=D3(i + T, j + T / 2, k - T), radius=0.25, material=(RT_LAMBERTIAN, RT_METAL, RT_DIELECTRIC)[n % 3],
                                    albedo=D3(0.3 + 0.1 * i, 0.3 + 0.1 * j, 0.3 + 0.1 * k), fuzz=0.1 * (n % 4),
                                    refraction_index=1.5))
    scene = rtzig.Scene.init(0x1A77 + T)
    scene.world = (RtSphere * len(sph))(*sph)
    return scene


def skim_camera(T, dv_y, spp=8, bounce_max=4):
    """A 64 x 4 camera on lattice(T) whose every primary ray skims: it sits 0.3 f32 ulps under the plane
    of the top poles of layer 1 (its f32 origin rounds onto the plane: what is left of the slab on that
    axis is the rounding of o * inv), before row (., 1, 1), and looks along +x.  du spreads the 64 columns over
    two thirds of the width of the cap that lies above that height; dv = (0, dv_y, 0), so the rows differ
    in a tilt of that size alone (d_y = dv_y (j + U(-0.5, 0.5)): both signs in row 0; 0 exactly for
    dv_y = 0).  The fields are set directly: no builder produces a dv of 2^-30."""
    scene = lattice(T)
    plane = 1.25 + T / 2
    delta = 0.3 * float(np.spacing(np.float32(plane)))
    du_z = math.sqrt(2 * 0.25 * delta) / 96  # the pixels are 1 away, the pole 2
    center = (T - 2.0, plane - delta, 1.0 - T)
    cam = RtCamera(image_width=64, image_height=4, samples_per_pixel=spp, bounce_max=bounce_max,
                   pixel_samples_scale=1.0 / spp, center=D3(*center),
                   pixel0=D3(center[0] + 1.0, center[1], center[2] - 31.5 * du_z), du=D3(0, 0, du_z), dv=D3(0, dv_y, 0),
                   defocus_disk_u=D3(0, 0, 0), defocus_disk_v=D3(0, 0, 0), defocus_angle=0.0, t_min=1e-3, t_max=INF,
                   seed=scene.seed)
    return rtzig.Camera(cam, scene)


def golden_params(width=400, aspect=16.0 / 9.0, spp=10, seed=0xDEADBEEF):
    # main.zig:24-31 preset
    return RtCameraParams(image_width=width, samples_per_pixel=spp, bounce_max=50,
                          aspect_ratio=aspect, look_from=D3(13, 2, 3), look_at=D3(0, 0, 0),
                          v_up=D3(0, 1, 0), vfov=20, defocus_angle=0.6, focus_dist=10,
                          t_min=1e-3, t_max=INF, seed=seed)


def with_camera(cam, **fields):
    """The camera with some rt_camera fields replaced (t_max, seed): the world stays as generated."""
    for k, v in fields.items():
        setattr(cam.cam, k, v)
    return cam


# name -> camera factory: every scene the GPU tests hold to the rule; the CPU test checks the input
# condition share_F32(1e-3) <= INPUT_CAP on each.
# More than one sample per pixel: a pixel average differs as soon as one of its samples diverges, so
# the share grows with spp.  On the final scene share_F32(1e-3) is 1.1% (spp 3) and 4.7% (spp 17)
# at depth 50, 0.26% and 1.6% at depth 2: spp 3 runs at depth 2, spp 17 at depth 1, and chapter 13
# (0.30% at spp 17) carries spp 17 at depth 50.
SCENES = {
    "final_d1": lambda: final(1),
    "final_d2": lambda: final(2),
    "final_d50": lambda: final(50),
    "chapter13": chapter13,
    "chapter9": chapter9,
    "materials": materials,
    "ground_99.9": lambda: ground(99.9),
    "ground_100.1": lambda: ground(100.1),
    "c1_straddle": c1_straddle,
    "large_2600": large,
    "final_w64_spp3_d2": lambda: final(2, width=64, spp=3),
    "final_w64_spp17_d1": lambda: final(1, width=64, spp=17),
    "chapter13_w64_spp17": lambda: chapter13(width=64, spp=17),
    # a finite interval: the f32 cast of t_max starts `closest`; about half the hits of the final scene
    # lie beyond t = 1.2, and chapter 13's ground and far spheres beyond 1.1
    "final_d2_tmax1.2": lambda: with_camera(final(2), t_max=1.2),
    "chapter13_tmax1.1": lambda: with_camera(chapter13(), t_max=1.1),
    "final_d2_seed63": lambda: with_camera(final(2), seed=1 << 63),  # a seed above 32 bits
}


def shares(x, ref):
    """Share of pixels whose max-channel |x - ref| exceeds each theta of THETAS."""
    d = np.abs(np.asarray(x) - ref).max(axis=-1).ravel()
    return [float((d > th).mean()) for th in THETAS]


def reference_pair(oracle, cam, threads=8):
    """(F64 image, F64 rays, F32 image, F32 rays) of oracle mode F for a camera and its scene."""
    f64, r64 = oracle.render_f(cam.cam, cam.scene.world, 64, threads=threads)
    f32, r32 = oracle.render_f(cam.cam, cam.scene.world, 32, threads=threads)
    return f64, r64, f32, r32


def check_against_pair(gpu, rays_gpu, pair, label=""):
    """The one rule: divergence, cap, paired bias, rays and finiteness of a fast-mode
    render against the F64 / F32 reference pair.  Prints every figure before it asserts."""
    f64, r64, f32, r32 = pair
    assert gpu.shape == f64.shape
    finite = bool(np.isfinite(gpu).all())
    sg, sf = shares(gpu, f64), shares(f32, f64)
    dg = (gpu - f64).reshape(-1, 3)
    df = (f32 - f64).reshape(-1, 3)
    n = dg.shape[0]
    mean_g, mean_f = dg.mean(axis=0), df.mean(axis=0)
    se = dg.std(axis=0, ddof=1) / np.sqrt(n)
    print(f"FASTORACLE {label} n={n} share_gpu={sg} share_f32={sf} mean_gpu={mean_g.tolist()} "
          f"mean_f32={mean_f.tolist()} se={se.tolist()} rays_gpu={rays_gpu} rays_f64={r64} rays_f32={r32} "
          f"finite={finite}")
    assert finite, "non-finite output"
    assert sf[0] <= INPUT_CAP, f"input condition: share_F32(1e-3) = {sf[0]}"
    for th, g, f in zip(THETAS, sg, sf):
        assert g <= 2 * f + 0.001, f"divergence at theta={th}: gpu {g} vs F32 {f}"
    assert sg[0] <= GPU_CAP, f"cap: share_gpu(1e-3) = {sg[0]}"
    for c in range(3):
        assert abs(mean_g[c]) <= 2 * abs(mean_f[c]) + 4 * se[c], \
            f"paired bias, channel {c}: gpu {mean_g[c]} vs F32 {mean_f[c]}, se {se[c]}"
    assert abs(rays_gpu - r64) <= 2 * abs(r32 - r64) + 0.002 * r64, \
        f"rays: gpu {rays_gpu}, F64 {r64}, F32 {r32}"
    return sg, sf

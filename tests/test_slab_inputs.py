"""The skimming rays of tests/slab_support.py reach what they are for (CPU): every one may use the tree,
nearly every one hits, and — the control — the numpy model of the walk's f32 slab test loses a share of
those hits on boxes without the builder's pad and none on boxes with it.  The shares are input
conditions measured on the model, not on the kernel: tests/test_gpu_slab.py runs the same rays on the
device, tests/test_slab_certificate_host.py the C++ model on the builder's own trees."""
import numpy as np
import pytest

import fast_scenes
import rtzig
import slab_support as ss

CASES = ["lattice_0", "lattice_64", "lattice_1024", "final"]
# share of the true hits the model drops on the hit sphere's own unpadded box, per rcp_ulps -1, 0, +1,
# as measured (the assertion asks for half)
MEASURED = {
    "lattice_0": (0.0876, 0.0850, 0.0874),
    "lattice_64": (0.1409, 0.1436, 0.1460),
    "lattice_1024": (0.1411, 0.1418, 0.1416),
    "final": (0.0252, 0.0245, 0.0260),}
# likewise for the primary rays of fast_scenes.skim_camera(T, dv_y), by (T, dv_y != 0): lost at any of the three.
# With d_y = 0 every ray has the same o_y and the same clamped reciprocal, so one rounding of o * 1e30 decides
# for all of them: at T = 0 it falls on the safe side (0 lost), at T = 64 on the other (all lost)
CAMERA_MEASURED = {(0, True): 0.833, (0, False): 0.0, (64, True): 0.750, (64, False): 1.0}
_CACHE = {}


def world_of(name):
    if name == "final":
        return rtzig.final_scene_camera(width=48, aspect_ratio=16 / 9, spp=2).scene.world
    return fast_scenes.lattice(int(name.split("_")[1])).world


def case(oracle, name):
    if name not in _CACHE:
        world = world_of(name)
        O, D = ss.case_rays(name, world)
        _CACHE[name] = (world, O, D, ss.ref_hits(oracle, world, O, D))
    return _CACHE[name]


@pytest.mark.parametrize("name", CASES)
def test_every_ray_may_use_the_tree(oracle, name):
    world, O, D, _ = case(oracle, name)
    bound = ss.bound_needed(world, O)
    assert ss.tree_ok(O, D, 1e-3, bound).all()
    # and the variants are there: zero, f32-denormal and f32-underflowing tilts
    small = np.sort(np.abs(D), axis=1)[:, 0]
    with np.errstate(under="ignore"):
        s32 = small.astype(np.float32)
    assert (small == 0).sum() == ss.N // 16
    assert ((s32 > 0) & (s32 < np.finfo(np.float32).tiny)).sum() == ss.N // 16
    assert ((small > 0) & (s32 == 0)).sum() == ss.N // 16


@pytest.mark.parametrize("name", CASES)
def test_nearly_every_ray_hits_within_ulps_of_a_face(oracle, name):
    world, O, D, ref = case(oracle, name)
    hit = ref["index"] >= 0
    print("SLABINPUT %s hit share %.4f, %d distinct spheres" % (name, hit.mean(), len(set(ref["index"][hit].tolist()))))
    assert hit.mean() >= 0.95
    assert len(set(ref["index"][hit].tolist())) >= min(60, len(world) // 2)
    # the hit point lies within 16 f32 ulps of a face of the hit sphere's tight box
    c, r = ss.centres_radii(world)
    k = ref["index"][hit]
    p = ref["point"][hit]
    gap = np.minimum(np.abs(p - (c[k] - r[k, None])), np.abs(p - (c[k] + r[k, None])))
    scale = ss.ulp32(np.abs(c[k]) + r[k, None])
    assert np.median((gap / scale).min(axis=1)) <= 16


@pytest.mark.parametrize("T", [0, 64])
@pytest.mark.parametrize("dv_y", [2.0 ** -30, 0.0])
def test_skim_camera_primary_rays_hit_under_the_pole_plane(oracle, T, dv_y):
    """The path-loop case's camera (fast_scenes.skim_camera): every pixel's rays, at the ends and the middle of
    the jitter range, hit the first sphere of the row within its cap, tilted by at most 2^-28."""
    cam = fast_scenes.skim_camera(T, dv_y)
    c, world = cam.cam, cam.scene.world
    total, D, ts = 0, [], []
    for j in range(c.image_height):
        for i in range(c.image_width):
            for off in (-0.5, 0.0, 0.499):
                d = [(c.pixel0[k] + c.du[k] * (i + off)) + c.dv[k] * (j + off) - c.center[k] for k in range(3)]
                assert d[0] == 1.0 and abs(d[1]) <= 2.0 ** -28 and (dv_y != 0 or d[1] == 0.0)
                k, t = oracle.world_hit(world, list(c.center), d, c.t_min, c.t_max)
                total += 1
                if k >= 0:
                    assert k == 1 * 4 + 1 and 1.9 < t < 2.0  # sphere (0, 1, 1), just before its pole
                    D.append(d)
                    ts.append(t)
    assert len(D) >= 0.95 * total
    _, rays = oracle.render_b(c, world, threads=4)
    assert rays > 1.5 * c.image_width * c.image_height * c.samples_per_pixel  # the paths go on
    # the control: without the pad the model loses these hits too (CAMERA_MEASURED), with it none
    O, D, ts = np.tile(np.array(list(c.center)), (len(D), 1)), np.array(D), np.array(ts)
    lost = np.zeros(len(D), bool)
    for ulps in (-1, 0, 1):
        lo, hi = ss.tight_boxes(world, 0.0)
        lost |= ~ss.slab_keeps(O, D, lo[5], hi[5], c.t_min, ts, rcp_ulps=ulps)
        lo, hi = ss.tight_boxes(world, 1.0, ss.extent(world))
        assert ss.slab_keeps(O, D, lo[5], hi[5], c.t_min, ts, rcp_ulps=ulps).all()
    print("SLABINPUT camera T=%d dv_y=%g: unpadded, the model loses %.3f of the primary hits" % (T, dv_y, lost.mean()))
    assert lost.mean() >= CAMERA_MEASURED[T, dv_y != 0] / 2


@pytest.mark.parametrize("name", CASES)
def test_control_unpadded_boxes_lose_hits_and_padded_ones_none(oracle, name):
    world, O, D, ref = case(oracle, name)
    hit = ref["index"] >= 0
    k = ref["index"][hit]
    shares = []
    for ulps in (-1, 0, 1):
        lo, hi = ss.tight_boxes(world, 0.0)
        kept = ss.slab_keeps(O[hit], D[hit], lo[k], hi[k], 1e-3, ref["t"][hit], rcp_ulps=ulps)
        shares.append(float((~kept).mean()))
        lo, hi = ss.tight_boxes(world, 1.0, ss.bound_needed(world, O))
        assert ss.slab_keeps(O[hit], D[hit], lo[k], hi[k], 1e-3, ref["t"][hit], rcp_ulps=ulps).all()
    print("SLABINPUT %s unpadded drop shares %s" % (name, ["%.4f" % s for s in shares]))
    for got, measured in zip(shares, MEASURED[name]):
        assert measured > 0 and got >= measured / 2

"""Radiance queries on the GPU (include/rt.h rt_radiance_rays): Camera.rayColor of
caller-supplied rays, bit for bit.

Two references.  The renderer identity: fed getRay's rays and the streams' states after getRay's draws,
the call must return the renderer's own image at one sample per pixel — oracle.render_b's, and
rt_render_rows_async's on the same context.  The model: tests/radiance_support.py's ray_color, which
tests/test_radiance_model.py holds to the C oracle, for everything a camera never produces.

Comparisons are gpu_support.same_bits; where the reference holds NaN (radiance_support.same_or_nan) a
NaN component must be NaN on the device and every other bit must match.  The shares asserted on a
reference are input conditions — they say that a case exercises what it is meant to — not tolerances."""
import math

import numpy as np
import pytest
import torch

import fast_scenes
import rtzig
from gpu_support import DEV, cached, same_bits
from gpu_support import module_renderers, renderers  # noqa: F401 (fixtures)
from radiance_support import Params, camera_rays, radiance_ref, same_or_nan
from rtzig.abi import RT_DIELECTRIC, RT_METAL
from rtzig.lib import RtError
from slab_support import tree_ok

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
PAD, SENTINEL = 8, -54321.0  # rows before and after d_sum, and what they hold


# ---- one call ------------------------------------------------------------------------------------------
def radiance(r, O, D, n=None, stride=3, states=None, keep=None, **kw):
    """One rt_radiance_rays call on the default stream: (sums (n, 3), [paths, segments, scanned]).  d_sum
    lies inside a larger buffer of sentinels and starts as NaN (never read when sample_begin == 0) or as
    `keep`; the rows around it and the inputs must come back untouched."""
    n = len(O) if n is None else n
    o = np.zeros((len(O), stride or 3))  # stride 0 means 3
    d = np.zeros((len(O), stride or 3))
    o[:, :3], d[:, :3] = O, D
    if stride > 3:
        o[:, 3:], d[:, 3:] = NAN, NAN  # the padding lane of a Zig @Vector(3, f64) is never read
    d_o, d_d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    d_st = torch.from_numpy(np.array(states, np.uint64).view(np.int64)).to(DEV) if states is not None else None
    buf = torch.full((len(O) + 2 * PAD, 3), SENTINEL, dtype=torch.float64, device=DEV)
    buf[PAD:PAD + n] = NAN if keep is None else torch.from_numpy(np.ascontiguousarray(keep)).to(DEV)
    stats = torch.zeros(3, dtype=torch.int64, device=DEV)
    r.radiance_rays(d_o.data_ptr(), d_d.data_ptr(), n, buf[PAD:].data_ptr(), d_stats_ptr=stats.data_ptr(),
                    d_states_ptr=d_st.data_ptr() if d_st is not None else None, ray_stride=stride, **kw)
    torch.cuda.synchronize()
    r.sync()  # reports a failure the kernel recorded
    host = buf.cpu().numpy()
    assert (host[:PAD] == SENTINEL).all() and (host[PAD + n:] == SENTINEL).all(), "d_sum written outside its n rows"
    assert same_bits(d_o.cpu().numpy(), o) and same_bits(d_d.cpu().numpy(), d), "the inputs were modified"
    if states is not None:
        assert np.array_equal(d_st.cpu().numpy().view(np.uint64), states), "the states were modified"
    return host[PAD:PAD + n].copy(), stats.cpu().numpy().tolist()


def render_1spp(r, cam):
    """rt_render_rows_async of the whole image on the context: ((H * W, 3) image, rays)."""
    img = torch.empty((cam.image_height * cam.image_width, 3), dtype=torch.float64, device=DEV)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    r.render_rows_async(cam, img.data_ptr(), d_stats_ptr=stats.data_ptr())
    torch.cuda.synchronize()
    r.sync()
    return img.cpu().numpy(), int(stats[0])


# ---- cameras, their rays and the renderer's own image ------------------------------------------------
def final_cam():
    """The final scene at 64 x 40, one sample per pixel: the tree in LDS, defocus 0.6."""
    return cached("rad_final", lambda: rtzig.final_scene_camera(width=64, aspect_ratio=1.6, spp=1))


CAMS = {
    "final": final_cam,
    "final_pinhole": lambda: cached("rad_pinhole", lambda: fast_scenes.with_camera(
        rtzig.final_scene_camera(width=64, aspect_ratio=1.6, spp=1), defocus_angle=0.0)),
    "chapter13": lambda: cached("rad_ch13", lambda: rtzig.chapter13_camera(width=48, spp=1)),  # the list walk, defocus 10
}


def identity_ref(oracle, name):
    """(origins, directions, states after getRay, oracle B's (P, 3) image at 1 spp, its rays): read-only."""
    def make():
        cam = CAMS[name]()
        O, D, S = camera_rays(oracle, cam.cam)
        img, rays = oracle.render_b(cam.cam, cam.scene.world, threads=8)
        out = (O, D, S, img.reshape(-1, 3), rays)
        for a in out[:4]:
            a.setflags(write=False)
        return out
    return cached(("rad_identity", name), make)


def params_of(cam):
    return dict(bounce_max=cam.bounce_max, t_min=cam.t_min, t_max=cam.t_max)


@pytest.fixture(scope="module")
def final_renderer(module_renderers):
    return module_renderers(final_cam().scene.world)


# ---- 1. the renderer identity --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CAMS))
def test_get_rays_and_states_return_the_renderers_image(oracle, name, renderers):
    cam = CAMS[name]()
    O, D, S, img, rays = identity_ref(oracle, name)
    P = len(O)
    assert (cam.cam.defocus_angle > 0) == (name != "final_pinhole") and 1200 < P <= 2560
    assert len({tuple(o) for o in O.tolist()}) == (P if name != "final_pinhole" else 1)  # defocus: every origin its own
    r = renderers(cam.scene.world)
    bvh = r.tree_info()["bvh"]
    assert bvh == (0 if name == "chapter13" else 1)
    got, stats = radiance(r, O, D, states=S, **params_of(cam.cam))
    assert r.kernel_name() == ("bvh_lds(radiance)" if bvh else "lds_u4(radiance)")
    assert same_bits(got, img), "%d of %d pixels differ from oracle B" % (int((got != img).any(axis=1).sum()), P)
    assert stats[:2] == [P, rays] and stats[2] == (0 if bvh else rays)
    own, own_rays = render_1spp(r, cam.cam)
    assert same_bits(own, img) and own_rays == rays
    assert same_bits(got, own)
    r.close()


# ---- 2. keyed streams against the model ----------------------------------------------------------------
SEED = 0x5EED0FCA11E75


def mixed_batch(oracle):
    """(origins, directions, kinds): every kind of ray a camera does not produce next to camera rays,
    interleaved lane by lane (a fixed permutation)."""
    world = final_cam().scene.world
    O0, D0, _, _, _ = identity_ref(oracle, "final")
    g = np.random.default_rng(14)
    big = [k for k, s in enumerate(world) if s.radius == 1.0]
    glass = [k for k in big if world[k].material == RT_DIELECTRIC]
    metal = [k for k in big if world[k].material == RT_METAL]
    assert len(glass) == 1 and len(metal) == 1, "the final scene's two big spheres"
    parts = {}
    pick = lambda n: g.choice(len(O0), n, replace=False)
    k = pick(160)
    parts["camera"] = (O0[k], D0[k])
    for name, idx in (("in_glass", glass[0]), ("in_metal", metal[0])):
        c = np.array(list(world[idx].center))
        parts[name] = (c + g.uniform(-0.5, 0.5, (48, 3)), g.standard_normal((48, 3)))
    # grazing the ground sphere (centre (0, -1000, 0), radius 1000): nearly horizontal, a hair above it
    o = np.stack([g.uniform(-8, 8, 48), 2.0 ** g.uniform(-30, -8, 48), g.uniform(-8, 8, 48)], axis=1)
    dg = np.stack([g.standard_normal(48), -2.0 ** g.uniform(-30, -6, 48), g.standard_normal(48)], axis=1)
    parts["grazing"] = (o, dg)
    k = pick(48)
    parts["dir_2^30"] = (O0[k], D0[k] * 2.0 ** 30)
    k = pick(48)
    parts["dir_2^-30"] = (O0[k], D0[k] * 2.0 ** -30)
    far = g.uniform([-12, .05, -12], [12, 3, 12], (48, 3)) * 400
    far[:, 0] = g.choice([-1.0, 1.0], 48) * g.uniform(2100, 4800, 48)  # beyond the tree's origin bound (2000)
    parts["far"] = (far, -far + g.standard_normal((48, 3)))
    k = pick(32)
    o, d = O0[k].copy(), D0[k].copy()
    bad = [NAN, INF, -INF]
    for q in range(32):
        (o if q & 1 else d)[q, q % 3] = bad[(q // 2) % 3]
    parts["non_finite"] = (o, d)
    k = pick(8)
    parts["zero_dir"] = (O0[k], np.zeros((8, 3)))
    kinds = np.concatenate([[name] * len(v[0]) for name, v in parts.items()])
    O = np.concatenate([v[0] for v in parts.values()])
    D = np.concatenate([v[1] for v in parts.values()])
    perm = np.random.default_rng(15).permutation(len(O))
    return np.ascontiguousarray(O[perm]), np.ascontiguousarray(D[perm]), kinds[perm]


def batch(oracle):
    return cached("rad_mixed", lambda: mixed_batch(oracle))


def model(oracle, key, O, D, bound, world=None, **kw):
    """radiance_ref on the final scene (or `world`) with the scanned segments counted by the tree's domain
    rule at origin bound `bound`: (sums, [paths, segments, scanned]), computed once per key."""
    def make():
        prm = Params(kw.pop("bounce_max", 50), kw.pop("t_min", 1e-3), kw.pop("t_max", INF))
        scanned = [0]

        def on_segment(o, d):
            scanned[0] += int(bound == 0 or not tree_ok([o], [d], prm.t_min, bound)[0])
        w = final_cam().scene.world if world is None else world
        sums, segs = radiance_ref(oracle, w, O, D, prm, kw.pop("seed", SEED), on_segment=on_segment, **kw)
        sums.setflags(write=False)
        n = len(O) * kw.get("sample_count", 1)
        return sums, [n, segs, scanned[0]]
    return cached(("rad_model", key, bound), make)


@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("bounce_max", [0, 1, 50])
def test_mixed_batch_keyed_streams_equal_the_model(oracle, final_renderer, samples, bounce_max):
    O, D, kinds = batch(oracle)
    bound = final_renderer.origin_bound()
    assert 2000 <= bound < 2001 and len(O) == 488
    ref, ref_stats = model(oracle, ("mixed", samples, bounce_max), O, D, bound, sample_count=samples, bounce_max=bounce_max)
    got, stats = radiance(final_renderer, O, D, seed=SEED, sample_count=samples, bounce_max=bounce_max)
    assert same_or_nan(got, ref), "%d of %d rays differ" % (
        int((~((got == ref) | (np.isnan(got) & np.isnan(ref)))).any(axis=1).sum()), len(O))
    assert stats == ref_stats
    # input conditions: what each kind is there for
    if bounce_max == 0:
        assert not got.any() and stats == [len(O) * samples, 0, 0]  # black, nothing traced
    if bounce_max == 50 and samples == 1:
        assert np.isnan(ref[kinds == "zero_dir"]).all()                   # unit(0) is NaN: a NaN sky
        assert np.isnan(ref[kinds == "non_finite"]).any(axis=1).sum() >= 8
        assert np.isfinite(ref[np.isin(kinds, ["camera", "in_glass", "in_metal", "grazing", "dir_2^30", "dir_2^-30", "far"])]).all()
        # the first segment of a scaled or far ray is scanned, later ones walk the tree
        n_first = int(np.isin(kinds, ["dir_2^30", "dir_2^-30", "far", "non_finite", "zero_dir"]).sum())
        assert n_first == 184 <= stats[2] < stats[1] / 3


@pytest.mark.parametrize("name, t_min, t_max, all_scanned", [
    ("tmin0", 0.0, INF, False), ("tmin_neg", -1e-3, INF, True), ("tmax_nan", 1e-3, NAN, False), ("empty", 5.0, 1.0, False),
    ("tmax2", 1e-3, 2.0, False)])
def test_intervals_zero_negative_nan_and_empty(oracle, final_renderer, name, t_min, t_max, all_scanned):
    O, D, kinds = batch(oracle)
    O, D = O[:192], D[:192]
    bound = final_renderer.origin_bound()
    ref, ref_stats = model(oracle, ("interval", name), O, D, bound, t_min=t_min, t_max=t_max)
    got, stats = radiance(final_renderer, O, D, seed=SEED, t_min=t_min, t_max=t_max)
    assert same_or_nan(got, ref) and stats == ref_stats
    if all_scanned:
        assert stats[2] == stats[1] > 192  # a negative t_min: nothing certifies the tree, every segment scanned
    if name in ("tmax_nan", "empty"):
        assert stats[1] == 192  # nothing can be hit: one segment, the sky


# ---- 3. shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_small_batches_at_the_default_grid(oracle, final_renderer, n):
    O, D, S, img, _ = identity_ref(oracle, "final")
    got, stats = radiance(final_renderer, O[:256], D[:256], n=n, states=S[:256], **params_of(final_cam().cam))
    assert same_bits(got, img[:n]) and stats[0] == n and stats[2] == 0


def test_one_block_refills_across_tiles_and_equals_the_default_grid(oracle, final_renderer, monkeypatch):
    """2,049 rays: 33 tiles.  One block's 16 waves hold two or three tiles each and refill their free
    lanes from them in every iteration; the default grid gives a wave one tile.  The hook changes no bit."""
    O, D, S, img, _ = identity_ref(oracle, "final")
    n = 2049
    prm = params_of(final_cam().cam)
    wide, wide_stats = radiance(final_renderer, O[:n], D[:n], states=S[:n], **prm)
    monkeypatch.setenv("RTZIG_RADIANCE_BLOCKS", "1")
    one, one_stats = radiance(final_renderer, O[:n], D[:n], states=S[:n], **prm)
    assert same_bits(one, wide) and one_stats == wide_stats
    assert same_bits(one, img[:n])
    # keyed streams, several samples: a lane keeps its ray while other lanes refill
    keyed1, s1 = radiance(final_renderer, O[:n], D[:n], seed=SEED, sample_count=3, bounce_max=50)
    monkeypatch.delenv("RTZIG_RADIANCE_BLOCKS")
    keyed, s0 = radiance(final_renderer, O[:n], D[:n], seed=SEED, sample_count=3, bounce_max=50)
    assert same_bits(keyed1, keyed) and s1 == s0 and s0[0] == 3 * n


# ---- 4. splits -----------------------------------------------------------------------------------------
def test_sample_splits_batch_splits_and_strides_leave_the_same_bits(oracle, final_renderer):
    O, D, _ = batch(oracle)
    n = len(O)
    r = final_renderer
    whole, stats = radiance(r, O, D, seed=SEED, sample_count=5, ray_base=1000)
    assert stats[0] == 5 * n
    # samples [0, 5) = [0, 2) + [2, 5): the second call continues from the stored sums
    first, s1 = radiance(r, O, D, seed=SEED, sample_count=2, ray_base=1000)
    both, s2 = radiance(r, O, D, seed=SEED, sample_begin=2, sample_count=3, ray_base=1000, keep=first)
    assert same_or_nan(both, whole) and [a + b for a, b in zip(s1, s2)] == stats
    assert not same_or_nan(first, whole)
    # one batch = two sub-batches with ray_base advanced (a cut inside a tile)
    cut = 203
    a, sa = radiance(r, O[:cut], D[:cut], seed=SEED, sample_count=5, ray_base=1000)
    b, sb = radiance(r, O[cut:], D[cut:], seed=SEED, sample_count=5, ray_base=1000 + cut)
    assert same_or_nan(np.concatenate([a, b]), whole) and [x + y for x, y in zip(sa, sb)] == stats
    # ... and the base matters: the same rays on other streams
    other, _ = radiance(r, O[cut:], D[cut:], seed=SEED, sample_count=5, ray_base=0)
    assert not same_or_nan(other, b)
    # stride 4 (Zig's @Vector(3, f64)) and 0 (means 3)
    for stride in (4, 0):
        got, st = radiance(r, O, D, seed=SEED, sample_count=5, ray_base=1000, stride=stride)
        assert same_or_nan(got, whole) and st == stats


# ---- 5. structures and contexts ------------------------------------------------------------------------
def test_large_scene_global_memory_tree(oracle, renderers):
    cam = cached("large", fast_scenes.large)
    g = np.random.default_rng(1)
    O = g.uniform([-12, .05, -12], [12, 3, 12], (512, 3)) * 2.5
    D = g.standard_normal((512, 3))
    r = renderers(cam.scene.world)
    assert r.tree_info()["bvh"] == 1
    ref, ref_stats = model(oracle, "large", O, D, r.origin_bound(), world=cam.scene.world, bounce_max=8, sample_count=2)
    got, stats = radiance(r, O, D, seed=SEED, bounce_max=8, sample_count=2)
    assert r.kernel_name() == "bvh_global(radiance)"
    assert same_bits(got, ref) and stats == ref_stats
    assert stats[2] == 0 and stats[1] > 1.5 * 1024  # bounces, all on the tree
    r.close()


def test_trained_tree_gives_the_same_bits(oracle, monkeypatch, renderers):
    O, D, _ = batch(oracle)
    cam = final_cam()
    monkeypatch.setenv("RTZIG_BVH_TRAIN", "1")
    r = renderers(cam.scene.world)
    train = rtzig.final_scene_camera(width=48, aspect_ratio=16 / 9, spp=2)
    img = torch.empty((train.height, train.width, 3), dtype=torch.float64, device=DEV)
    r.render_rows_async(train.cam, img.data_ptr())
    torch.cuda.synchronize()
    assert r.tree_info()["trained"] == 1
    ref, ref_stats = model(oracle, ("mixed", 1, 50), O, D, r.origin_bound(), sample_count=1, bounce_max=50)
    got, stats = radiance(r, O, D, seed=SEED)
    assert r.tree_info()["trained"] == 1  # walked as it is
    assert same_or_nan(got, ref) and stats == ref_stats
    r.close()


def test_reserved_origin_bound_same_bits_fewer_scanned(oracle, renderers):
    O, D, kinds = batch(oracle)
    r = renderers(final_cam().scene.world)
    ref, ref_stats = model(oracle, ("mixed", 1, 50), O, D, r.origin_bound(), sample_count=1, bounce_max=50)
    r.reserve_origin_bound(6000)
    assert 6000 <= r.origin_bound() < 6100
    got, stats = radiance(r, O, D, seed=SEED)
    assert same_or_nan(got, ref) and stats[:2] == ref_stats[:2]
    assert stats[2] == ref_stats[2] - int((kinds == "far").sum())  # the far origins' first segments are on the tree now
    r.close()


@pytest.mark.parametrize("kind", ["instrumented", "f32"])
def test_instrumented_and_f32_contexts_give_the_same_bits(oracle, kind, renderers):
    O, D, _ = batch(oracle)
    r = renderers(final_cam().scene.world, "f32" if kind == "f32" else "f64", profile=kind == "instrumented")
    ref, ref_stats = model(oracle, ("mixed", 1, 50), O, D, r.origin_bound(), sample_count=1, bounce_max=50)
    got, stats = radiance(r, O, D, seed=SEED)
    assert r.kernel_name() == "bvh_lds(radiance)"
    assert same_or_nan(got, ref) and stats == ref_stats
    r.close()


def test_non_default_stream_needs_no_host_sync(oracle, final_renderer):
    O, D, S, img, _ = identity_ref(oracle, "final")
    h_o, h_d = torch.from_numpy(O.copy()).pin_memory(), torch.from_numpy(D.copy()).pin_memory()
    h_s = torch.from_numpy(S.view(np.int64).copy()).pin_memory()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        # the inputs and the NaN fill are produced on the stream; the sums are consumed on it
        d_o = h_o.to(DEV, non_blocking=True) * 1.0
        d_d = h_d.to(DEV, non_blocking=True) + 0.0
        d_s = h_s.to(DEV, non_blocking=True) + 0
        sums = torch.full((len(O), 3), NAN, dtype=torch.float64, device=DEV)
        final_renderer.radiance_rays(d_o.data_ptr(), d_d.data_ptr(), len(O), sums.data_ptr(), d_states_ptr=d_s.data_ptr(),
                                     stream_ptr=s.cuda_stream, **params_of(final_cam().cam))
        twice = sums * 2
        got, got2 = sums.to("cpu", non_blocking=True), twice.to("cpu", non_blocking=True)
    s.synchronize()
    assert same_bits(got.numpy(), img) and same_bits(got2.numpy(), img * 2)


def test_kernel_times_and_empty_calls(oracle, renderers):
    O, D, S, img, _ = identity_ref(oracle, "final")
    r = renderers(final_cam().scene.world, timing=True)
    radiance(r, O[:256], D[:256], states=S[:256], **params_of(final_cam().cam))
    sample_ms, reduce_ms = r.kernel_times()
    assert sample_ms > 0 and reduce_ms == 0
    name = r.kernel_name()
    assert name.endswith("(radiance)")
    # n_rays == 0, sample_count == 0 and "nothing asked for" return RT_OK and launch nothing
    sums = torch.full((4, 3), SENTINEL, dtype=torch.float64, device=DEV)
    stats = torch.zeros(3, dtype=torch.int64, device=DEV)
    r.render_rows_async(final_cam().cam, torch.empty((2560, 3), dtype=torch.float64, device=DEV).data_ptr())
    other = r.kernel_name()
    assert other != name
    r.radiance_rays(1, 1, 0, sums.data_ptr(), d_stats_ptr=stats.data_ptr())  # the ray pointers are never read
    r.radiance_rays(1, 1, 4, sums.data_ptr(), d_stats_ptr=stats.data_ptr(), sample_count=0)
    r.radiance_rays(1, 1, 4)
    torch.cuda.synchronize()
    assert (sums.cpu().numpy() == SENTINEL).all() and not stats.cpu().numpy().any()
    assert r.kernel_name() == other
    # d_stats alone still launches
    d_o, d_d = torch.from_numpy(O[:4].copy()).to(DEV), torch.from_numpy(D[:4].copy()).to(DEV)
    r.radiance_rays(d_o.data_ptr(), d_d.data_ptr(), 4, d_stats_ptr=stats.data_ptr(), seed=SEED)
    torch.cuda.synchronize()
    assert stats[0] == 4 and stats[1] >= 4 and r.kernel_name() == name
    r.close()
    r = renderers()
    with pytest.raises(RtError, match="no scene"):
        r.radiance_rays(1, 1, 4, d_sum_ptr=1)
    r.close()


# ---- 6. Python -----------------------------------------------------------------------------------------
def test_python_wrappers_and_resolve(oracle, final_renderer):
    O, D, _ = batch(oracle)
    keep = np.isfinite(O).all(axis=1) & np.isfinite(D).all(axis=1) & D.any(axis=1)
    O, D = np.ascontiguousarray(O[keep][:300]), np.ascontiguousarray(D[keep][:300])
    scene = final_cam().scene
    dev, _ = radiance(final_renderer, O, D, seed=scene.seed, sample_count=4, ray_base=7)
    assert np.isfinite(dev).all()
    assert same_bits(rtzig.radiance(scene.world, O, D, samples=4, seed=scene.seed, ray_base=7), dev)
    assert same_bits(scene.radiance(O, D, samples=4, ray_base=7), dev)
    assert not same_bits(rtzig.radiance(scene.world, O, D, samples=4, seed=scene.seed + 1, ray_base=7), dev)
    assert rtzig.radiance(scene.world, np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 3)
    # states through the wrapper: the renderer identity again
    Oc, Dc, S, img, _ = identity_ref(oracle, "final")
    assert same_bits(scene.radiance(Oc[:500], Dc[:500], states=S[:500]), img[:500])
    # rt_accum_resolve on d_sum: sum * (1.0 / n), and the packed bytes
    d_sum = torch.from_numpy(dev).to(DEV)
    out = torch.empty((300, 3), dtype=torch.float64, device=DEV)
    final_renderer.resolve(d_sum.data_ptr(), 300, 4, out.data_ptr())
    rgb = torch.empty((300, 3), dtype=torch.uint8, device=DEV)
    final_renderer.resolve(d_sum.data_ptr(), 300, 4, rgb.data_ptr(), output="rgb8")
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), dev * (1.0 / 4))
    assert np.array_equal(rgb.cpu().numpy(), oracle.to_rgb8(dev * (1.0 / 4)))

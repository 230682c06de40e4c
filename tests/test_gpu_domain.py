"""The value and size ranges include/rt.h allows but the scene-shaped tests never reach: a finite or
empty hit interval (t_max), seeds above 32 bits, sample numbers with bit 31 set up to the last one
the ABI admits, a selection longer than one round of its one-block scan, and the resolve kernels on
accumulator values no render produces.

Every comparison is of bits (np.array_equal, or int64 views), and ray counts are equal.  The
references never come from the code under test: oracle B (oracle_render_b / oracle_accumulate_b), the
per-sample Python reference of tests/gpu_support.py, numpy, oracle.to_rgb8, or a count identity
(a ray per sample when nothing can be hit)."""
import math

import numpy as np
import pytest
import torch

import domain_values as dv
import fast_scenes
import rtzig
from fast_scenes import always_list_scene, far_origin_scene
from gpu_support import (DEV, FLOOR, MAX_C, MIN_C, SEL_BLOCK, TOL, Buffers, add_sample, assert_equal, i32, list_a,
                         select_numpy, synthetic)
from gpu_support import module_renderers, renderers  # noqa: F401 (fixtures)
from rtzig.abi import D3, RT_LAMBERTIAN, RtCamera, RtSphere

pytestmark = pytest.mark.gpu

INF = math.inf
MODES = ["ring", "direct"]
# t_min is 1e-3 everywhere here: -1, 0, 1e-3 and -inf leave an empty interval; 1e300 is inf as f32
TMAX = [-1.0, 0.0, 1e-3, 1.2, 2.0, 50.0, 1e300, -INF]
SEEDS = [0, 1 << 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15]
LAST = 2 ** 32 - 1  # sample_begin + sample_count may reach it, and a pixel's count


def with_fields(cam, **fields):
    """A copy of an rt_camera with some fields replaced."""
    c = RtCamera.from_buffer_copy(cam)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def final64():
    return rtzig.final_scene_camera(width=64, aspect_ratio=1.5, spp=4)


def final37():
    return rtzig.final_scene_camera(width=37, aspect_ratio=16 / 9, spp=1)


def materials64():
    scene = fast_scenes.materials().scene
    return (rtzig.Camera.builder(64, 1.5).setScene(scene).setDefocusAngle(2.0).setFocusDist(1.5)
            .setViewport((0, 0.3, 0.5), (0, 0, -1), 70).setSamplesPerPixel(4).build())


def _always():
    return always_list_scene(3, True, 2)[1]


def _far():
    return far_origin_scene(width=64)[1]


SCENES = {"final64": final64, "final37": final37, "materials64": materials64, "large": fast_scenes.large,
          "always": _always, "far": _far, "chapter13": lambda: rtzig.chapter13_camera(width=37, spp=1)}
_CAMS, _REFS = {}, {}


def scene(name):
    if name not in _CAMS:
        _CAMS[name] = SCENES[name]()
    return _CAMS[name]


def ref_b(oracle, name, **fields):
    """Oracle B's (image, rays) of a scene with some camera fields replaced; computed once, read-only."""
    key = (name,) + tuple(sorted(fields.items()))
    if key not in _REFS:
        cam = scene(name)
        img, rays = oracle.render_b(with_fields(cam.cam, **fields), cam.scene.world, threads=16)
        img.setflags(write=False)
        _REFS[key] = (img, rays)
    return _REFS[key]


def sky_only(oracle, name):
    """Oracle B at bounce_max = 1 of a world no ray hits (one small sphere behind the camera), at the
    scene's own camera, seed and sample count: what every sample returns when the interval is empty."""
    key = (name, "sky")
    if key not in _REFS:
        c = with_fields(scene(name).cam, bounce_max=1, t_max=INF)
        W, H = c.image_width, c.image_height
        back = [2 * c.center[k] - (c.pixel0[k] + c.du[k] * (W / 2) + c.dv[k] * (H / 2)) for k in range(3)]
        behind = (RtSphere * 1)(RtSphere(center=D3(*back), radius=0.01, material=RT_LAMBERTIAN, albedo=D3(1, 1, 1)))
        sky, rays = oracle.render_b(c, behind, threads=16)
        assert rays == W * H * c.samples_per_pixel and (sky > 0).all()
        sky.setflags(write=False)
        _REFS[key] = sky
    return _REFS[key]


def render_rows(r, c):
    """One render of camera struct c on renderer r: (image, rays, samples)."""
    out = torch.full((c.image_height, c.image_width, 3), float("nan"), dtype=torch.float64, device=DEV)
    st = torch.zeros(2, dtype=torch.int64, device=DEV)
    r.render_rows_async(c, out.data_ptr(), d_stats_ptr=st.data_ptr())
    r.sync()
    st = st.cpu().tolist()
    return out.cpu().numpy(), st[0], st[1]


def fill(n, width=3, salt=0):
    """A known finite pattern for a pre-filled accumulator: dyadic values in [0.25, 16)."""
    a = ((np.arange(n * width, dtype=np.int64) * 7919 + salt) % 1009) / 64.0 + 0.25
    return a.reshape(n, width) if width > 1 else a


# ---- finite t_max ------------------------------------------------------------------------------------
def check_tmax(oracle, name, r, t_max, where):
    cam = scene(name)
    c = with_fields(cam.cam, t_max=t_max)
    img, rays, samples = render_rows(r, c)
    ref, ref_rays = ref_b(oracle, name, t_max=t_max)
    assert samples == cam.width * cam.height * c.samples_per_pixel, where
    assert np.array_equal(img, ref), (where, int((img != ref).any(-1).sum()))
    assert rays == ref_rays, where
    if t_max <= c.t_min:  # nothing can be hit: one ray per sample, and every sample is the sky
        assert rays == samples, where
        assert np.array_equal(img, sky_only(oracle, name)), where


def test_tmax_changes_the_image_on_the_oracle(oracle):
    """Teeth, on the oracle alone: at t_max = 1.2 the final scene differs from the unbounded render on
    more than a tenth of its pixels (about half), and an empty interval is the sky-only image."""
    full = ref_b(oracle, "final64", t_max=INF)[0]
    assert (ref_b(oracle, "final64", t_max=1.2)[0] != full).any(-1).mean() > 0.10
    assert (ref_b(oracle, "final64", t_max=2.0)[0] != full).any(-1).mean() > 0.10
    for t in (-1.0, 0.0, 1e-3, -INF):
        img, rays = ref_b(oracle, "final64", t_max=t)
        assert np.array_equal(img, sky_only(oracle, "final64")) and rays == 64 * 42 * 4
        assert (img != full).any(-1).mean() > 0.10


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", ["bvh", "smem_u4", "lds_u4"])
def test_tmax_final_scene_every_walk(oracle, variant, mode, monkeypatch, renderers):
    """The BVH walk and both list walks, in both unit modes (separate instantiations): `closest`
    starts from t_max in each."""
    monkeypatch.setenv("RTZIG_KERNEL", variant)
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    r = renderers(scene("final64"))
    for t_max in TMAX:
        check_tmax(oracle, "final64", r, t_max, (variant, mode, t_max))
        name = r.kernel_name()
        assert name.startswith("bvh_" if variant == "bvh" else variant), name
        if variant == "bvh":  # the list walks' names do not carry the unit mode
            assert ("direct" in name) == (mode == "direct"), name
    r.close()


def test_tmax_trained_tree(oracle, monkeypatch, renderers):
    monkeypatch.setenv("RTZIG_BVH_TRAIN", "1")
    r = renderers(scene("final64"))
    for t_max in TMAX:
        check_tmax(oracle, "final64", r, t_max, ("trained", t_max))
        assert r.tree_info()["trained"] == 1
    r.close()


@pytest.mark.parametrize("name", ["large", "always", "far", "materials64"])
def test_tmax_other_structures(oracle, name, monkeypatch, renderers):
    """The global-memory tree (2600 spheres), the always-list's runtime loop (more than four entries),
    the far-origin walk without culling (RTZIG_BVH_ORIGIN_SCALE shrinks the bound so that ordinary
    rays take it) and the materials scene (7 spheres: the list walk from LDS)."""
    if name in ("always", "far"):
        monkeypatch.setenv("RTZIG_KERNEL", "bvh")
    if name == "far":
        monkeypatch.setenv("RTZIG_BVH_ORIGIN_SCALE", "0.05")
    r = renderers(scene(name))
    info = r.tree_info()
    for t_max in TMAX:
        check_tmax(oracle, name, r, t_max, (name, t_max))
    kernel = r.kernel_name()
    r.close()
    if name == "large":
        assert kernel.startswith("bvh_global"), kernel
    elif name == "always":
        assert kernel.startswith("bvh_") and info["always"] > 4, (kernel, info)
    elif name == "far":
        assert kernel.startswith("bvh_") and info["always"] >= 1, (kernel, info)
    else:
        assert kernel.startswith("lds_u4"), kernel


def feature_sums(oracle, c, spheres, begin, count, start=None):
    """The per-sample Python reference of tests/gpu_support.py over samples [begin, begin + count),
    added onto `start` (four arrays; None: zeros)."""
    P = c.image_width * c.image_height
    if start is None:
        start = (np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P), np.zeros(P, np.uint32))
    sums = tuple(a.copy() for a in start)
    for s in range(begin, begin + count):
        add_sample(oracle, c, spheres, s, *sums)
    return sums


@pytest.mark.parametrize("name, kernel, env, values", [
    ("final37", "bvh_lds(features)", None, TMAX),
    ("final37", "smem_u4(features)", "smem_u4", [1.2, 0.0]),
    ("chapter13", "lds_u4(features)", None, [1.2, 1e-3]),
    ("large", "bvh_global(features)", None, [1.2, -1.0]),
], ids=["bvh_lds", "smem_u4", "lds_u4", "bvh_global"])
def test_tmax_feature_pass(oracle, name, kernel, env, values, monkeypatch, renderers):
    """The feature pass's closest hit lies in (t_min, t_max) too; an empty interval leaves hits 0."""
    if env:
        monkeypatch.setenv("RTZIG_KERNEL", env)
    cam = scene(name)
    n = 2 if name == "large" else 3
    r = renderers(cam)
    P = cam.width * cam.height
    unbounded = None
    for t_max in [INF] + list(values):
        c = with_fields(cam.cam, t_max=t_max)
        buf = Buffers(P, poison=True)
        r.features(c, 0, 1, **buf.ptrs())
        r.features(c, 1, n - 1, **buf.ptrs())
        got = buf.host()
        assert r.kernel_name() == kernel
        want = feature_sums(oracle, c, cam.scene.world, 0, n)
        assert_equal(got, want, (name, t_max))
        if t_max == INF:
            unbounded = want
        elif t_max <= c.t_min:
            assert (got[3] == 0).all() and all((a == 0).all() for a in got[:3]), (name, t_max)
        elif t_max == 1.2:  # the bound does cut hits off: the case is not the unbounded one
            assert (want[3] < unbounded[3]).any(), name
    r.sync()
    r.close()


def gather_case(oracle, r, cam, c, base, n, where):
    """A sparse gather pass of n samples at camera struct c, every pixel standing at `base` samples on
    pre-filled buffers, then one over the other pixels: accum against oracle_accumulate_b, m2 in the
    stated order from per-sample colours (oracle_accumulate_b at count 1 from zero), counts, the rays
    of both passes together, and the unlisted pixels untouched in between."""
    W, H = cam.width, cam.height
    P = W * H
    world = cam.scene.world
    A = np.sort(list_a()) if P == 740 else np.arange(2, P, 3)
    rest = np.setdiff1d(np.arange(P), A)
    acc0, m20 = fill(P), fill(P, 1, salt=5)
    d_acc, d_m2 = torch.from_numpy(acc0).to(DEV), torch.from_numpy(m20).to(DEV)
    d_cnt = torch.full((P,), i32(base), dtype=torch.int32, device=DEV)
    st = torch.zeros(2, dtype=torch.int64, device=DEV)
    # a pixel without samples starts from 0: its sums are overwritten, not read
    start_acc = acc0 if base else np.zeros((P, 3))
    start_m2 = m20 if base else np.zeros(P)
    want_acc, want_rays = oracle.accumulate_b(c, world, base, n, start_acc.reshape(H, W, 3), threads=16)
    want_acc = want_acc.reshape(P, 3)
    want_m2 = start_m2.copy()
    for s in range(n):
        col = oracle.accumulate_b(c, world, base + s, 1, threads=16)[0].reshape(P, 3)
        y = (col[:, 0] + col[:, 1]) + col[:, 2]
        want_m2 = want_m2 + y * y
    perm = np.random.default_rng(9).permutation(A)
    r.accumulate_pixels(c, perm, n, d_acc.data_ptr(), d_m2.data_ptr(), d_cnt.data_ptr(), d_stats_ptr=st.data_ptr())
    torch.cuda.synchronize()
    assert "gather" in r.kernel_name()
    acc, m2, cnt = d_acc.cpu().numpy(), d_m2.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)
    assert np.array_equal(acc[A], want_acc[A]), (where, int((acc[A] != want_acc[A]).any(-1).sum()))
    assert np.array_equal(m2[A], want_m2[A]), where
    assert (cnt[A] == base + n).all() and (cnt[rest] == base).all(), where
    assert np.array_equal(acc[rest], acc0[rest]) and np.array_equal(m2[rest], m20[rest]), where
    assert int(st[1]) == len(A) * n
    r.accumulate_pixels(c, rest, n, d_acc.data_ptr(), d_m2.data_ptr(), d_cnt.data_ptr(), d_stats_ptr=st.data_ptr())
    torch.cuda.synchronize()
    r.sync()
    assert np.array_equal(d_acc.cpu().numpy(), want_acc) and np.array_equal(d_m2.cpu().numpy(), want_m2), where
    assert (d_cnt.cpu().numpy().view(np.uint32) == base + n).all(), where
    assert st.cpu().tolist() == [want_rays, P * n], where
    return want_acc


def test_tmax_gather_pass(oracle, renderers):
    cam = scene("final37")
    r = renderers(cam)
    sky = None
    for t_max in TMAX:
        c = with_fields(cam.cam, t_max=t_max)
        sums = gather_case(oracle, r, cam, c, 0, 3, ("gather", t_max))
        if t_max <= c.t_min:
            sky = sums if sky is None else sky
            assert np.array_equal(sums, sky)  # every empty interval gives the same sky sums
    r.close()


# ---- 64-bit seeds ------------------------------------------------------------------------------------
def test_seed_bit_63_changes_the_image_on_the_oracle(oracle):
    a = ref_b(oracle, "final64", seed=0xDEADBEEF)[0]
    b = ref_b(oracle, "final64", seed=0xDEADBEEF | 1 << 63)[0]
    assert (a != b).any(-1).mean() > 0.9
    imgs = [ref_b(oracle, "final64", seed=s)[0] for s in SEEDS]
    assert all((imgs[i] != imgs[j]).any(-1).mean() > 0.9 for i in range(4) for j in range(i))


@pytest.mark.parametrize("mode", MODES)
def test_seeds_colour_render(oracle, mode, monkeypatch, renderers):
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = scene("final64")
    r = renderers(cam)
    for seed in SEEDS:
        img, rays, samples = render_rows(r, with_fields(cam.cam, seed=seed))
        ref, ref_rays = ref_b(oracle, "final64", seed=seed)
        assert np.array_equal(img, ref) and rays == ref_rays and samples == 64 * 42 * 4, hex(seed)
        assert ("direct" in r.kernel_name()) == (mode == "direct")
    r.close()


def test_seeds_feature_pass(oracle, renderers):
    cam = scene("final37")
    r = renderers(cam)
    for seed in SEEDS:
        c = with_fields(cam.cam, seed=seed)
        buf = Buffers(740, poison=True)
        r.features(c, 0, 2, **buf.ptrs())
        assert_equal(buf.host(), feature_sums(oracle, c, cam.scene.world, 0, 2), hex(seed))
    r.sync()
    r.close()


def test_seeds_gather_pass(oracle, renderers):
    cam = scene("final37")
    r = renderers(cam)
    for seed in SEEDS:
        gather_case(oracle, r, cam, with_fields(cam.cam, seed=seed), 0, 3, hex(seed))
    r.close()


# ---- sample numbers with bit 31 set, up to the last admissible one ----------------------------------
RANGES = [(2 ** 31 - 7, 20), (LAST - 100, 100)]  # across 2^31; the last 100 samples: three chunks


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("begin, count", RANGES, ids=["across-2^31", "last-100"])
def test_high_sample_range_onto_a_filled_accumulator(oracle, begin, count, mode, monkeypatch, renderers):
    """Ring mode's chunk table (s_begin + rel[i]) and direct mode's sample number (fs + s_begin) with
    bit 31 set, continued from stored sums; a two-call split of the range gives the same bits."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = scene("final37")
    r = renderers(cam)
    acc0 = fill(740)
    want, want_rays = oracle.accumulate_b(cam.cam, cam.scene.world, begin, count, acc0.reshape(20, 37, 3), threads=16)
    for split in ([count], [37, count - 37] if count > 37 else [7, count - 7]):
        accum = torch.from_numpy(acc0).to(DEV)
        st = torch.zeros(2, dtype=torch.int64, device=DEV)
        done = begin
        for k in split:
            r.accumulate(cam.cam, accum.data_ptr(), done, k, d_stats_ptr=st.data_ptr())
            assert ("direct" in r.kernel_name()) == (mode == "direct")
            done += k
        r.sync()
        got = accum.cpu().numpy().reshape(20, 37, 3)
        assert np.array_equal(got, want), (split, int((got != want).any(-1).sum()))
        assert st.cpu().tolist() == [want_rays, 740 * count], split
    r.close()
    assert begin + count <= LAST and (want != acc0.reshape(20, 37, 3)).mean() > 0.9


@pytest.mark.parametrize("base, n", [(2 ** 31 - 7, 12), (LAST - 12, 12)], ids=["across-2^31", "to-the-last-count"])
def test_high_counts_gather_pass(oracle, base, n, renderers):
    """The gather pass builds the sample number as counts[p] + k, in the seed window and per lane."""
    cam = scene("final37")
    r = renderers(cam)
    gather_case(oracle, r, cam, cam.cam, base, n, (base, n))
    r.close()


def test_high_sample_begin_feature_pass(oracle, renderers):
    cam = scene("final37")
    begin = LAST - 8
    start = (fill(740), fill(740, salt=3), fill(740, 1, salt=7), np.full(740, 3, np.uint32))
    r = renderers(cam)
    buf = Buffers(740)
    for t, a in zip((buf.albedo, buf.normal, buf.depth), start):
        t.copy_(torch.from_numpy(a))
    buf.hits.fill_(3)
    r.features(cam.cam, begin, 5, **buf.ptrs())
    r.features(cam.cam, begin + 5, 3, **buf.ptrs())
    got = buf.host()
    r.sync()
    r.close()
    want = feature_sums(oracle, cam.cam, cam.scene.world, begin, 8, start)
    assert_equal(got, want)
    low = feature_sums(oracle, cam.cam, cam.scene.world, begin - 2 ** 31, 8, start)
    assert not np.array_equal(want[2], low[2])  # bit 31 of the sample number reaches the key


# ---- selection beyond one scan round, and counts above 2^31 ------------------------------------------
@pytest.fixture(scope="module")
def ctx(module_renderers):
    return module_renderers()


def run_select(r, accum, m2, counts, min_c, max_c, tol, floor):
    n = len(counts)
    d_accum, d_m2 = torch.from_numpy(accum).to(DEV), torch.from_numpy(m2).to(DEV)
    d_counts = torch.from_numpy(counts.astype(np.uint32).view(np.int32)).to(DEV)
    d_list = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_n = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    d_err = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
    r.select(d_accum.data_ptr(), d_m2.data_ptr(), d_counts.data_ptr(), n, min_c, max_c, tol, floor, d_list.data_ptr(),
             d_n.data_ptr(), d_err_ptr=d_err.data_ptr())
    k = int(d_n.item())
    return k, d_list.cpu().numpy(), d_err.cpu().numpy()


@pytest.mark.parametrize("n", [1024 ** 2 + 1024 + 17, 2 * 1024 ** 2 + 5], ids=["two-rounds", "three-rounds"])
@pytest.mark.parametrize("pattern", ["all", "alternating", "random", "single-last"])
def test_select_beyond_one_scan_round(ctx, pattern, n):
    """More than 1024 blocks of 1024 pixels: select_scan_kernel's second and third rounds, whose block
    offsets start from the total the earlier rounds carried."""
    assert (n + SEL_BLOCK - 1) // SEL_BLOCK > SEL_BLOCK
    accum, m2, counts = synthetic(pattern, n)
    want, want_err = select_numpy(accum, m2, counts)
    k, lst, err = run_select(ctx, accum, m2, counts, MIN_C, MAX_C, TOL, FLOOR)
    assert k == len(want)
    assert np.array_equal(lst[:k], want)
    assert dv.same_bits_or_nan(err, want_err)
    if pattern == "all":
        assert k == n
    if pattern == "single-last":
        assert want.tolist() == [n - 1]
    if pattern in ("alternating", "random"):  # selected pixels on both sides of the round boundary
        assert (want < SEL_BLOCK ** 2).any() and (want >= SEL_BLOCK ** 2).any()


def test_select_huge_counts(ctx):
    """Counts at and above 2^31 convert to double unsigned; max_count = 2^32 - 1 holds the last count
    back.  The numpy side goes through uint64."""
    n = 3 * SEL_BLOCK + 17
    rng = np.random.default_rng(41)
    counts = rng.choice(np.array([2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], np.uint64), n)
    c = counts.astype(np.float64)
    assert c.min() == 2.0 ** 31 - 1 and c.max() == 2.0 ** 32 - 1
    accum = np.array([0.1, 0.2, 0.3]) * (1 + rng.random((n, 1))) * c[:, None]
    S = (accum[:, 0] + accum[:, 1]) + accum[:, 2]
    m2 = S * (S / c) * (1 + 6 * rng.random(n))  # err = sqrt(k / (n - 1)), k < 6: up to 5.3e-5
    tol = 2e-5
    want, want_err = select_numpy(accum, m2, counts, min_c=4, max_c=LAST, tol=tol, floor=0.01)
    assert 0 < len(want) < n and (counts[want] < LAST).all()
    assert ((want_err > tol) & (counts == LAST)).any()  # held back by max_count alone
    k, lst, err = run_select(ctx, accum, m2, counts, 4, LAST, tol, 0.01)
    assert k == len(want) and np.array_equal(lst[:k], want)
    assert np.array_equal(err.view(np.int64), want_err.view(np.int64))


# ---- the resolve kernels on synthetic accumulators ---------------------------------------------------
def run_resolve(r, a, n_samples, output, counts=None):
    """rt_accum_resolve (or _counts) of the (n, 3) array a into a buffer with guard elements behind the
    last pixel: (the n pixels, True if the guard is untouched)."""
    n = len(a)
    d_a = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if output == "linear":
        out = torch.full((3 * n + 8,), -7.5, dtype=torch.float64, device=DEV)
    else:
        out = torch.full((3 * n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    if counts is None:
        r.resolve(d_a.data_ptr(), n, n_samples, out.data_ptr(), output=output)
    else:
        d_c = torch.from_numpy(counts.astype(np.uint32).view(np.int32)).to(DEV)
        r.resolve_counts(d_a.data_ptr(), d_c.data_ptr(), n, out.data_ptr(), output=output)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    guard = host[3 * n:]
    return host[:3 * n].reshape(n, 3), bool((guard == (-7.5 if output == "linear" else 0xA5)).all())


@pytest.mark.parametrize("n_samples", [1, 3, 7, 500, 2 ** 31, LAST])
def test_resolve_on_byte_boundaries_and_unrendered_values(ctx, oracle, n_samples):
    a = dv.pixels(3 * 256 + 17)
    assert len(dv.channel_values()) <= len(a)  # every channel meets every value
    with np.errstate(all="ignore"):
        want = a * (1.0 / np.float64(n_samples))
    lin, ok = run_resolve(ctx, a, n_samples, "linear")
    assert ok and dv.same_bits_or_nan(lin, want)
    if n_samples == 1:
        assert dv.same_bits_or_nan(lin, a)
    rgb, ok = run_resolve(ctx, a, n_samples, "rgb8")
    ref = oracle.to_rgb8(want)
    assert ok and np.array_equal(rgb, ref), np.argwhere(rgb != ref)[:8].tolist()
    if n_samples == 1:
        assert len(np.unique(rgb)) == 256


@pytest.mark.parametrize("n_pixels", [1, 255, 256, 257, 3 * 256 + 17])
def test_resolve_writes_exactly_its_pixels(ctx, oracle, n_pixels):
    """Block edges of the 256-thread resolve; the RGB8 stores are 3 bytes per pixel, so a wider store
    at the last pixel would land in the guard."""
    a = dv.pixels(3 * 256 + 17)[-n_pixels:]
    with np.errstate(all="ignore"):
        want = a * (1.0 / np.float64(7))
    lin, ok = run_resolve(ctx, a, 7, "linear")
    assert ok and dv.same_bits_or_nan(lin, want)
    rgb, ok = run_resolve(ctx, a, 7, "rgb8")
    assert ok and np.array_equal(rgb, oracle.to_rgb8(want))
    cnt = np.full(n_pixels, 7, np.uint64)
    lin, ok = run_resolve(ctx, a, None, "linear", counts=cnt)
    assert ok and dv.same_bits_or_nan(lin, want)
    rgb, ok = run_resolve(ctx, a, None, "rgb8", counts=cnt)
    assert ok and np.array_equal(rgb, oracle.to_rgb8(want))


def test_resolve_counts_up_to_the_last_count(ctx, oracle):
    """Every value under every count, the counts converted unsigned; a pixel without samples is exactly
    0 whatever its sums hold (NaN here)."""
    C = np.array([0, 1, 2, 3, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, LAST], np.uint64)
    n = 8 * len(dv.channel_values())
    a = dv.pixels(n, repeat=8)
    counts = C[np.arange(n) % 8]
    a[counts == 0] = np.nan
    with np.errstate(all="ignore"):
        want = a * (1.0 / counts.astype(np.float64))[:, None]
    want[counts == 0] = 0.0
    lin, ok = run_resolve(ctx, a, None, "linear", counts=counts)
    assert ok and dv.same_bits_or_nan(lin, want)
    assert (lin[counts == 0].view(np.int64) == 0).all()
    rgb, ok = run_resolve(ctx, a, None, "rgb8", counts=counts)
    assert ok and np.array_equal(rgb, oracle.to_rgb8(want))
    one = counts == 1
    assert np.array_equal(rgb[one], oracle.to_rgb8(a[one])) and len(np.unique(rgb[one])) == 256

"""Ray queries on the GPU (include/rt.h rt_trace_rays): the closest hit of
caller-supplied rays, bit for bit HittableList.hit's.

The reference is computed here, on the CPU, from the oracle's per-ray helpers alone: oracle.world_hit
for the winning sphere and its root, then oracle.sphere_hit on that sphere for the point, the normal
and the face.  Every comparison is np.array_equal on the raw values (equal_nan for the normal: the
zero-radius sphere's 1 / r is infinite).  The hit shares asserted on the reference are input
conditions — they say that a case exercises what it is meant to — not tolerances."""
import math

import numpy as np
import pytest
import torch

import fast_scenes
import rtzig
from gpu_support import DEV, cached
from gpu_support import module_renderers, renderers  # noqa: F401 (fixtures)
from rtzig.lib import RtError
from trace_support import FIELDS, Out, assert_equal, assert_sentinel, trace

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
N = 4096


# ---- rays and the reference --------------------------------------------------------------------------
def base_rays():
    g = np.random.default_rng(1)
    O = g.uniform([-12, .05, -12], [12, 3, 12], (N, 3))
    D = g.standard_normal((N, 3))
    return O, D


def intervals_of(n, t_min, t_max):
    iv = np.empty((n, 2))
    iv[:, 0] = t_min
    iv[:, 1] = t_max
    return iv


def ref_hits(oracle, spheres, O, D, iv):
    """HittableList.hit of every ray (O[q], D[q]) in (iv[q, 0], iv[q, 1]): the dict rt_trace_rays fills."""
    n = len(O)
    out = dict(index=np.full(n, -1, np.int32), t=np.full(n, INF), point=np.zeros((n, 3)), normal=np.zeros((n, 3)),
               front=np.zeros(n, np.uint8))
    for q in range(n):
        o, d = O[q].tolist(), D[q].tolist()
        k, t = oracle.world_hit(spheres, o, d, float(iv[q, 0]), float(iv[q, 1]))
        if k < 0:
            continue
        rec = oracle.sphere_hit(spheres[k], o, d, float(iv[q, 0]), float(iv[q, 1]))
        assert rec is not None and rec["t"] == t
        out["index"][q], out["t"][q], out["front"][q] = k, t, rec["front"]
        out["point"][q], out["normal"][q] = rec["point"], rec["normal"]
    for a in out.values():
        a.setflags(write=False)
    return out


def final_cam():
    return cached("final_cam", lambda: rtzig.final_scene_camera(width=48, aspect_ratio=16 / 9, spp=2))


def base_ref(oracle):
    O, D = cached("base_rays", base_rays)
    return cached("base_ref", lambda: ref_hits(oracle, final_cam().scene.world, O, D, intervals_of(N, 1e-3, INF)))


def share(ref):
    return float((ref["index"] >= 0).mean())


# ---- 1. base, all five outputs, BVH in LDS -----------------------------------------------------------
def test_base_rays_all_outputs_bvh_in_lds(oracle, renderers):
    O, D = cached("base_rays", base_rays)
    ref = base_ref(oracle)
    # input conditions
    assert abs(share(ref) - 0.4985) < 0.0006
    assert abs(float((ref["index"] == 0).mean()) - 0.377) < 0.0006  # the ground sphere
    assert len(set(ref["index"].tolist())) == 272  # 271 distinct spheres, and the miss
    r = renderers(final_cam().scene.world)
    assert r.tree_info()["bvh"] == 1
    got, stats = trace(r, O, D)
    assert "(trace)" in r.kernel_name() and r.kernel_name().startswith("bvh_lds")
    assert stats == [N, 0]
    assert_equal(got, ref, label="base")
    for n in (1, 63, 64, 65):
        got, stats = trace(r, O[:128], D[:128], n=n)
        assert stats == [n, 0]
        assert_equal(got, ref, n=n, label="prefix %d" % n)
        assert_sentinel(got, n)
    r.close()


# ---- 2. intervals ------------------------------------------------------------------------------------
def interval_cases(oracle):
    """name -> (rays used, scalar (t_min, t_max) or None, per-ray intervals or None, check(ref, base))."""
    base = base_ref(oracle)
    first = base["t"]  # inf on a miss

    def peel(ref, b):
        had = b["index"] >= 0
        assert abs(float((ref["index"][had] >= 0).mean()) - 0.988) < 0.0006
        both = had & (ref["index"] >= 0)
        assert (ref["t"][both] > b["t"][both]).all()

    def neg_all(ref, b):
        assert abs(share(ref) - 0.939) < 0.0006
        hit = ref["index"] >= 0
        assert 0.4 < float((ref["t"][hit] < 0).mean()) < 0.6

    def same(ref, b):
        assert all(np.array_equal(ref[f], b[f][:len(ref[f])], equal_nan=True) for f in FIELDS)

    def none(ref, b):
        assert share(ref) == 0.0

    def near(x):
        return lambda ref, b: abs(share(ref) - x) < 0.0006

    def check(f):
        def run(ref, b):
            assert f(ref, b) is not False
        return run

    def tmax2(ref, b):
        assert abs(share(ref) - 0.276) < 0.0006
        assert abs(float((ref["index"] != b["index"]).mean()) - 0.223) < 0.0006

    iv_tmax = intervals_of(N, 1e-3, np.random.default_rng(2).uniform(.5, 20, N))
    return {
        "tmax2": (N, (1e-3, 2.0), None, tmax2),
        "per_ray_tmax": (N, None, iv_tmax, check(lambda ref, b: abs(share(ref) - 0.432) < 0.0006)),
        "peel": (N, None, intervals_of(N, first, INF), peel),
        "strict_tmax": (N, None, intervals_of(N, 1e-3, first), none),
        "neg_all": (512, (-INF, INF), None, neg_all),
        "neg_5": (512, (-5.0, INF), None, check(near(0.863))),
        "neg_behind": (512, (-INF, 0.0), None, check(near(0.469))),
        "zero_tmin": (N, (0.0, INF), None, same),
        "tiny_tmin": (N, (1e-300, INF), None, same),
        "huge_tmax": (N, (1e-3, 1e300), None, same),
        "tiny_tmax": (N, (1e-3, 1e-300), None, none),
        "inverted": (N, (1e-3, -1.0), None, none),
        "nan_tmin": (N, (NAN, INF), None, none),
        "nan_tmax": (N, (1e-3, NAN), None, none),
    }


CASES = ["tmax2", "per_ray_tmax", "peel", "strict_tmax", "neg_all", "neg_5", "neg_behind", "zero_tmin", "tiny_tmin",
         "huge_tmax", "tiny_tmax", "inverted", "nan_tmin", "nan_tmax"]


@pytest.fixture(scope="module")
def final_renderer(module_renderers):
    return module_renderers(final_cam().scene.world)


@pytest.mark.parametrize("name", CASES)
def test_interval_cases(oracle, final_renderer, name):
    O, D = cached("base_rays", base_rays)
    n, scalar, iv, check = interval_cases(oracle)[name]
    O, D = O[:n], D[:n]
    ref_iv = iv[:n] if iv is not None else intervals_of(n, *scalar)
    ref = cached("iv_" + name, lambda: ref_hits(oracle, final_cam().scene.world, O, D, ref_iv))
    check(ref, base_ref(oracle))
    if scalar is not None:
        got, stats = trace(final_renderer, O, D, t_min=scalar[0], t_max=scalar[1])
    else:
        got, stats = trace(final_renderer, O, D, t_min=NAN, t_max=NAN, iv=ref_iv)  # the scalars are not used
    assert stats[0] == n
    assert_equal(got, ref, label=name)


def test_interval_edge_cases_interleaved_lane_by_lane(oracle, final_renderer):
    O, D = cached("base_rays", base_rays)
    O, D = O[:1024], D[:1024]
    edge = [(1e-3, INF), (-INF, INF), (1e-3, -1.0), (NAN, INF), (0.0, INF), (-5.0, INF), (1e-3, NAN), (1e-3, 2.0),
            (-INF, 0.0), (1e-300, INF), (1e-3, 1e-300), (INF, INF), (-INF, -INF), (1e-3, 1e300), (-0.0, 0.5)]
    iv = np.array([edge[q % len(edge)] for q in range(1024)])
    ref = cached("iv_mixed", lambda: ref_hits(oracle, final_cam().scene.world, O, D, iv))
    assert 0.2 < share(ref) < 0.8
    got, stats = trace(final_renderer, O, D, iv=iv)
    assert stats[0] == 1024 and 0 < stats[1] < 1024  # both routes in every wave
    assert_equal(got, ref, label="mixed")


def test_non_finite_and_zero_components_are_misses_and_scanned(oracle, final_renderer):
    """Every component in turn NaN, +inf, -inf; zero directions; all six NaN.  Legal input: the result is
    what the reference's comparisons give, a miss in every case, and none of these rays may use the tree."""
    O, D = cached("base_rays", base_rays)
    O, D = O[:640].copy(), D[:640].copy()
    bad = (NAN, INF, -INF)
    for q in range(576):  # 18 kinds, lane by lane
        (O if q % 6 < 3 else D)[q, q % 3] = bad[(q // 6) % 3]
    D[576:608] = 0.0
    D[592:608, 1] = -0.0
    O[608:640], D[608:640] = NAN, NAN
    ref = cached("non_finite", lambda: ref_hits(oracle, final_cam().scene.world, O, D, intervals_of(640, 1e-3, INF)))
    assert share(ref) == 0.0
    got, stats = trace(final_renderer, O, D)
    assert stats == [640, 640]
    assert_equal(got, ref, label="non-finite")
    # interleaved with ordinary rays, which stay on the tree and keep their hits
    O2, D2 = cached("base_rays", base_rays)
    O2, D2 = O2[:640].copy(), D2[:640].copy()
    O2[::2], D2[::2] = O[::2], D[::2]
    base = base_ref(oracle)
    got, stats = trace(final_renderer, O2, D2)
    assert stats == [640, 320]
    assert (got["index"][::2] == -1).all() and np.isinf(got["t"][::2]).all()
    assert_equal({f: got[f][1::2] for f in FIELDS}, {f: base[f][1:640:2] for f in FIELDS}, label="interleaved")


# ---- 3. the scale ladder -----------------------------------------------------------------------------
@pytest.mark.parametrize("e", [-140, -60, 60, 140, 400, -1000, -600, 600])
def test_direction_scale_ladder(oracle, final_renderer, e):
    O, D = cached("base_rays", base_rays)
    O, D = O[:1024], D[:1024]
    base = base_ref(oracle)
    Ds = D * 2.0 ** e  # a power of two: exact, or a clean underflow / overflow
    t_min = 1e-3 * 2.0 ** -e
    ref = cached("scale_%d" % e, lambda: ref_hits(oracle, final_cam().scene.world, O, Ds, intervals_of(1024, t_min, INF)))
    if e in (-1000, -600, 600):
        assert share(ref) == 0.0
    else:
        assert np.array_equal(ref["index"], base["index"][:1024])
        assert np.array_equal(ref["t"] * 2.0 ** e, base["t"][:1024])
    got, stats = trace(final_renderer, O, Ds, t_min=t_min)
    assert_equal(got, ref, label="2^%d" % e)
    assert stats[0] == 1024
    if abs(e) >= 140:
        assert stats[1] == 1024  # outside any f32 range the slab walk could be trusted in


# ---- 4. far origins ----------------------------------------------------------------------------------
def test_far_origins_scan_then_tree_after_reserve(oracle, renderers):
    O, D = cached("base_rays", base_rays)
    Of = O * 400
    Df = -Of + D
    cam = final_cam()
    ref = cached("far", lambda: ref_hits(oracle, cam.scene.world, Of, Df, intervals_of(N, 1e-3, INF)))
    assert 4798 < np.abs(Of).max() < 4800
    assert abs(share(ref) - 0.987) < 0.0015  # 4048 of 4096
    r = renderers(cam.scene.world)
    # the tree's bound is the scene's extent, 2000 (the ground sphere: |c_y| + r).  Rays starting
    # within it belong on the tree (rt_trace.h keeps them there), so the scan takes exactly the
    # rays beyond it: most of the batch, and all of the sub-batch that lies beyond
    bound = r.origin_bound()
    assert 2000 <= bound < 2001
    beyond = np.abs(Of).max(axis=1) > bound
    assert beyond.mean() > 0.8
    got, stats = trace(r, Of, Df)
    assert stats == [N, int(beyond.sum())]
    assert_equal(got, ref, label="far, scanned")
    n_b = int(beyond.sum())
    got_b, stats = trace(r, Of[beyond], Df[beyond])
    assert stats == [n_b, n_b]
    assert_equal(got_b, {f: ref[f][beyond] for f in FIELDS}, label="far, every ray scanned")
    r.reserve_origin_bound(6000)
    assert 6000 <= r.origin_bound() < 6100
    got, stats = trace(r, Of, Df)
    assert stats == [N, 0]
    assert_equal(got, ref, label="far, tree")
    bound = r.origin_bound()
    r.reserve_origin_bound(100)  # smaller: a no-op
    assert r.origin_bound() == bound
    # the renderer on the rebuilt tree
    W, H = cam.width, cam.height
    img = torch.empty((H, W, 3), dtype=torch.float64, device=DEV)
    r.render_rows_async(cam.cam, img.data_ptr())
    torch.cuda.synchronize()
    r.sync()
    ref_img = cached("final48_b", lambda: oracle.render_b(cam.cam, cam.scene.world, threads=4)[0])
    assert np.array_equal(img.cpu().numpy(), ref_img)
    r.close()


# ---- 5. other structures -----------------------------------------------------------------------------
def test_chapter13_list_walk_scans_every_ray(oracle, renderers):
    cam = cached("ch13", lambda: rtzig.chapter13_camera(width=37))
    g = np.random.default_rng(5)
    O = g.uniform([-3, -0.4, -3], [3, 2, 1], (1000, 3))
    D = g.standard_normal((1000, 3))
    ref = cached("ch13_ref", lambda: ref_hits(oracle, cam.scene.world, O, D, intervals_of(1000, 1e-3, INF)))
    assert 0.3 < share(ref) < 0.9 and len(set(ref["index"].tolist())) == 6  # every sphere, and misses
    r = renderers(cam.scene.world)
    assert r.tree_info()["bvh"] == 0 and r.origin_bound() == 0.0
    got, stats = trace(r, O, D)
    assert "(trace)" in r.kernel_name() and "bvh" not in r.kernel_name()
    assert stats == [1000, 1000]
    assert_equal(got, ref, label="chapter 13")
    r.close()


def test_large_scene_global_memory_tree(oracle, renderers):
    cam = cached("large", fast_scenes.large)
    O, D = cached("base_rays", base_rays)
    O, D = O[:1024] * 2.5, D[:1024]
    ref = cached("large_ref", lambda: ref_hits(oracle, cam.scene.world, O, D, intervals_of(1024, 1e-3, INF)))
    assert 0.4 < share(ref) < 0.9 and len(set(ref["index"].tolist())) > 50
    r = renderers(cam.scene.world)
    assert r.tree_info()["bvh"] == 1
    got, stats = trace(r, O, D)
    assert r.kernel_name() == "bvh_global(trace)"
    assert stats == [1024, 0]
    assert_equal(got, ref, label="large")
    r.close()


@pytest.mark.parametrize("precision, bvh", [("f64", 0), ("f32", 1)])
def test_exact_duplicate_never_wins_and_zero_radius_sphere(oracle, precision, bvh, renderers):
    """fast_scenes.materials(): sphere 5 is an exact copy of sphere 4, sphere 6 has radius 0.  Seven
    spheres walk the list on a parity context and the tree on an RT_PRECISION_F32 one (the trace itself is
    always parity arithmetic): the lowest index wins in both."""
    cam = cached("materials", fast_scenes.materials)
    g = np.random.default_rng(9)
    O = g.uniform([-3, 0.6, -3], [3, 3, 2], (1024, 3))
    D = np.array([1.0, 0.0, -1.0]) - O
    D[512:] += g.standard_normal((512, 3)) * 0.3  # around the target too: every sphere, and misses
    O[1000:] = [0.0, 2.0, -1.0]                   # straight down through the zero-radius sphere
    D[1000:] = [0.0, -1.0, 0.0]
    ref = cached("materials_ref", lambda: ref_hits(oracle, cam.scene.world, O, D, intervals_of(1024, 1e-3, INF)))
    assert (ref["index"][:512] == 4).mean() > 0.9 and not (ref["index"] == 5).any()
    r = renderers(cam.scene.world, precision)
    assert r.tree_info()["bvh"] == bvh
    got, stats = trace(r, O, D)
    assert stats == [1024, 1024 * (1 - bvh)]
    assert not (got["index"] == 5).any()
    assert_equal(got, ref, label="materials " + precision)
    r.close()


# ---- 6. tree independence ----------------------------------------------------------------------------
def test_trained_tree_gives_the_same_bits(oracle, monkeypatch, renderers):
    O, D = cached("base_rays", base_rays)
    ref = base_ref(oracle)
    cam = final_cam()
    monkeypatch.setenv("RTZIG_BVH_TRAIN", "1")
    r = renderers(cam.scene.world)
    img = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device=DEV)
    r.render_rows_async(cam.cam, img.data_ptr())
    torch.cuda.synchronize()
    assert r.tree_info()["trained"] == 1
    got, stats = trace(r, O, D)
    assert stats == [N, 0]
    assert_equal(got, ref, label="trained tree")
    r.close()


# ---- 7. plumbing -------------------------------------------------------------------------------------
def test_stride_4_and_output_subsets(oracle, final_renderer):
    O, D = cached("base_rays", base_rays)
    O, D = O[:1000], D[:1000]
    ref = base_ref(oracle)
    got, stats = trace(final_renderer, O, D, stride=4)
    assert stats == [1000, 0]
    assert_equal(got, ref, n=1000, label="stride 4")
    got, _ = trace(final_renderer, O, D, stride=0)  # 0 means 3
    assert_equal(got, ref, n=1000, label="stride 0")
    for fields in (("index",), ("t",), ("point",), ("normal",), ("front",), ("index", "t"), ("point", "front"), ()):
        got, stats = trace(final_renderer, O, D, fields=fields)
        assert stats == [1000, 0]  # d_stats alone still launches
        assert_equal(got, ref, n=1000, fields=fields, label="subset %s" % (fields,))
        assert_sentinel(got, 0, fields=[f for f in FIELDS if f not in fields])


def test_non_default_stream_needs_no_host_sync(oracle, final_renderer):
    O, D = cached("base_rays", base_rays)
    ref = base_ref(oracle)
    h_o, h_d = torch.from_numpy(O).pin_memory(), torch.from_numpy(D).pin_memory()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        out = Out(N)  # the sentinel fills run on the stream too
        # the inputs are produced on the stream: copies, then arithmetic that leaves the bits alone
        d_o = h_o.to(DEV, non_blocking=True) * 1.0
        d_d = h_d.to(DEV, non_blocking=True) + 0.0
        final_renderer.trace_rays(d_o.data_ptr(), d_d.data_ptr(), N, stream_ptr=s.cuda_stream, **out.ptrs())
        idx2 = out.index * 2  # consumed on the stream
        got = {f: getattr(out, f).to("cpu", non_blocking=True) for f in FIELDS}
    s.synchronize()
    assert_equal({f: v.numpy() for f, v in got.items()}, ref, label="stream")
    assert np.array_equal(idx2.cpu().numpy(), ref["index"] * 2)


@pytest.mark.parametrize("kind", ["instrumented", "f32"])
def test_instrumented_and_f32_contexts_give_the_same_bits(oracle, kind, renderers):
    O, D = cached("base_rays", base_rays)
    ref = base_ref(oracle)
    r = renderers(final_cam().scene.world, "f32" if kind == "f32" else "f64")
    if kind == "instrumented":
        r.enable_profile(True)
    got, stats = trace(r, O, D)
    assert stats == [N, 0] and "(trace)" in r.kernel_name()
    assert_equal(got, ref, label=kind)
    r.close()


def test_kernel_times_and_empty_calls(oracle, renderers):
    O, D = cached("base_rays", base_rays)
    r = renderers(final_cam().scene.world)
    r.enable_timing(True)
    trace(r, O[:256], D[:256])
    sample_ms, reduce_ms = r.kernel_times()
    assert sample_ms > 0 and reduce_ms == 0
    name = r.kernel_name()
    # n_rays == 0 and "nothing asked for" return RT_OK and launch nothing
    out = Out(4)
    r.trace_rays(1, 1, 0, **out.ptrs())          # the pointers are never read
    r.trace_rays(1, 1, 4)
    torch.cuda.synchronize()
    assert_sentinel(out.host(), 0)
    assert r.kernel_name() == name
    r.close()
    r = renderers()
    with pytest.raises(RtError, match="no scene"):
        r.trace_rays(1, 1, 4, d_index_ptr=1)
    with pytest.raises(RtError, match="no scene"):
        r.reserve_origin_bound(10.0)
    r.close()


# ---- 8. Python ---------------------------------------------------------------------------------------
def test_python_wrappers_equal_the_device_result(oracle):
    O, D = cached("base_rays", base_rays)
    O, D = O[:777], D[:777]
    ref = base_ref(oracle)
    scene = final_cam().scene
    for got in (rtzig.trace_rays(scene.world, O, D), scene.hit(O, D)):
        assert got["front"].dtype == bool and got["index"].dtype == np.int32
        got = dict(got, front=got["front"].astype(np.uint8))
        assert_equal(got, ref, n=777, label="python")
    iv = intervals_of(777, 1e-3, 2.0)
    ref2 = cached("iv_tmax2", lambda: ref_hits(oracle, scene.world, *cached("base_rays", base_rays), intervals_of(N, 1e-3, 2.0)))
    got = scene.hit(O, D, intervals=iv)
    assert_equal(dict(got, front=got["front"].astype(np.uint8)), ref2, n=777, label="python intervals")
    got = scene.hit(O, D, t_max=2.0)
    assert_equal(dict(got, front=got["front"].astype(np.uint8)), ref2, n=777, label="python t_max")
    assert rtzig.trace_rays(scene.world, np.zeros((0, 3)), np.zeros((0, 3)))["index"].shape == (0,)


def test_object_id_map_of_the_pixel_centre_rays(oracle):
    cam = final_cam()
    c = cam.cam
    W, H = cam.width, cam.height
    jj, ii = np.mgrid[0:H, 0:W]
    px = [(c.pixel0[k] + c.du[k] * ii.astype(np.float64)) + c.dv[k] * jj.astype(np.float64) for k in range(3)]
    O = np.tile(np.array(list(c.center)), (H * W, 1))
    D = np.stack([p.ravel() for p in px], axis=1) - O
    ref = cached("idmap", lambda: ref_hits(oracle, cam.scene.world, O, D, intervals_of(H * W, c.t_min, c.t_max)))
    assert 0.5 < share(ref) < 1.0 and len(set(ref["index"].tolist())) > 20
    got = cam.scene.hit(O, D, t_min=c.t_min, t_max=c.t_max)
    assert np.array_equal(got["index"].reshape(H, W), ref["index"].reshape(H, W))
    assert np.array_equal(got["t"], ref["t"])

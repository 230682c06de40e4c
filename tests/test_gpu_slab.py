"""The BVH walk's f32 slab test on the device, on the rays its padding certificate is tightest for
(csrc/rt_bvh.cpp "Padding rules"; tests/slab_support.py): skimming rays through rt_trace_rays and
rt_occluded_rays, and a camera whose every primary ray skims through the path loop.

Every comparison is bit for bit against the oracle (oracle.world_hit / oracle.sphere_hit per ray,
oracle.render_b per image), and every ray query asserts stats == [N, 0]: no ray may be left to the list
scan, which would answer it without the boxes.  A walk that dropped a box these rays need — a shaved
pad, a bound rounded inward, a broken broadcast in the packed fma — shows here as a lost hit.  That the
rays do need the pad is shown on the CPU (tests/test_slab_inputs.py, the control)."""
import numpy as np
import pytest
import torch

import fast_scenes
import occlusion_support as occ
import rtzig
import slab_support as ss
from gpu_support import DEV, cached
from gpu_support import renderers  # noqa: F401 (fixture)
from trace_support import assert_equal, trace

pytestmark = pytest.mark.gpu

N = ss.N


# ---- the cases -------------------------------------------------------------------------------------------
def world_of(name):
    def make():
        if name == "final":
            return rtzig.final_scene_camera(width=48, aspect_ratio=16 / 9, spp=2)
        if name == "large":
            return fast_scenes.large()
        return fast_scenes.lattice(int(name.split("_")[1]))
    made = cached("slab_world_" + name, make)
    return made.scene.world if hasattr(made, "scene") else made.world


def case(oracle, name, n=N, **kw):
    """(world, O, D, reference) of a named case: computed once, read-only.  The first word of the name is
    the scene; a suffix (lattice_0_far) is another ray set over it."""
    world = world_of("_".join(name.split("_")[:2]) if name.startswith("lattice") else name)

    def make():
        O, D = ss.case_rays(name, world, n, **kw)
        ref = ss.ref_hits(oracle, world, O, D)
        assert (ref["index"] >= 0).mean() >= 0.95, "%s: only %.3f of the rays hit" % (name, (ref["index"] >= 0).mean())
        return O, D, ref
    return (world,) + cached("slab_case_" + name, make)


def tree_renderer(renderers, world, O, precision="f64"):
    """A renderer whose tree covers the origins: the bound is reserved where the scene's own is short."""
    r = renderers(world, precision)
    assert r.tree_info()["bvh"] == 1
    need = float(np.abs(O).max())
    if r.origin_bound() < need:
        r.reserve_origin_bound(need)
    assert r.origin_bound() >= need
    return r


def check_trace(r, O, D, ref, label):
    got, stats = trace(r, O, D)
    assert stats == [len(O), 0], "%s: stats %s" % (label, stats)
    assert_equal(got, ref, label=label)


# ---- 1. rt_trace_rays ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ss.LATTICE_T)
def test_lattice_bvh_in_lds(oracle, T, renderers):
    world, O, D, ref = case(oracle, "lattice_%d" % T)
    assert (ref["index"] >= 0).all() and len(set(ref["index"].tolist())) == 64
    r = tree_renderer(renderers, world, O)
    assert r.tree_info()["always"] == 0  # every sphere stands behind boxes
    check_trace(r, O, D, ref, "lattice %d" % T)
    assert "(trace)" in r.kernel_name() and r.kernel_name().startswith("bvh_lds")
    r.close()


def test_final_scene_sah_tree(oracle, renderers):
    world, O, D, ref = case(oracle, "final")
    r = tree_renderer(renderers, world, O)
    assert r.tree_info()["trained"] == 0
    check_trace(r, O, D, ref, "final")
    assert "(trace)" in r.kernel_name() and r.kernel_name().startswith("bvh_lds")
    r.close()


def test_final_scene_trained_tree(oracle, monkeypatch, renderers):
    world, O, D, ref = case(oracle, "final")
    cam = cached("slab_world_final", None)
    monkeypatch.setenv("RTZIG_BVH_TRAIN", "1")
    r = tree_renderer(renderers, world, O)
    img = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device=DEV)
    r.render_rows_async(cam.cam, img.data_ptr())
    torch.cuda.synchronize()
    assert r.tree_info()["trained"] == 1
    check_trace(r, O, D, ref, "final, trained tree")
    r.close()


def test_large_scene_global_memory_tree(oracle, renderers):
    world, O, D, ref = case(oracle, "large", n=1024)
    assert len(set(ref["index"].tolist())) > 500
    r = tree_renderer(renderers, world, O)
    check_trace(r, O, D, ref, "large")
    assert r.kernel_name() == "bvh_global(trace)"
    r.close()


def test_origins_out_at_a_reserved_bound(oracle, renderers):
    """The |o| part of the pad: origins 5000 to 5990 away along the travel axis, a tree reserved for 6000."""
    world, O, D, ref = case(oracle, "lattice_0_far", reach=(5000, 5990))
    assert 5900 < np.abs(O).max() < 6000
    r = renderers(world)
    assert r.origin_bound() < 4  # the scene's own extent: every one of these rays would be scanned
    r.reserve_origin_bound(6000)
    assert 6000 <= r.origin_bound() < 6100
    check_trace(r, O, D, ref, "bound 6000")
    r.close()


# ---- 2. rt_occluded_rays: the any-hit walk, whose upper never shrinks ----------------------------------------
@pytest.mark.parametrize("name", ["lattice_0", "lattice_64", "lattice_1024", "final"])
def test_occlusion_bytes_and_bits(oracle, name, renderers):
    world, O, D, ref = case(oracle, name)
    want = ref["index"] >= 0
    r = tree_renderer(renderers, world, O)
    got = occ.query(r, O, D)
    assert got["stats"] == [N, 0, int(want.sum())]
    occ.assert_answers(got, want, label=name)
    r.close()


# ---- 3. other instantiations of the walker ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice_64", "final"])
@pytest.mark.parametrize("kind", ["instrumented", "f32"])
def test_instrumented_and_f32_contexts_give_the_same_bits(oracle, kind, name, renderers):
    world, O, D, ref = case(oracle, name)
    r = tree_renderer(renderers, world, O, "f32" if kind == "f32" else "f64")
    if kind == "instrumented":
        r.enable_profile(True)
    check_trace(r, O, D, ref, "%s, %s" % (name, kind))
    assert "(trace)" in r.kernel_name()
    r.close()


# ---- 4. the path loop: run_f64 with suspension and resume --------------------------------------------------
@pytest.mark.parametrize("mode", ["ring", "direct"])
@pytest.mark.parametrize("dv_y", [2.0 ** -30, 0.0])
@pytest.mark.parametrize("T", [0, 64])
def test_path_loop_every_primary_ray_skims(oracle, T, dv_y, mode, monkeypatch, renderers):
    """fast_scenes.skim_camera: 64 x 4 at 8 spp, bounce_max 4; that its primary rays hit under the pole
    plane is checked on the CPU (tests/test_slab_inputs.py)."""
    cam = cached(("slab_cam", T, dv_y), lambda: fast_scenes.skim_camera(T, dv_y))
    ref, rays = cached(("slab_img", T, dv_y), lambda: oracle.render_b(cam.cam, cam.scene.world, threads=4))
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    r = renderers(cam.scene.world)
    assert r.tree_info()["bvh"] == 1
    img = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device=DEV)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)  # {rays, samples}
    r.render_rows_async(cam.cam, img.data_ptr(), d_stats_ptr=stats.data_ptr())
    torch.cuda.synchronize()
    r.sync()
    assert r.kernel_name().startswith("bvh_lds") and ("direct" in r.kernel_name()) == (mode == "direct")
    got = img.cpu().numpy()
    assert np.array_equal(got, ref), "%d of %d pixels differ" % (int((got != ref).any(-1).sum()), cam.width * cam.height)
    assert stats.cpu().numpy().tolist() == [rays, cam.width * cam.height * cam.cam.samples_per_pixel]
    r.close()

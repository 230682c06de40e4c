"""What the occlusion tests share (include/rt.h rt_occluded_rays): the ray sets, the
CPU reference, the sentinel-filled device buffers and one call helper.  A helper module, not a test:
pytest does not rewrite its asserts, so every assert here carries its own message.

The reference is oracle.world_hit(...)[0] >= 0 per ray: HittableList.hit returned true.  The ray sets
that tests/test_gpu_trace.py also uses (the base rays, the 15-interval edge list, the 640 non-finite
rays) are restated here, not imported; every cache key carries the prefix "occ_"."""
import math

import numpy as np
import torch

import rtzig
from gpu_support import DEV, cached

INF, NAN = math.inf, math.nan
N = 4096
BOX_LO, BOX_HI = [-12, .05, -12], [12, 3, 12]
U8_SENTINEL = 0xAB
MASK_SENTINEL = 0x5A5A5A5A5A5A5A5A
EDGE = [(1e-3, INF), (-INF, INF), (1e-3, -1.0), (NAN, INF), (0.0, INF), (-5.0, INF), (1e-3, NAN), (1e-3, 2.0),
        (-INF, 0.0), (1e-300, INF), (1e-3, 1e-300), (INF, INF), (-INF, -INF), (1e-3, 1e300), (-0.0, 0.5)]


# ---- rays ------------------------------------------------------------------------------------------------
def final_cam():
    return cached("occ_final_cam", lambda: rtzig.final_scene_camera(width=48, aspect_ratio=16 / 9, spp=2))


def base_rays():
    def make():
        g = np.random.default_rng(1)
        O = g.uniform(BOX_LO, BOX_HI, (N, 3))
        D = g.standard_normal((N, 3))
        O.setflags(write=False)
        D.setflags(write=False)
        return O, D
    return cached("occ_base_rays", make)


def targets():
    """The end points of the targets-mode case: uniform over the base rays' box."""
    def make():
        B = np.random.default_rng(3).uniform(BOX_LO, BOX_HI, (N, 3))
        B.setflags(write=False)
        return B
    return cached("occ_targets", make)


def ground_rays():
    """Rays leaving points just above the ground (y = 1e-2) toward (0.5, 1, 0.25): only the tree's
    spheres can occlude them."""
    def make():
        O = np.random.default_rng(4).uniform([-11, 0, -11], [11, 0, 11], (N, 3))
        O[:, 1] = 1e-2
        D = np.tile(np.array([0.5, 1.0, 0.25]), (N, 1))
        return O, D
    return cached("occ_ground_rays", make)


def non_finite_rays():
    """640 rays: every component in turn NaN, +inf, -inf (18 kinds, lane by lane), zero directions
    (+0 and -0), all six NaN."""
    O, D = base_rays()
    O, D = O[:640].copy(), D[:640].copy()
    bad = (NAN, INF, -INF)
    for q in range(576):
        (O if q % 6 < 3 else D)[q, q % 3] = bad[(q // 6) % 3]
    D[576:608] = 0.0
    D[592:608, 1] = -0.0
    O[608:640], D[608:640] = NAN, NAN
    return O, D


def intervals_of(n, t_min, t_max):
    iv = np.empty((n, 2))
    iv[:, 0] = t_min
    iv[:, 1] = t_max
    return iv


def edge_intervals(n):
    return np.array([EDGE[q % len(EDGE)] for q in range(n)])


# ---- the reference ---------------------------------------------------------------------------------------
def ref_occluded(oracle, spheres, O, D, iv):
    """(occluded (n,) bool, closest root (n,) f64, inf on a miss) of HittableList.hit per ray."""
    n = len(O)
    occ, t = np.zeros(n, bool), np.full(n, INF)
    for q in range(n):
        k, tq = oracle.world_hit(spheres, O[q].tolist(), D[q].tolist(), float(iv[q, 0]), float(iv[q, 1]))
        if k >= 0:
            occ[q], t[q] = True, tq
    occ.setflags(write=False)
    t.setflags(write=False)
    return occ, t


def base_ref(oracle):
    O, D = base_rays()
    return cached("occ_base_ref", lambda: ref_occluded(oracle, final_cam().scene.world, O, D, intervals_of(N, 1e-3, INF)))


def sphere_hits(oracle, sphere, O, D, t_min, t_max):
    """(n,) bool: this one sphere's own Sphere.hit."""
    return np.array([oracle.sphere_hit(sphere, O[q].tolist(), D[q].tolist(), t_min, t_max) is not None
                     for q in range(len(O))])


def mask_of(occ):
    """The d_mask words of an (n,) bool array: bit q & 63 of word q >> 6, zero past n."""
    pad = np.zeros((len(occ) + 63) // 64 * 64, bool)
    pad[:len(occ)] = occ
    return np.packbits(pad, bitorder="little").view(np.uint64)


# ---- the device ------------------------------------------------------------------------------------------
def strided(A, stride):
    a = np.zeros((len(A), stride or 3))  # stride 0 means 3
    a[:, :3] = A
    if stride > 3:
        a[:, 3:] = NAN  # the padding lane of a Zig @Vector(3, f64) is never read
    return torch.from_numpy(a).to(DEV)


def query(r, O, E, t_min=1e-3, t_max=INF, iv=None, n=None, stride=3, targets=False, outputs=("u8", "mask", "stats")):
    """One rt_occluded_rays call on the default stream over the first n of the rays.  The buffers are
    sized for all of them and pre-filled with sentinels (the stats with 0); returns them whole, as
    dict(u8 (len(O),) uint8, mask (ceil(len(O) / 64),) uint64, stats [rays, scanned, occluded])."""
    n = len(O) if n is None else n
    d_o, d_e = strided(O, stride), strided(E, stride)
    d_iv = torch.from_numpy(np.ascontiguousarray(iv)).to(DEV) if iv is not None else None
    u8 = torch.full((len(O),), U8_SENTINEL, dtype=torch.uint8, device=DEV)
    mask = torch.from_numpy(np.full((len(O) + 63) // 64, MASK_SENTINEL, np.uint64).view(np.int64)).to(DEV)
    stats = torch.zeros(3, dtype=torch.int64, device=DEV)
    r.occluded_rays(d_o.data_ptr(), d_e.data_ptr(), n, t_min, t_max,
                    d_occluded_ptr=u8.data_ptr() if "u8" in outputs else None,
                    d_mask_ptr=mask.data_ptr() if "mask" in outputs else None,
                    d_intervals_ptr=d_iv.data_ptr() if iv is not None else None,
                    d_stats_ptr=stats.data_ptr() if "stats" in outputs else None,
                    ray_stride=stride, targets=targets)
    torch.cuda.synchronize()
    r.sync()  # reports a failure the kernel recorded
    return dict(u8=u8.cpu().numpy(), mask=mask.cpu().numpy().view(np.uint64), stats=stats.cpu().numpy().tolist())


def assert_answers(got, occ, n=None, label=""):
    """u8 and mask equal the reference over the first n rays, and nothing past them was written."""
    n = len(occ) if n is None else n
    words = (n + 63) // 64
    assert np.array_equal(got["u8"][:n], occ[:n].astype(np.uint8)), "%s: u8 differs" % label
    assert (got["u8"][n:] == U8_SENTINEL).all(), "%s: u8 written past the last ray" % label
    assert np.array_equal(got["mask"][:words], mask_of(occ[:n])), "%s: mask differs" % label
    assert (got["mask"][words:] == np.uint64(MASK_SENTINEL)).all(), "%s: mask written past the last word" % label


def trace_hit(r, O, D, t_min=1e-3, t_max=INF, iv=None):
    """rt_trace_rays' index >= 0 for the same rays: the closest-hit call's answer to the same question."""
    d_o, d_d = strided(O, 3), strided(D, 3)
    d_iv = torch.from_numpy(np.ascontiguousarray(iv)).to(DEV) if iv is not None else None
    idx = torch.full((len(O),), -7, dtype=torch.int32, device=DEV)
    r.trace_rays(d_o.data_ptr(), d_d.data_ptr(), len(O), t_min, t_max, d_index_ptr=idx.data_ptr(),
                 d_intervals_ptr=d_iv.data_ptr() if iv is not None else None)
    torch.cuda.synchronize()
    r.sync()
    return idx.cpu().numpy() >= 0

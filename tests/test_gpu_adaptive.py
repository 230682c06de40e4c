"""Adaptive sampling on the GPU (include/rt.h rt_render_pixels_accumulate / rt_accum_select /
rt_accum_resolve_counts).  The contract: after any sequence of gather passes every
pixel is, bit for bit, the pixel of a one-pass render at that pixel's own sample count — the stream
key (seed, pixel, sample) does not depend on spp, and a pixel's colours are added in sample order —
so oracle B at spp = counts[p] checks pixel p.  No tolerances anywhere: the image tests compare bits
against oracle B or the existing GPU paths, the selection against the formula in numpy."""
import numpy as np
import pytest
import torch

import rtzig
from gpu_support import H37 as H
from gpu_support import NPIX37 as NPIX
from gpu_support import W37 as W
from gpu_support import (DEV, FLOOR, MAX_C, MIN_C, SEL_BLOCK, TOL, Bufs, cam37, list_a, list_b, ref37, select_numpy,
                         synthetic, unchanged_outside)
from gpu_support import module_renderers, renderers  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


def expected(oracle, counts):
    """Per pixel, oracle B at that pixel's count (0 where it has none)."""
    out = np.zeros((NPIX, 3))
    for n in np.unique(counts):
        if n:
            out[counts == n] = ref37(oracle, int(n))[0].reshape(NPIX, 3)[counts == n]
    return out


# ---- 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 48])
def test_identity_list_equals_oracle(oracle, n, renderers):
    cam = cam37()
    r = renderers(cam)
    b = Bufs()
    b.add(r, cam, None, n)
    img = b.resolved(r)
    _, _, counts = b.bits()
    r.sync()
    assert "gather" in r.kernel_name() and "bvh" in r.kernel_name()
    r.close()
    ref, rays = ref37(oracle, n)
    assert np.array_equal(img, ref.reshape(NPIX, 3))
    assert (counts == n).all()
    assert b.stats.cpu().tolist() == [rays, NPIX * n]


# ---- 2, 8 ------------------------------------------------------------------------------------------
def sparse_passes(r, cam, b):
    """10 samples for every pixel, 7 more for list A, 5 more for list B; checks after each pass that
    the pixels outside its list kept their bits.  Returns the expected counts."""
    A, B = list_a(), list_b()
    b.add(r, cam, None, 10)
    s0 = b.bits()
    b.add(r, cam, A, 7)
    s1 = b.bits()
    unchanged_outside(s0, s1, A)
    b.add(r, cam, torch.from_numpy(B).to(DEV), 5)  # a device tensor, int64: validated and converted
    s2 = b.bits()
    unchanged_outside(s1, s2, B)
    want = np.full(NPIX, 10)
    want[A] += 7
    want[B] += 5
    assert sorted(np.unique(want)) == [10, 15, 17, 22]
    assert np.array_equal(s2[2], want)
    assert int(b.stats[1]) == NPIX * 10 + len(A) * 7 + len(B) * 5
    return want


def test_sparse_lists_with_uneven_counts(oracle, renderers):
    cam = cam37()
    r = renderers(cam)
    b = Bufs()
    want = sparse_passes(r, cam, b)
    img, rgb = b.resolved(r), b.resolved(r, output="rgb8")
    r.sync()
    r.close()
    ref = expected(oracle, want)
    assert np.array_equal(img, ref)
    assert np.array_equal(rgb, oracle.to_rgb8(ref))


def test_fast_mode(renderers):
    """RT_PRECISION_F32: every pixel is the one-pass fast render's at its count."""
    cam = cam37()
    r = renderers(cam, precision="f32")
    b = Bufs()
    want = sparse_passes(r, cam, b)
    assert "fast_f32" in r.kernel_name() and "gather" in r.kernel_name()
    img = b.resolved(r)
    ref = np.zeros((NPIX, 3))
    one = torch.zeros((NPIX, 3), dtype=torch.float64, device=DEV)
    for n in (10, 15, 17, 22):
        r.render_rows_async(cam37(n).cam, one.data_ptr())
        ref[want == n] = one.cpu().numpy()[want == n]
    r.sync()
    r.close()
    assert np.isfinite(ref).all() and np.array_equal(img, ref)


# ---- 3 ---------------------------------------------------------------------------------------------
def test_list_order_does_not_matter(renderers):
    cam = cam37()
    r = renderers(cam)
    A = np.sort(list_a())
    got = []
    for order in (A, A[::-1].copy(), np.random.default_rng(3).permutation(A)):
        b = Bufs()
        b.add(r, cam, None, 3)
        b.add(r, cam, order, 5)
        got.append(b.bits())
    r.sync()
    r.close()
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert np.array_equal(x, y)
    assert set(np.unique(got[0][2])) == {3, 8}


# ---- 4 ---------------------------------------------------------------------------------------------
def test_runtime_split(oracle, monkeypatch, renderers):
    """A cap of 7 samples of the 740 pixels (and a little): 24 samples run as 7 + 7 + 7 + 3."""
    cam = cam37()
    r = renderers(cam)
    whole = Bufs()
    whole.add(r, cam, None, 24)
    monkeypatch.setenv("RTZIG_GATHER_BYTES", str(NPIX * 24 * 7 + 100))
    split = Bufs()
    r.enable_timing(True)
    split.add(r, cam, None, 24)
    assert r.kernel_times_total()[2] == 4  # four sub-passes, all timed
    r.enable_timing(False)
    for x, y in zip(whole.bits(), split.bits()):
        assert np.array_equal(x, y)
    assert np.array_equal(split.resolved(r), ref37(oracle, 24)[0].reshape(NPIX, 3))
    assert whole.stats.cpu().tolist() == split.stats.cpu().tolist() == [ref37(oracle, 24)[1], NPIX * 24]
    # a sparse list at a cap of exactly one sample of it: 3 sub-passes of 1
    monkeypatch.setenv("RTZIG_GATHER_BYTES", str(250 * 24))
    split.add(r, cam, list_a(), 3)
    want = np.full(NPIX, 24)
    want[list_a()] += 3
    assert np.array_equal(split.resolved(r), expected(oracle, want))
    before = split.bits()
    monkeypatch.setenv("RTZIG_GATHER_BYTES", str(NPIX * 24 - 1))  # below one sample of the list
    with pytest.raises(rtzig.RtError) as e:
        split.add(r, cam, None, 1)
    assert e.value.code == -4
    for x, y in zip(before, split.bits()):
        assert np.array_equal(x, y)
    r.sync()
    r.close()


# ---- 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ring", "direct"])
def test_interoperation_with_row_passes(oracle, mode, monkeypatch, renderers):
    cam = cam37()
    r = renderers(cam)
    b = Bufs(m2=False)  # row passes keep no m2: the gather pass runs without one
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    r.accumulate(cam.cam, b.accum.data_ptr(), 0, 10)
    assert ("direct" in r.kernel_name()) == (mode == "direct")
    b.counts.fill_(10)
    A = list_a()
    b.add(r, cam, A, 6)
    img = b.resolved(r)
    r.sync()
    r.close()
    want = np.full(NPIX, 10)
    want[A] = 16
    assert np.array_equal(b.bits()[2], want)
    assert np.array_equal(img, expected(oracle, want))


# ---- 6 ---------------------------------------------------------------------------------------------
def test_m2_is_bit_exact_and_a_new_pixel_overwrites(oracle, renderers):
    cam = cam37()
    r = renderers(cam)
    # per-sample colours from the existing API: a zeroed accumulator and one sample (0 + c is exact)
    cols = np.zeros((12, NPIX, 3))
    one = torch.empty((NPIX, 3), dtype=torch.float64, device=DEV)
    for s in range(12):
        one.zero_()
        r.accumulate(cam.cam, one.data_ptr(), s, 1)
        cols[s] = one.cpu().numpy()
    A = list_a()
    b = Bufs(fill=float("nan"))  # counts 0: the NaNs must be overwritten, never read
    nan_bits = b.bits()
    for count in (4, 3, 5):
        b.add(r, cam, A, count)
    acc, m2, counts = b.bits()
    img = b.resolved(r)
    r.sync()
    r.close()
    sums, msq = np.zeros((NPIX, 3)), np.zeros(NPIX)
    for s in range(12):  # the stated order: y = (r + g) + b, m2 += y * y, sample by sample
        sums = sums + cols[s]
        y = (cols[s][:, 0] + cols[s][:, 1]) + cols[s][:, 2]
        msq = msq + y * y
    assert np.array_equal(acc[A], sums.view(np.int64)[A])
    assert np.array_equal(m2[A], msq.view(np.int64)[A])
    assert (msq[A] > 0).all()
    want = np.zeros(NPIX, np.int64)
    want[A] = 12
    assert np.array_equal(counts, want)
    unchanged_outside(nan_bits, (acc, m2, counts), A)
    assert np.array_equal(img, expected(oracle, want))  # 0 where a pixel has no sample


# ---- 7 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def select_renderer(module_renderers):
    return module_renderers()


@pytest.mark.parametrize("n", [1, 63, 64, 65, NPIX, 3 * SEL_BLOCK + 17])
@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "single-last", "below-min", "at-max", "v-negative",
                                     "nan-m2", "random"])
def test_select_against_numpy(select_renderer, pattern, n):
    r = select_renderer
    accum, m2, counts = synthetic(pattern, n)
    want, want_err = select_numpy(accum, m2, counts)
    d_accum, d_m2 = torch.from_numpy(accum).to(DEV), torch.from_numpy(m2).to(DEV)
    d_counts = torch.from_numpy(counts.astype(np.int32)).to(DEV)
    d_list = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_n = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    d_err = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
    for err_ptr in (d_err.data_ptr(), None):  # d_err is optional
        r.select(d_accum.data_ptr(), d_m2.data_ptr(), d_counts.data_ptr(), n, MIN_C, MAX_C, TOL, FLOOR, d_list.data_ptr(),
                 d_n.data_ptr(), d_err_ptr=err_ptr)
        k = int(d_n.item())
        assert k == len(want)
        assert np.array_equal(d_list[:k].cpu().numpy(), want)  # ascending, as numpy lists them
        d_n.fill_(-1)
    got_err = d_err.cpu().numpy()
    # bit-equal to the formula; a NaN (from a NaN m2) compares as NaN: IEEE leaves its payload open
    nan = np.isnan(want_err)
    assert np.array_equal(np.isnan(got_err), nan)
    assert np.array_equal(got_err[~nan].view(np.int64), want_err[~nan].view(np.int64))
    if pattern == "none":
        assert len(want) == 0
    if pattern == "all":
        assert len(want) == n
    if pattern == "single-last":
        assert want.tolist() == [n - 1]
    if pattern == "v-negative":
        assert (want_err == 0).all() and len(want) == 0
    assert r.workspace_bytes() >= 4 * ((n + SEL_BLOCK - 1) // SEL_BLOCK) + 8 * ((n + 63) // 64)


# ---- 9 ---------------------------------------------------------------------------------------------
def test_render_adaptive_end_to_end(oracle):
    """min 8, step 8, max 64 at tolerance 0.08 (floor 0.01).  The tolerance comes from a CPU replay of
    the loop on oracle B's images at spp 1..64 (per-sample colours as differences of the unscaled
    sums): it ended with 235 / 35 / 56 / 50 / 28 / 36 / 42 / 258 pixels at 8 / 16 / ... / 64 samples,
    so the run is far from degenerate."""
    cam = cam37()
    rounds = []

    def on_round(rnd, lst, accum, m2, counts):
        assert rnd == len(rounds)
        c = counts.cpu().numpy().astype(np.int64)
        a, m = accum.cpu().numpy(), m2.cpu().numpy()
        with np.errstate(all="ignore"):
            n = c.astype(np.float64)
            S = (a[:, 0] + a[:, 1]) + a[:, 2]
            mean = S / n
            v = m - S * mean
            v = np.where(v < 0, 0.0, v)
            err = np.sqrt((v / (n - 1)) / n) / np.where(mean > 0.01, mean, 0.01)
            sel = (c < 8) | ((c < 64) & ~(err <= 0.08))
        assert np.array_equal(lst.cpu().numpy(), np.flatnonzero(sel))
        rounds.append(len(lst))

    img, counts = rtzig.render_adaptive(cam.cam, cam.scene.world, 8, 64, 8, 0.08, floor=0.01, on_round=on_round)
    assert img.shape == (H, W, 3) and counts.shape == (H, W) and counts.dtype == np.uint32
    assert rounds[-1] == 0 and all(k > 0 for k in rounds[:-1]) and len(rounds) >= 2
    c = counts.reshape(-1).astype(np.int64)
    assert ((c % 8 == 0) & (c >= 8) & (c <= 64)).all()
    assert len(np.unique(c)) >= 3, np.unique(c, return_counts=True)
    assert np.array_equal(img.reshape(NPIX, 3), expected(oracle, c))
    ppm, counts2 = cam.render_adaptive(8, 64, 8, 0.08, floor=0.01, output="rgb8")
    assert np.array_equal(counts2, counts)
    assert np.array_equal(ppm.pixels, oracle.to_rgb8(img))
    img3, counts3 = rtzig.render_adaptive(cam.cam, cam.scene.world, 8, 64, 8, 0.08, floor=0.01)
    assert np.array_equal(img3, img) and np.array_equal(counts3, counts)


# ---- the list walk, arguments ----------------------------------------------------------------------
def test_chapter13_list_walk(oracle, renderers):
    """5 spheres: the reference's list walk, geometry in LDS (the gather twin of lds_u4)."""
    def cam13(spp):
        return rtzig.chapter13_camera(width=W, aspect_ratio=16 / 9, spp=spp)
    cam = cam13(1)
    assert cam.width * cam.height == NPIX
    r = renderers(cam)
    b = Bufs()
    A = list_a()
    b.add(r, cam, None, 5)
    b.add(r, cam, A, 4)
    assert r.kernel_name() == "lds_u4(gather)"
    img = b.resolved(r)
    r.sync()
    r.close()
    ref = {n: oracle.render_b(cam13(n).cam, cam.scene.world, threads=16) for n in (5, 9)}
    want = ref[5][0].reshape(NPIX, 3).copy()
    want[A] = ref[9][0].reshape(NPIX, 3)[A]
    assert np.array_equal(img, want)
    assert int(b.stats[1]) == NPIX * 5 + len(A) * 4


def test_arguments(renderers):
    cam = cam37()
    r = renderers(cam)
    b = Bufs(fill=7.0)
    before = b.bits()
    b.add(r, cam, None, 0)                      # no samples: OK, nothing touched
    b.add(r, cam, np.zeros(0, np.int64), 3)     # an empty list: the same
    for bad in ([0, 740], [-1], [5, 9, 5]):     # out of range, negative, twice: refused on the host
        with pytest.raises(ValueError):
            b.add(r, cam, bad, 1)
    with pytest.raises(rtzig.RtError) as e:     # a NULL list is the whole image
        r.accumulate_pixels(cam.cam, None, 1, b.accum.data_ptr(), None, b.counts.data_ptr(), n_pixels=739)
    assert e.value.code == -1
    r.enable_profile(True)
    with pytest.raises(rtzig.RtError) as e:     # no instrumented gather kernel
        b.add(r, cam, None, 1)
    assert e.value.code == -1 and "instrumented" in str(e.value)
    r.enable_profile(False)
    out = torch.empty((NPIX, 3), dtype=torch.float64, device=DEV)
    with pytest.raises(rtzig.RtError) as e:
        r.resolve_counts(b.accum.data_ptr(), None, NPIX, out.data_ptr())
    assert e.value.code == -1
    for x, y in zip(before, b.bits()):
        assert np.array_equal(x, y)
    r.sync()
    r.close()

"""Progressive rendering on the GPU (include/rt.h rt_render_rows_accumulate / rt_accum_resolve,
DESIGN.md §5.7): samples [a, b) added onto the stored unscaled sums of samples [0, a) and scaled by
1/b are, bit for bit, the one-pass render at spp = b — the reference adds a pixel's samples strictly
in sample order and scales once (camera.zig:133-137), and the stream key (seed, pixel, sample) does
not depend on spp.  So oracle B at spp = samples_done checks every intermediate image."""
import numpy as np
import pytest
import torch

import rtzig
from gpu_support import DEV, cam37, ref37
from gpu_support import renderers  # noqa: F401 (fixture)
from rtzig.abi import RT_PROFILE_STATS_WORDS

pytestmark = pytest.mark.gpu

MODES = ["ring", "direct"]


def new_accum(n_pixels, fill=None):
    a = torch.empty((n_pixels, 3), dtype=torch.float64, device=DEV)
    if fill is not None:
        a.fill_(fill)
    return a


def resolved(r, accum, shape, n_samples, output="linear", stream_ptr=None):
    out = torch.empty(shape + (3,), dtype=torch.float64 if output == "linear" else torch.uint8, device=DEV)
    r.resolve(accum.data_ptr(), shape[0] * shape[1], n_samples, out.data_ptr(), output=output, stream_ptr=stream_ptr)
    return out


def accumulate_all(r, cam, accum, split, stats=None, **rows):
    done = 0
    for count in split:
        r.accumulate(cam.cam, accum.data_ptr(), done, count, d_stats_ptr=stats.data_ptr() if stats is not None else None,
                     **rows)
        done += count
    return done


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("split", [[100], [1, 99], [48, 52], [49, 1, 50], [17] * 5 + [15]], ids=lambda s: "-".join(map(str, s)))
def test_every_prefix_equals_oracle_every_split_equals_one_pass(oracle, split, mode, monkeypatch, renderers):
    """Each pass's resolved image is oracle B at spp = samples_done; the last one is also the
    one-pass render at spp 100, its RGB8 resolve is Color.toRgb of it, and the passes' ray and
    sample counts sum to the one-pass counts."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = cam37(100)
    H, W = cam.height, cam.width
    assert (H, W) == (20, 37)
    r = renderers(cam)
    accum = new_accum(H * W)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    done = 0
    for count in split:
        r.accumulate(cam.cam, accum.data_ptr(), done, count, d_stats_ptr=stats.data_ptr())
        done += count
        img = resolved(r, accum, (H, W), done).cpu().numpy()
        assert np.array_equal(img, ref37(oracle, done)[0]), (split, done)
        assert ("direct" in r.kernel_name()) == (mode == "direct")
    assert done == 100
    rgb = resolved(r, accum, (H, W), 100, output="rgb8").cpu().numpy()
    r.sync()
    r.close()
    ref, rays = ref37(oracle, 100)
    assert np.array_equal(img, rtzig.render(cam.cam, cam.scene.world, n_gpus=1))
    assert np.array_equal(rgb, oracle.to_rgb8(ref))
    st = stats.cpu().tolist()
    assert st[0] == rays and st[1] == 740 * 100


@pytest.mark.parametrize("split", [[150, 150], [1, 299]], ids=lambda s: "-".join(map(str, s)))
def test_seeded_sum_through_a_handoff_chain(oracle, split, monkeypatch, renderers):
    """One tile, many chunks per pass (test_running_sum_handoff_chains), ring mode forced: chunk 0 of
    the second pass takes the stored sum and every later chunk waits on the tile's flag."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", "ring")
    cam = (rtzig.Camera.builder(8, 1.0).setScene(rtzig.Scene.init(0x5eed).generateWorld())
           .setDefocusAngle(0.6).setFocusDist(10).setViewport((13, 2, 3), (0, 0, 0), 20)
           .setSamplesPerPixel(300).build())
    r = renderers(cam)
    accum = new_accum(64)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    assert accumulate_all(r, cam, accum, split, stats) == 300
    img = resolved(r, accum, (8, 8), 300).cpu().numpy()
    r.sync()
    assert "direct" not in r.kernel_name()
    r.close()
    ref, rays = oracle.render_b(cam.cam, cam.scene.world, threads=16)
    assert np.array_equal(img, ref)
    assert stats.cpu().tolist() == [rays, 64 * 300]


@pytest.mark.parametrize("mode", MODES)
def test_new_image_overwrites_continuation_reads(oracle, mode, monkeypatch, renderers):
    """sample_begin = 0 ignores what the accumulator held (NaN here; any sum would keep it)."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = cam37(100)
    r = renderers(cam)
    accum = new_accum(740, fill=float("nan"))
    accumulate_all(r, cam, accum, [60, 40])
    img = resolved(r, accum, (20, 37), 100).cpu().numpy()
    r.sync()
    r.close()
    assert np.array_equal(img, ref37(oracle, 100)[0])


@pytest.mark.parametrize("order", [("direct", "ring"), ("ring", "direct")], ids=lambda o: "-".join(o))
def test_modes_may_change_between_passes(oracle, order, monkeypatch, renderers):
    """The accumulator is the same plain data in both modes: one pass in each on one buffer."""
    cam = cam37(100)
    r = renderers(cam)
    accum = new_accum(740)
    done = 0
    for mode, count in zip(order, [48, 52]):
        monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
        r.accumulate(cam.cam, accum.data_ptr(), done, count)
        assert ("direct" in r.kernel_name()) == (mode == "direct")
        done += count
    img = resolved(r, accum, (20, 37), 100).cpu().numpy()
    r.sync()
    r.close()
    assert np.array_equal(img, ref37(oracle, 100)[0])


@pytest.mark.parametrize("mode", MODES)
def test_row_subsets(oracle, mode, monkeypatch, renderers):
    """Rows 1, 4, 7, ... into an accumulator of n_rows x W pixels."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = cam37(7)
    n_rows = len(range(1, 20, 3))
    r = renderers(cam)
    accum = new_accum(n_rows * 37)
    accumulate_all(r, cam, accum, [3, 4], row0=1, row_step=3, n_rows=n_rows)
    img = resolved(r, accum, (n_rows, 37), 7).cpu().numpy()
    r.sync()
    r.close()
    assert np.array_equal(img, rtzig.render(cam.cam, cam.scene.world, n_gpus=1)[1::3])
    assert np.array_equal(img, ref37(oracle, 7)[0][1::3])


@pytest.mark.parametrize("mode", MODES)
def test_no_host_sync_between_passes(oracle, mode, monkeypatch, renderers):
    """Four passes and the resolve back to back on one non-default stream, one synchronize at the
    end: the accumulator is ordered across the launches by the stream alone."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = cam37(100)
    r = renderers(cam)
    accum = new_accum(740)
    out = torch.empty((20, 37, 3), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()  # the allocations; nothing below waits on the host until the end
    s = torch.cuda.Stream()
    for k in range(4):
        r.accumulate(cam.cam, accum.data_ptr(), 25 * k, 25, stream_ptr=s.cuda_stream)
    r.resolve(accum.data_ptr(), 740, 100, out.data_ptr(), stream_ptr=s.cuda_stream)
    s.synchronize()
    img = out.cpu().numpy()
    r.sync()
    r.close()
    assert np.array_equal(img, ref37(oracle, 100)[0])


def test_after_a_pending_deferred_call(oracle, monkeypatch, renderers):
    """An accumulate pass is a plain call: it first runs the reduce pass a deferred call left
    pending, whose output is then complete on that call's out stream."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", "direct")
    cam = cam37(100)
    r = renderers(cam)
    frame = torch.zeros((20, 37, 3), dtype=torch.float64, device=DEV)
    accum = new_accum(740)
    torch.cuda.synchronize()
    render, coll = torch.cuda.Stream(), torch.cuda.Stream()
    r.render_rows_async(cam.cam, frame.data_ptr(), stream_ptr=render.cuda_stream, out_stream_ptr=coll.cuda_stream,
                        deferred=True)
    assert r.fold_pending()
    r.accumulate(cam.cam, accum.data_ptr(), 0, 100, stream_ptr=render.cuda_stream)
    assert not r.fold_pending()
    with torch.cuda.stream(coll):
        got = frame.clone()  # ordered after the deferred frame's output
    img = resolved(r, accum, (20, 37), 100, stream_ptr=render.cuda_stream)
    torch.cuda.synchronize()
    r.sync()
    r.close()
    ref = ref37(oracle, 100)[0]
    assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(img.cpu().numpy(), ref)


@pytest.mark.parametrize("mode", MODES)
def test_fast_mode(mode, monkeypatch, renderers):
    """RT_PRECISION_F32: the passes resolve to the one-pass fast render's bits."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = rtzig.final_scene_camera(width=120, aspect_ratio=1.5, spp=16)
    H, W = cam.height, cam.width
    r = renderers(cam, precision="f32")
    one = torch.zeros((H, W, 3), dtype=torch.float64, device=DEV)
    st1 = torch.zeros(2, dtype=torch.int64, device=DEV)
    r.render_rows_async(cam.cam, one.data_ptr(), d_stats_ptr=st1.data_ptr())
    accum = new_accum(H * W)
    st2 = torch.zeros(2, dtype=torch.int64, device=DEV)
    accumulate_all(r, cam, accum, [5, 11], st2)
    assert "fast_f32" in r.kernel_name()
    img = resolved(r, accum, (H, W), 16)
    torch.cuda.synchronize()
    r.sync()
    r.close()
    assert torch.isfinite(one).all() and torch.equal(img, one)
    assert st1.cpu().tolist() == st2.cpu().tolist() and int(st2[1]) == H * W * 16


@pytest.mark.parametrize("mode", MODES)
def test_instrumented_context(oracle, mode, monkeypatch, renderers):
    """The instrumented kernels (72-word stats) accumulate the same bits; words 0-1 of the passes
    sum to the one-pass counts."""
    monkeypatch.setenv("RTZIG_UNIT_MODE", mode)
    cam = cam37(7)
    r = renderers(cam, profile=True)
    accum = new_accum(740)
    stats = torch.zeros(RT_PROFILE_STATS_WORDS, dtype=torch.int64, device=DEV)
    accumulate_all(r, cam, accum, [3, 4], stats)
    assert "prof" in r.kernel_name()
    img = resolved(r, accum, (20, 37), 7).cpu().numpy()
    r.sync()
    r.close()
    ref, rays = ref37(oracle, 7)
    assert np.array_equal(img, ref)
    st = stats.cpu().tolist()
    assert st[0] == rays and st[1] == 740 * 7


def test_arguments(renderers):
    cam = cam37(4)
    r = renderers(cam)
    accum = new_accum(740, fill=7.0)
    torch.cuda.synchronize()
    r.accumulate(cam.cam, accum.data_ptr(), 5, 0)  # no samples: OK, nothing touched
    r.accumulate(cam.cam, accum.data_ptr(), 0, 3, n_rows=0)  # no rows: the same
    with pytest.raises(rtzig.RtError) as e:
        r.accumulate(cam.cam, accum.data_ptr(), 2 ** 32 - 2, 2)
    assert e.value.code == -1
    with pytest.raises(rtzig.RtError) as e:
        r.accumulate(cam.cam, None, 0, 1)
    assert e.value.code == -1
    with pytest.raises(rtzig.RtError) as e:
        r.accumulate(cam.cam, accum.data_ptr(), 0, 1, row0=19, n_rows=2)  # past the image
    assert e.value.code == -1
    r.sync()
    torch.cuda.synchronize()
    assert bool((accum == 7.0).all())
    r.accumulate(cam.cam, accum.data_ptr(), 2 ** 32 - 3, 2)  # the last admissible samples
    r.sync()
    r.close()
    assert bool(torch.isfinite(accum).all()) and not bool((accum == 7.0).all())


def test_generator():
    cam = cam37(10)
    items = list(rtzig.render_progressive(cam.cam, cam.scene.world, [2, 3, 5]))
    assert [n for n, _ in items] == [2, 5, 10]
    assert np.array_equal(items[-1][1], rtzig.render(cam.cam, cam.scene.world, n_gpus=1))
    ppm = list(cam.render_progressive([4, 6], output="rgb8"))[-1]
    assert ppm[0] == 10 and np.array_equal(ppm[1].pixels, rtzig.to_rgb8(items[-1][1]))

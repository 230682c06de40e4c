"""Every GPU config at its full image size, through size-independent properties (the
oracle checks crops of these in test_gpu_configs.py; a full frame would take it minutes):

* row-partition invariance: the full frame (one launch; ring mode) equals, row for row, the 8
  interleaved row sets an 8-GPU job renders (rows r, r + 8, ...; direct mode for configs 3 and 4,
  whose row sets store 1.2-1.4 GB of samples, ring mode for config 5's) — the
  RNG is keyed by the global pixel and both modes add every pixel's samples in sample order, so not
  one bit may change;
* exact sample counts and finite, in-range output (linear f64 in [0, 1] before the scale).
"""
import pytest
import torch

import rtzig
from gpu_support import renderers  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def _partition_check(make, cam, n_parts=8):
    H, W = cam.height, cam.width
    spp = cam.cam.samples_per_pixel
    r = make(cam)
    full = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    st = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    r.render_rows_async(cam.cam, full.data_ptr(), d_stats_ptr=st.data_ptr())
    r.sync()
    assert int(st[1]) == H * W * spp
    for part in range(n_parts):
        n = (H - part + n_parts - 1) // n_parts
        buf = torch.zeros((n, W, 3), dtype=torch.float64, device="cuda:0")
        r.render_rows_async(cam.cam, buf.data_ptr(), row0=part, row_step=n_parts, n_rows=n)
        r.sync()
        assert torch.equal(full[part::n_parts], buf), f"row set {part}::{n_parts} differs"
    assert torch.isfinite(full).all() and (full >= 0).all() and (full <= 1).all()
    r.close()


def test_config4_full_frame_partition_invariant(renderers):
    """Config 4, the bench workload: 1200x800, 500 spp, 485 spheres."""
    _partition_check(renderers, rtzig.final_scene_camera(width=1200, aspect_ratio=1.5, spp=500))


def test_config3_full_frame_partition_invariant(renderers):
    """Config 3: chapter 13 scene, 1200x675, 500 spp."""
    _partition_check(renderers, rtzig.chapter13_camera(width=1200, spp=500))


def test_config5_full_image_partition_invariant(renderers):
    """Config 5's image, 3840x2160, at 200 of its 10000 spp (its full spp is one 9.7-s launch, run by
    tools/configs_bench.py; config 5's row at 10000 spp is checked against the oracle in
    test_gpu_configs.py)."""
    _partition_check(renderers, rtzig.final_scene_camera(width=3840, aspect_ratio=16 / 9, spp=200))

"""bench.py's plain and --full runs, and --dump-outputs.

A plain run times its steps and prints the line; the side measurements (`roofline`, `fast_f32`,
`dropin_ms`, `cpu_baseline`) appear only with --full.  --dump-outputs writes the last timed step's
frame (reference: the framebuffer Camera.render fills, camera.zig:125,138), which must equal the
drop-in render of the same scene bit for bit in either mode.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, ASPECT, SPP = 96, 16 / 9, 4


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=110, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return lines[0]


def test_bench_full_and_dump_options_parse():
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d", "--steps", "3", "--warmup", "0"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 3 and a.warmup == 0
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--dump-outputs"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


@pytest.fixture(scope="module")
def whole_frame():
    import rtzig
    cam = rtzig.final_scene_camera(width=W, aspect_ratio=ASPECT, spp=SPP)
    return rtzig.render(cam.cam, cam.scene.world, n_gpus=1, device=0)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_bench_dump_outputs_is_the_timed_frame(tmp_path, whole_frame, full):
    steps = 3
    args = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--width", str(W), "--aspect", repr(ASPECT),
            "--spp", str(SPP), "--dump-outputs", str(tmp_path / "out")]
    # --full: the fast-mode frames render into the row buffers after the timed steps; the dump must
    # still be the last timed (f64 parity) frame.  The CPU baseline and the one-shot child processes
    # are the slow legs and have tests of their own.
    line = _bench(args + (["--full", "--no-cpu-baseline", "--no-dropin"] if full else []))
    assert line["steps"] == steps and line["full"] is full and line["dtype"] == "f64"
    H = line["config"]["height"]
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(W * H * SPP / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert "dropin_ms" not in line and line["cpu_baseline"] is None
    if full:
        assert line["roofline"]["kernel"] and line["fast_f32"]["dtype"] == "f32"
    else:
        assert line["roofline"] is None and line["fast_f32"] is None
    assert os.listdir(tmp_path / "out") == ["image.npy"]
    img = np.load(tmp_path / "out" / "image.npy")
    assert img.dtype == np.float64 and img.shape == (H, W, 3) == whole_frame.shape
    assert np.array_equal(img, whole_frame)

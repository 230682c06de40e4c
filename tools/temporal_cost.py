"""What rt_temporal_accumulate costs and what it buys.

cost.json: on config 4's image (1200x800, final scene, 485 spheres), the buffers of two cameras a small
step apart, each from a 16-sample every-pixel gather pass and a 4-sample feature pass.  Kernel time of
the call from the context's own events (rt_context_kernel_times) against its yardstick — rt_denoise at
its default levels on the same buffers — the two alternating in one run, medians of --reps after a
warm-up; the current frame's sums are restored before every call, so every call merges the same data.
The bar: no dearer than the yardstick's median plus the yardstick's own min-max spread.

quality.json: a --frames camera path (a translation of about one pixel per frame) over config 4's scene at
--width, at each of --path-samples samples per frame: RMSE per frame against a --ref-spp render of that frame's camera
with a seed of its own, of the denoised and of the merged noisy image, with the temporal pass off and on at
max_history 16 / 64 / 256.  The same for a chapter-13 path (metal and glass: view-dependent surfaces, where
reprojected history lags), which is recorded, not judged.
    python tools/temporal_cost.py --out-dir profiles/temporal"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracing-with-zig_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtzig  # noqa: E402
from rtzig.abi import RtCamera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=16)
ap.add_argument("--feature-samples", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--width", type=int, default=300)
ap.add_argument("--path-samples", type=int, nargs="+", default=[4, 16])
ap.add_argument("--ref-spp", type=int, default=512)
ap.add_argument("--out-dir", default=None)
a = ap.parse_args()
assert a.reps >= 5

DEV = "cuda:0"


def final_camera(scene, width, step):
    """Config 4's camera moved `step` units along z (look-from and look-at alike: a translation)."""
    return (rtzig.Camera.builder(width, 1.5).setScene(scene).setDefocusAngle(0.6).setFocusDist(10)
            .setViewport((13, 2, 3 + step), (0, 0, step), 20).setSamplesPerPixel(1).build().cam)


def med(v):
    return round(statistics.median(v), 4)


# ---- cost ---------------------------------------------------------------------------------------------
base = rtzig.final_scene_camera(width=1200, aspect_ratio=1.5, spp=1)
scene = base.scene
cams = [final_camera(scene, 1200, 0.0), final_camera(scene, 1200, 0.006)]  # about one pixel at the focus distance
cams[1].seed = cams[0].seed + 1
W, H = cams[0].image_width, cams[0].image_height
P = W * H
r = rtzig.DeviceRenderer(0)
r.set_scene(scene.world)
r.enable_timing(True)
stream = torch.cuda.Stream()
sp = stream.cuda_stream


def buffers():
    return dict(accum=torch.empty((P, 3), dtype=torch.float64, device=DEV), m2=torch.empty(P, dtype=torch.float64, device=DEV),
                counts=torch.zeros(P, dtype=torch.int32, device=DEV), albedo=torch.empty((P, 3), dtype=torch.float64, device=DEV),
                normal=torch.empty((P, 3), dtype=torch.float64, device=DEV), depth=torch.empty(P, dtype=torch.float64, device=DEV),
                hits=torch.empty(P, dtype=torch.int32, device=DEV))


sets = [buffers(), buffers()]  # [0]: the previous frame, [1]: the current one
ptrs = [dict({k: v.data_ptr() for k, v in s.items()}, feature_samples=a.feature_samples) for s in sets]
hist = torch.zeros(P, dtype=torch.int32, device=DEV)
out = torch.empty((P, 3), dtype=torch.float64, device=DEV)
var = torch.empty(P, dtype=torch.float64, device=DEV)
torch.cuda.synchronize()
for c, d in zip(cams, ptrs):
    r.accumulate_pixels(c, None, a.samples, d["accum"], d["m2"], d["counts"], stream_ptr=sp)
    r.features(c, 0, a.feature_samples, d["albedo"], d["normal"], d["depth"], d["hits"], stream_ptr=sp)
stream.synchronize()
fresh = {k: sets[1][k].clone() for k in ("accum", "m2", "counts")}


def temporal():
    with torch.cuda.stream(stream):
        for k, v in fresh.items():
            sets[1][k].copy_(v)
    r.temporal_accumulate(cams[1], ptrs[1], cams[0], ptrs[0], d_history_ptr=hist.data_ptr(), stream_ptr=sp)
    s, d = r.kernel_times()
    return s + d


def denoise():
    d = ptrs[1]
    r.denoise(W, H, d["accum"], d["m2"], d["counts"], out.data_ptr(), d_albedo_ptr=d["albedo"], d_normal_ptr=d["normal"],
              d_depth_ptr=d["depth"], d_hits_ptr=d["hits"], feature_samples=a.feature_samples, d_var_out_ptr=var.data_ptr(),
              stream_ptr=sp)
    s, dd = r.kernel_times()
    return s + dd


for _ in range(2):  # warm-up
    temporal(), denoise()
y, t = [], []
for _ in range(a.reps):  # alternating
    y.append(denoise())
    t.append(temporal())
stream.synchronize()
first = {k: sets[1][k].clone() for k in fresh}
h = hist.cpu().numpy().view(np.uint32)
hit = sets[1]["hits"].cpu().numpy() > 0
temporal()
stream.synchronize()
spread = max(y) - min(y)
# bytes the call moves when every tap is read once: both frames' records (accum 24, m2 8, counts 4, albedo 24,
# normal 24, depth 8, hits 4 = 96 B) read, the current sums written back (36 B), history written (4 B)
bytes_per_pixel = 96 + 96 + 36 + 4
cost = {
    "image": f"{W}x{H}", "spheres": len(scene.world), "samples": a.samples, "feature_samples": a.feature_samples,
    "reps": a.reps, "camera_step": 0.006,
    "yardstick": "rt_denoise at its default levels (%d)" % rtzig.denoise_params().levels,
    "yardstick_ms": [round(x, 4) for x in y], "yardstick_median_ms": med(y), "yardstick_spread_ms": round(spread, 4),
    "temporal_ms": [round(x, 4) for x in t], "temporal_median_ms": med(t),
    "temporal_over_yardstick": round(statistics.median(t) / statistics.median(y), 4),
    "bar_ms": round(statistics.median(y) + spread, 4),
    "meets_bar": statistics.median(t) <= statistics.median(y) + spread,
    "bytes_per_pixel": bytes_per_pixel,
    "effective_GBps": round(bytes_per_pixel * P / (statistics.median(t) * 1e-3) / 1e9, 1),
    "hit_pixels": int(hit.sum()), "hit_pixels_with_history": int((h[hit] > 0).sum()),
    "two_runs_bit_equal": all(bool(torch.equal(first[k].view(torch.uint8), sets[1][k].view(torch.uint8))) for k in first),
}
print(json.dumps(cost), file=sys.stderr, flush=True)
r.sync()
r.close()
del sets, fresh, first, out, var, hist


# ---- quality ------------------------------------------------------------------------------------------
def rmse(x, ref):
    return round(float(np.sqrt(np.mean((np.asarray(x, np.float64) - ref) ** 2))), 6)


def reference(cam, world, f):
    c = RtCamera.from_buffer_copy(cam)
    c.samples_per_pixel, c.pixel_samples_scale = a.ref_spp, 1.0 / a.ref_spp
    c.seed = cam.seed + 0x1000 + f  # shares no sample with the frames it judges
    return rtzig.render(c, world, n_gpus=1)


def table(path, world, refs, spp):
    rows = {}
    variants = [("off", False)] + [("max_history_%d" % n, rtzig.temporal_params(max_history=n)) for n in (16, 64, 256)]
    for name, temporal_arg in variants:
        frames = list(rtzig.render_sequence(path, world, spp, feature_spp=a.feature_samples, temporal=temporal_arg))
        rows[name] = {"denoised": [rmse(fr["image"], refs[f]) for f, fr in enumerate(frames)],
                      "noisy": [rmse(fr["noisy"], refs[f]) for f, fr in enumerate(frames)],
                      "mean_history": [round(float(fr["history"].mean()), 2) for fr in frames],
                      "pixels_with_history": [round(float((fr["history"] > 0).mean()), 4) for fr in frames]}
        print(json.dumps({name: rows[name]["denoised"]}), file=sys.stderr, flush=True)
    tail = slice(len(path) // 2, None)  # the steady half of the path
    return {"rmse_per_frame": rows,
            "rmse_mean_second_half": {n: {k: round(statistics.mean(v[k][tail]), 6) for k in ("denoised", "noisy")}
                                      for n, v in rows.items()}}


wq = a.width
step = 0.006 * 1200 / wq  # about one pixel per frame at this width
final_path = [final_camera(scene, wq, step * f) for f in range(a.frames)]
ch13 = rtzig.chapter13_camera(width=wq, aspect_ratio=16 / 9, spp=1)
s13 = ch13.scene
# chapter 13: 20 degrees over wq * 9 / 16 rows, the spheres about 3.4 units away
step13 = 3.4 * np.radians(20.0) / (wq * 9 / 16)
ch13_path = [(rtzig.Camera.builder(wq, 16 / 9).setScene(s13).setDefocusAngle(10.0).setFocusDist(3.4)
              .setViewport((-2 + step13 * f, 2, 1), (step13 * f, 0, -1), 20).setSamplesPerPixel(1).build().cam)
             for f in range(a.frames)]
final_refs = [reference(c, scene.world, f) for f, c in enumerate(final_path)]
ch13_refs = [reference(c, s13.world, f) for f, c in enumerate(ch13_path)]
quality = {
    "frames": a.frames, "samples_per_frame": a.path_samples, "feature_samples": a.feature_samples, "reference_spp": a.ref_spp,
    "final_scene": dict(image=f"{final_path[0].image_width}x{final_path[0].image_height}", camera_step=round(step, 5),
                        **{"spp_%d" % n: table(final_path, scene.world, final_refs, n) for n in a.path_samples}),
    "chapter13_moving_recorded_not_judged": dict(image=f"{ch13_path[0].image_width}x{ch13_path[0].image_height}",
                                                 camera_step=round(float(step13), 5),
                                                 **{"spp_%d" % n: table(ch13_path, s13.world, ch13_refs, n) for n in a.path_samples}),
}
if a.out_dir:
    os.makedirs(a.out_dir, exist_ok=True)
    for name, obj in (("cost.json", cost), ("quality.json", quality)):
        with open(os.path.join(a.out_dir, name), "w") as f:
            f.write(json.dumps(obj, indent=1) + "\n")
print(json.dumps({"cost": cost, "quality": quality}, indent=1))  # one object: the two files' contents

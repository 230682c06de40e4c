"""What rt_denoise costs and what it buys, on config 4's image (1200x800, final scene,
485 spheres).  The buffers come from a 16-sample every-pixel gather pass and a 4-sample feature pass.

cost.json: kernel time of the whole call at 5 levels (and at the default level count) against its yardstick — the
16-sample every-pixel gather pass itself, sample + reduce: a denoiser dearer than the samples it
stands in for has no case — from the context's own events (rt_context_kernel_times), the two
alternating in one run, medians of --reps after a warm-up.  The context times a call as a whole, so the
stages come from calls of 0 .. 6 levels: levels == 0 is prepare + prefilter, level k the difference of
the calls with k + 1 and k levels; with RTZIG_DENOISE_FORM forcing the tile and the direct form in turn
that is also the A/B per level which chose the default form of each step.

quality.json: RMSE against the 500-spp frame of the noisy 16-spp image, of the denoised image at
1 .. 6 levels and of plain 32- and 64-spp renders, for --seeds camera seeds on the same world (a render
is deterministic, so the seeds are the table's run-to-run spread); the reference frame has a seed of
its own, so it shares no sample with the images it judges.
    python tools/denoise_cost.py --out-dir profiles/denoise"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracing-with-zig_amd"))
import torch  # noqa: E402

import rtzig  # noqa: E402
from rtzig.abi import RtCamera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=16)
ap.add_argument("--feature-samples", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--ref-spp", type=int, default=500)
ap.add_argument("--seeds", type=int, default=3)
ap.add_argument("--max-levels", type=int, default=6)
ap.add_argument("--out-dir", default=None)
a = ap.parse_args()
assert a.reps >= 5

DEV = "cuda:0"
cam = rtzig.final_scene_camera(width=1200, aspect_ratio=1.5, spp=1)
H, W = cam.height, cam.width
P = H * W
r = rtzig.DeviceRenderer(0)
r.set_scene(cam.scene.world)
r.enable_timing(True)
stream = torch.cuda.Stream()
sp = stream.cuda_stream
accum = torch.empty((P, 3), dtype=torch.float64, device=DEV)
m2 = torch.empty(P, dtype=torch.float64, device=DEV)
counts = torch.zeros(P, dtype=torch.int32, device=DEV)
alb = torch.empty((P, 3), dtype=torch.float64, device=DEV)
nrm = torch.empty((P, 3), dtype=torch.float64, device=DEV)
dep = torch.empty(P, dtype=torch.float64, device=DEV)
hits = torch.empty(P, dtype=torch.int32, device=DEV)
out = torch.empty((P, 3), dtype=torch.float64, device=DEV)
var = torch.empty(P, dtype=torch.float64, device=DEV)
big = torch.empty((P, 3), dtype=torch.float64, device=DEV)
torch.cuda.synchronize()


def med(v):
    return round(statistics.median(v), 4)


def gather(camera, n):
    """The yardstick: n samples for every pixel of a new image (sample + reduce, ms)."""
    with torch.cuda.stream(stream):
        counts.zero_()
    r.accumulate_pixels(camera, None, n, accum.data_ptr(), m2.data_ptr(), counts.data_ptr(), stream_ptr=sp)
    s, d = r.kernel_times()
    return s + d


def features(camera):
    r.features(camera, 0, a.feature_samples, alb.data_ptr(), nrm.data_ptr(), dep.data_ptr(), hits.data_ptr(), stream_ptr=sp)


def denoise(levels, form=None):
    """One rt_denoise call on the buffers as they are (ms, reported as the sample kernel)."""
    if form is None:
        os.environ.pop("RTZIG_DENOISE_FORM", None)
    else:
        os.environ["RTZIG_DENOISE_FORM"] = form
    r.denoise(W, H, accum.data_ptr(), m2.data_ptr(), counts.data_ptr(), out.data_ptr(), d_albedo_ptr=alb.data_ptr(),
              d_normal_ptr=nrm.data_ptr(), d_depth_ptr=dep.data_ptr(), d_hits_ptr=hits.data_ptr(),
              feature_samples=a.feature_samples, params=rtzig.denoise_params(levels=levels), d_var_out_ptr=var.data_ptr(),
              stream_ptr=sp)
    s, d = r.kernel_times()
    os.environ.pop("RTZIG_DENOISE_FORM", None)
    return s + d


# ---- cost ---------------------------------------------------------------------------------------------
LV = list(range(a.max_levels + 1))
r.accumulate(cam.cam, big.data_ptr(), 0, a.ref_spp, stream_ptr=sp)  # warm-up: code objects, tree training
gather(cam.cam, a.samples)
features(cam.cam)
for n in LV:  # warm-up of every timed shape
    denoise(n), denoise(n, "tile"), denoise(n, "direct")
y, whole, dflt = [], [], []
DEFAULT_LEVELS = rtzig.denoise_params().levels
by_form = {f: {n: [] for n in LV} for f in ("tile", "direct")}
for _ in range(a.reps):  # alternating
    y.append(gather(cam.cam, a.samples))
    whole.append(denoise(5))
    dflt.append(denoise(DEFAULT_LEVELS))
    for f in ("tile", "direct"):
        for n in LV:
            by_form[f][n].append(denoise(n, f))
denoise(5)
stream.synchronize()
first = out.clone()
denoise(5)
stream.synchronize()
spread = max(y) - min(y)
m = {f: {n: statistics.median(v) for n, v in by_form[f].items()} for f in by_form}
cost = {
    "image": f"{W}x{H}", "spheres": len(cam.scene.world), "samples": a.samples, "feature_samples": a.feature_samples,
    "reps": a.reps, "tree": r.tree_info(),
    "yardstick_ms": [round(t, 4) for t in y], "yardstick_median_ms": med(y), "yardstick_spread_ms": round(spread, 4),
    "denoise_5_levels_ms": [round(t, 4) for t in whole], "denoise_5_levels_median_ms": med(whole),
    "default_levels": DEFAULT_LEVELS, "denoise_default_levels_ms": [round(t, 4) for t in dflt],
    "denoise_default_levels_median_ms": med(dflt),
    "denoise_over_yardstick": round(statistics.median(whole) / statistics.median(y), 4),
    "bar_ms": round(statistics.median(y) + spread, 4),
    "meets_bar": statistics.median(whole) <= statistics.median(y) + spread,
    "prepare_plus_prefilter_ms": round(m["tile"][0], 4),
    "whole_call_median_ms_by_levels": {f: {str(n): round(m[f][n], 4) for n in LV} for f in m},
    "level_ms": {f: {f"step_{1 << k}": round(m[f][k + 1] - m[f][k], 4) for k in range(a.max_levels)} for f in m},
    "two_runs_bit_equal": bool(torch.equal(first, out)),
}
print(json.dumps(cost), file=sys.stderr, flush=True)


# ---- quality ------------------------------------------------------------------------------------------
def rmse(x, ref):
    return float(torch.sqrt(torch.mean((x - ref) ** 2)))


def plain(camera, n):
    r.accumulate(camera, big.data_ptr(), 0, n, stream_ptr=sp)
    img = torch.empty_like(big)
    r.resolve(big.data_ptr(), P, n, img.data_ptr(), stream_ptr=sp)
    stream.synchronize()
    return img


rows = []
for k in range(a.seeds):
    c = RtCamera.from_buffer_copy(cam.cam)
    c.seed = cam.cam.seed + k
    rc = RtCamera.from_buffer_copy(cam.cam)
    rc.seed = cam.cam.seed + 0x1000 + k  # the reference shares no sample with the images it judges
    ref = plain(rc, a.ref_spp)
    row = {"seed": hex(c.seed), "plain_32": rmse(plain(c, 32), ref), "plain_64": rmse(plain(c, 64), ref)}
    gather(c, a.samples)
    features(c)
    noisy = torch.empty_like(big)
    r.resolve_counts(accum.data_ptr(), counts.data_ptr(), P, noisy.data_ptr(), stream_ptr=sp)
    stream.synchronize()
    row["noisy_%d" % a.samples] = rmse(noisy, ref)
    for n in range(1, a.max_levels + 1):
        denoise(n)
        stream.synchronize()
        row["denoised_levels_%d" % n] = rmse(out, ref)
    rows.append({k2: (v if isinstance(v, str) else round(v, 6)) for k2, v in row.items()})
    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
keys = [k for k in rows[0] if k != "seed"]
quality = {
    "image": f"{W}x{H}", "reference_spp": a.ref_spp, "samples": a.samples, "feature_samples": a.feature_samples,
    "rmse_by_seed": rows,
    "rmse_mean": {k: round(statistics.mean(x[k] for x in rows), 6) for k in keys},
    "rmse_spread": {k: round(max(x[k] for x in rows) - min(x[k] for x in rows), 6) for k in keys},
}
r.sync()
r.close()
if a.out_dir:
    os.makedirs(a.out_dir, exist_ok=True)
    for name, obj in (("cost.json", cost), ("quality.json", quality)):
        with open(os.path.join(a.out_dir, name), "w") as f:
            f.write(json.dumps(obj, indent=1) + "\n")
print(json.dumps({"cost": cost, "quality": quality}, indent=1))  # one object: the two files' contents

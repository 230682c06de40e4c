"""What adaptive sampling costs, on config 4 (final scene, 1200x800):
  - a gather pass over every pixel (NULL list) of 10 and of 50 samples against rt_render_rows_accumulate
    forced to direct mode at the same sizes — sample kernel and reduce pass, HIP events
    (rt_context_kernel_times), both continuing an image at 16 samples;
  - sparse gather passes of 50 samples over ascending lists holding 50%, 10% and 1% of the pixels
    (drawn at random, fixed seed), each against that share of the full pass;
  - rt_accum_select and rt_accum_resolve_counts (torch events around the calls);
  - one render_adaptive run (min 16, step 16, max 500): total samples, wall time, rounds, the histogram
    of counts — and the one-pass 500-spp render's wall time.
    python tools/adaptive_cost.py --out profiles/adaptive/cost.json"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracing-with-zig_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtzig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1200)
ap.add_argument("--aspect", type=float, default=1.5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--min", type=int, default=16)
ap.add_argument("--step", type=int, default=16)
ap.add_argument("--max", type=int, default=500)
ap.add_argument("--tolerance", type=float, default=0.05)
ap.add_argument("--floor", type=float, default=0.01)
ap.add_argument("--out", default=None)
a = ap.parse_args()

DEV = "cuda:0"
cam = rtzig.final_scene_camera(width=a.width, aspect_ratio=a.aspect, spp=a.max)
H, W = cam.height, cam.width
N = H * W
r = rtzig.DeviceRenderer(0)
r.set_scene(cam.scene.world)
r.enable_timing(True)
accum = torch.zeros((N, 3), dtype=torch.float64, device=DEV)
m2 = torch.zeros(N, dtype=torch.float64, device=DEV)
counts = torch.zeros(N, dtype=torch.int32, device=DEV)
out = torch.empty((N, 3), dtype=torch.float64, device=DEV)
BASE = 16  # the image every timed pass continues


def med(xs):
    return round(statistics.median(xs), 4)


def reset():
    counts.fill_(BASE)
    torch.cuda.synchronize()


def gather_ms(pixels, n, k=None):
    """Median (sample kernel, reduce pass) ms of a gather pass of n samples over `pixels`."""
    ts = []
    for _ in range(a.reps + 1):  # the first run warms up (workspace, tree)
        reset()
        r.accumulate_pixels(cam.cam, pixels, n, accum.data_ptr(), m2.data_ptr(), counts.data_ptr(), n_pixels=k)
        ts.append(r.kernel_times())
    return med([t[0] for t in ts[1:]]), med([t[1] for t in ts[1:]]), r.kernel_name()


def rows_ms(n):
    os.environ["RTZIG_UNIT_MODE"] = "direct"
    ts = []
    for _ in range(a.reps + 1):
        r.accumulate(cam.cam, accum.data_ptr(), BASE, n)
        ts.append(r.kernel_times())
    del os.environ["RTZIG_UNIT_MODE"]
    return med([t[0] for t in ts[1:]]), med([t[1] for t in ts[1:]]), r.kernel_name()


def event_ms(fn):
    ts = []
    for _ in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return med(ts[1:])


res = {"workload": f"final scene {W}x{H}", "reps": a.reps, "continuing_at_samples": BASE}
# ---- whole-image gather passes against row passes in direct mode -----------------------------------
r.accumulate_pixels(cam.cam, None, BASE, accum.data_ptr(), m2.data_ptr(), counts.data_ptr())  # real sums to continue
res["full"] = {}
for n in (10, 50):
    gs, gr, gname = gather_ms(None, n)
    ds, dr, dname = rows_ms(n)
    e = {"samples": n, "gather": {"sample_ms": gs, "reduce_ms": gr, "kernel": gname},
         "rows_direct": {"sample_ms": ds, "reduce_ms": dr, "kernel": dname},
         "gather_over_rows": round((gs + gr) / (ds + dr), 4)}
    res["full"][str(n)] = e
    print(json.dumps(e), file=sys.stderr, flush=True)
# ---- sparse lists ----------------------------------------------------------------------------------
full50 = res["full"]["50"]["gather"]
rng = np.random.default_rng(0xADA)
res["sparse_50_samples"] = {}
for share in (0.5, 0.1, 0.01):
    k = int(N * share)
    lst = torch.from_numpy(np.sort(rng.choice(N, k, replace=False)).astype(np.int32)).to(DEV)
    gs, gr, gname = gather_ms(lst.data_ptr(), 50, k)
    want = (full50["sample_ms"] + full50["reduce_ms"]) * share
    e = {"pixels": k, "sample_ms": gs, "reduce_ms": gr, "share_of_full_ms": round(want, 4),
         "over_share": round((gs + gr) / want, 4), "kernel": gname}
    res["sparse_50_samples"][str(share)] = e
    print(json.dumps(e), file=sys.stderr, flush=True)
# ---- select, resolve -------------------------------------------------------------------------------
reset()
d_list = torch.empty(N, dtype=torch.int32, device=DEV)
d_n = torch.zeros(1, dtype=torch.int32, device=DEV)
res["select_ms"] = event_ms(lambda: r.select(accum.data_ptr(), m2.data_ptr(), counts.data_ptr(), N, a.min, a.max,
                                             a.tolerance, a.floor, d_list.data_ptr(), d_n.data_ptr()))
res["select_selected"] = int(d_n.item())
res["resolve_counts_ms"] = event_ms(lambda: r.resolve_counts(accum.data_ptr(), counts.data_ptr(), N, out.data_ptr()))
r.sync()
r.close()
# ---- render_adaptive against the one-pass render ---------------------------------------------------
rounds = []
walls, one_walls = [], []
for _ in range(3):
    rounds.clear()
    t0 = time.perf_counter()
    img, cnt = rtzig.render_adaptive(cam.cam, cam.scene.world, a.min, a.max, a.step, a.tolerance, floor=a.floor,
                                     on_round=lambda k, lst, *_: rounds.append(int(lst.numel())))
    walls.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()  # the one-pass render through the same layers: a fresh context, a device image
    r1 = rtzig.DeviceRenderer(0)
    r1.set_scene(cam.scene.world)
    frame = torch.empty((H, W, 3), dtype=torch.float64, device=DEV)
    r1.render_rows_async(cam.cam, frame.data_ptr())
    one_img = frame.cpu().numpy()
    r1.sync()
    r1.close()
    one_walls.append((time.perf_counter() - t0) * 1e3)
values, number = np.unique(cnt, return_counts=True)
res["render_adaptive"] = {
    "min": a.min, "step": a.step, "max": a.max, "tolerance": a.tolerance, "floor": a.floor,
    "rounds": len(rounds), "selected_per_round": list(rounds), "total_samples": int(cnt.sum(dtype=np.int64)),
    "share_of_uniform_max": round(float(cnt.sum(dtype=np.int64)) / (N * a.max), 4),
    "mean_spp": round(float(cnt.mean()), 2),
    "wall_ms": [round(x, 2) for x in walls], "median_wall_ms": round(statistics.median(walls), 2),
    "one_pass_max_spp_wall_ms": [round(x, 2) for x in one_walls],
    "one_pass_median_wall_ms": round(statistics.median(one_walls), 2),
    "walls_include": "context creation, scene upload, tree training (memoised after the first run) and the copy "
                     "of the image to the host, on both sides",
    "pixels_at_max_equal_one_pass": bool(np.array_equal(img[cnt == a.max], one_img[cnt == a.max])),
    "counts_histogram": {str(int(v)): int(k) for v, k in zip(values, number)},
}
text = json.dumps(res, indent=1)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
print(text)

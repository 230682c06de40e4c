"""What progressive rendering costs: config 4 (1200x800, 500 spp) accumulated in
1 pass, 10 passes of 50 and 50 passes of 10 samples (rt_render_rows_accumulate), a linear resolve
(rt_accum_resolve) after every pass.  Wall time from the first launch to the last resolve, everything
issued back to back on one stream with ONE synchronize at the end; the per-pass overhead is
(wall - the one-pass wall) / (passes - 1).  Each pass picks its own unit mode and BVH training from
its size, as a user's would; the last image of every split is compared with the one-pass image.
    python tools/progressive_cost.py --out profiles/progressive/cost.json"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracing-with-zig_amd"))
import torch  # noqa: E402

import rtzig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1200)
ap.add_argument("--aspect", type=float, default=1.5)
ap.add_argument("--spp", type=int, default=500)
ap.add_argument("--passes", type=int, nargs="+", default=[1, 10, 50])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()

cam = rtzig.final_scene_camera(width=a.width, aspect_ratio=a.aspect, spp=a.spp)
H, W = cam.height, cam.width
r = rtzig.DeviceRenderer(0)
r.set_scene(cam.scene.world)
accum = torch.empty((H * W, 3), dtype=torch.float64, device="cuda:0")
out = torch.empty((H, W, 3), dtype=torch.float64, device="cuda:0")
stream = torch.cuda.Stream()
torch.cuda.synchronize()


def run(n_passes):
    """Wall ms of spp samples in n_passes equal passes, a resolve after each; the kernels' names."""
    count = a.spp // n_passes
    assert count * n_passes == a.spp
    names = set()
    t0 = time.perf_counter()
    for k in range(n_passes):
        r.accumulate(cam.cam, accum.data_ptr(), k * count, count, stream_ptr=stream.cuda_stream)
        r.resolve(accum.data_ptr(), H * W, (k + 1) * count, out.data_ptr(), stream_ptr=stream.cuda_stream)
        names.add(r.kernel_name())
    stream.synchronize()
    return (time.perf_counter() - t0) * 1e3, sorted(names)


res = {"workload": f"final scene {W}x{H}, {a.spp} spp, linear resolve after every pass", "reps": a.reps, "splits": {}}
one = None
for n in a.passes:
    run(n)  # warm-up: workspace of the split's unit mode, tree training, schedule upload
    img = out.clone()
    if one is None:
        one = img
    ms, names = zip(*[run(n) for _ in range(a.reps)])
    e = {"passes": n, "samples_per_pass": a.spp // n, "wall_ms": [round(x, 3) for x in ms],
         "median_wall_ms": round(statistics.median(ms), 3), "kernels": names[0],
         "bit_equal_to_first_split": bool(torch.equal(img, one))}
    res["splits"][str(n)] = e
    print(json.dumps(e), file=sys.stderr, flush=True)
r.sync()
r.close()
base = res["splits"][str(a.passes[0])]
for n in a.passes[1:]:
    e = res["splits"][str(n)]
    e["overhead_ms_per_extra_pass"] = round((e["median_wall_ms"] - base["median_wall_ms"]) / (n - a.passes[0]), 4)
text = json.dumps(res, indent=1)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
print(text)

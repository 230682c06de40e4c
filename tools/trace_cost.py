"""What a ray query costs: rt_trace_rays on the camera rays of config 4's image with
defocus_angle = 0 — 16 rays per pixel through jittered pixel positions, 15.36 M rays, laid out
sample-major so that a wave holds 64 neighbouring pixels (the feature pass's coherence) — writing
index + t.  The yardstick runs in the same process: rt_render_rows_features at 16 samples on that
camera, plus a device-to-device copy that moves the bytes the trace reads and writes (60 B per ray: a
copy of a buffer of half that size); bar = feature + copy + the yardstick's spread, i.e. the pass's
walk plus the memory traffic with no overlap at all.  Kernel times from the context's own events
(rt_context_kernel_times), the copy from torch events, all alternating, medians of --reps runs after
a warm-up of each.  Also, without a bar: all five outputs; the same rays under a fixed permutation
(incoherent); 65 536 far-origin rays before and after rt_context_reserve_origin_bound; the 1-ray and
64-ray kernel times; two runs compared bit for bit.
    python tools/trace_cost.py --out profiles/trace/cost.json"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--width", type=int, default=1200)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.reps >= 7
DEV = "cuda:0"


def med(v):
    return round(statistics.median(v), 4)


cam = rtzig.final_scene_camera(width=a.width, aspect_ratio=1.5, spp=1)
c = RtCamera.from_buffer_copy(cam.cam)
c.defocus_angle = 0.0
H, W = cam.height, cam.width
P, S = H * W, a.samples
n = P * S
r = rtzig.DeviceRenderer(0)
r.set_scene(cam.scene.world)
r.enable_timing(True)
stream = torch.cuda.Stream()
sp = stream.cuda_stream
f64 = dict(dtype=torch.float64, device=DEV)

with torch.cuda.stream(stream):
    # ray s * P + p: through pixel p's position jittered by sample s's offsets, from the camera centre
    g = torch.Generator(device=DEV).manual_seed(1)
    pix = torch.arange(P, device=DEV)
    fi = (pix % W).to(torch.float64).repeat(S) + (torch.rand(n, generator=g, **f64) - 0.5)
    fj = (pix // W).to(torch.float64).repeat(S) + (torch.rand(n, generator=g, **f64) - 0.5)
    vec = lambda v: torch.tensor(list(v), **f64)
    center = vec(c.center)
    D = (vec(c.pixel0) + fi[:, None] * vec(c.du) + fj[:, None] * vec(c.dv)) - center
    O = center.expand(n, 3).contiguous()
    del fi, fj
    perm = torch.randperm(n, generator=g, device=DEV)
    D_inc = D[perm].contiguous()
    del perm
    idx = torch.empty(n, dtype=torch.int32, device=DEV)
    t = torch.empty(n, **f64)
    point = torch.empty((n, 3), **f64)
    normal = torch.empty((n, 3), **f64)
    front = torch.empty(n, dtype=torch.uint8, device=DEV)
    alb = torch.empty((P, 3), **f64)
    nrm = torch.empty((P, 3), **f64)
    dep = torch.empty(P, **f64)
    hits = torch.empty(P, dtype=torch.int32, device=DEV)
    copy_src = torch.empty(n * 30, dtype=torch.uint8, device=DEV)  # read 30 B + write 30 B per ray
    copy_dst = torch.empty_like(copy_src)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
stream.synchronize()


def trace(o, d, count, full=False, st=None):
    extra = dict(d_point_ptr=point.data_ptr(), d_normal_ptr=normal.data_ptr(), d_front_ptr=front.data_ptr()) if full else {}
    r.trace_rays(o.data_ptr(), d.data_ptr(), count, c.t_min, c.t_max, d_index_ptr=idx.data_ptr(), d_t_ptr=t.data_ptr(),
                 d_stats_ptr=st.data_ptr() if st is not None else None, stream_ptr=sp, **extra)
    s, red = r.kernel_times()
    assert red == 0
    return s


def features():
    r.features(c, 0, S, alb.data_ptr(), nrm.data_ptr(), dep.data_ptr(), hits.data_ptr(), stream_ptr=sp)
    s, red = r.kernel_times()
    return s + red


def copy():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        copy_dst.copy_(copy_src)
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


features(), copy(), trace(O, D, n), trace(O, D, n, full=True), trace(O, D_inc, n)  # warm-up of every timed shape
y, cp, tr, tf, ti = [], [], [], [], []
for _ in range(a.reps):  # alternating
    y.append(features())
    cp.append(copy())
    tr.append(trace(O, D, n))
    tf.append(trace(O, D, n, full=True))
    ti.append(trace(O, D_inc, n))
name = r.kernel_name()
trace(O, D, n, st=stats)
stream.synchronize()
first_idx, first_t = idx.clone(), t.clone()
trace(O, D, n)
stream.synchronize()
two_equal = bool(torch.equal(first_idx, idx) and torch.equal(first_t.view(torch.int64), t.view(torch.int64)))
hit_share = float((idx >= 0).double().mean())
routing = stats.cpu().tolist()

tiny = {}
for k in (1, 64):
    trace(O, D, k)
    tiny[str(k)] = med([trace(O, D, k) for _ in range(a.reps)])

# far origins: 65 536 rays from 400x the scene's radius of interest, aimed back at it
nf = 65536
with torch.cuda.stream(stream):
    Of = torch.rand((nf, 3), generator=g, **f64) * torch.tensor([24.0, 2.95, 24.0], **f64) + torch.tensor([-12.0, 0.05, -12.0], **f64)
    Of = Of * 400
    Df = -Of + torch.randn((nf, 3), generator=g, **f64)
stream.synchronize()
far = {"rays": nf, "bound_before": r.origin_bound()}
stats.zero_()
torch.cuda.synchronize()
trace(Of, Df, nf)
far["scan_ms"] = med([trace(Of, Df, nf) for _ in range(a.reps)])
trace(Of, Df, nf, st=stats)
stream.synchronize()
far["scanned_before"] = stats.cpu().tolist()[1]
far_idx = idx[:nf].clone()
r.reserve_origin_bound(6000)
far["bound_after"] = r.origin_bound()
stats.zero_()
torch.cuda.synchronize()
trace(Of, Df, nf)
far["tree_ms"] = med([trace(Of, Df, nf) for _ in range(a.reps)])
trace(Of, Df, nf, st=stats)
stream.synchronize()
far["scanned_after"] = stats.cpu().tolist()[1]
far["same_indices"] = bool(torch.equal(far_idx, idx[:nf]))
info = r.tree_info()
r.sync()
r.close()

spread = max(y) - min(y)
bar = statistics.median(y) + statistics.median(cp) + spread
res = {
    "image": f"{W}x{H}", "rays_per_pixel": S, "rays": n, "reps": a.reps, "spheres": len(cam.scene.world), "tree": info,
    "trace_kernel": name, "hit_share": round(hit_share, 4), "stats": routing,
    "feature_ms": [round(v, 4) for v in y], "feature_median_ms": med(y), "feature_spread_ms": round(spread, 4),
    "copy_bytes_moved": n * 60, "copy_ms": [round(v, 4) for v in cp], "copy_median_ms": med(cp),
    "trace_ms": [round(v, 4) for v in tr], "trace_median_ms": med(tr),
    "bar_ms": round(bar, 4), "meets_bar": statistics.median(tr) <= bar,
    "rays_per_second": round(n / (statistics.median(tr) * 1e-3)),
    "all_outputs_ms": [round(v, 4) for v in tf], "all_outputs_median_ms": med(tf),
    "incoherent_ms": [round(v, 4) for v in ti], "incoherent_median_ms": med(ti),
    "tiny_batch_ms": tiny, "far_origins": far, "two_runs_bit_equal": two_equal,
}
text = json.dumps(res, indent=1)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
print(text)

"""Python mirror of the reference's host API over the C ABI (names follow the Zig code).

    scene = Scene.init(0xdeadbeef)                      # Scene.zig:23
    scene.generateWorld()                               # Scene.zig:48
    camera = (Camera.builder(400, 16.0 / 9.0)           # camera.zig:109
              .setScene(scene).setDefocusAngle(0.6).setFocusDist(10)
              .setViewport((13, 2, 3), (0, 0, 0), 20).setSamplesPerPixel(10)
              .build())                                 # camera.zig:300
    ppm = camera.render()                               # camera.zig:123 -> rt_render (HIP)
    ppm.saveBinary("images/chapter14.ppm")              # ppm.zig:42

Scene generation and camera construction run in the C++ host mirror (csrc/rt_host.cpp); render()
runs the HIP kernel on gfx950 GPUs.  There is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np

from . import abi
from .abi import D3, RtCamera, RtCameraParams, RtOptions, RtSphere
from .lib import check, load

INF = math.inf


class Scene:
    """Scene.zig:16-187: world (Hittable list), seed, interval."""

    def __init__(self, seed):
        self.seed = seed
        self.world = (RtSphere * 0)()
        self.interval = (1e-3, INF)  # Scene.zig:21
        self.prng_state = None       # Xoshiro256++ words after generateWorld (for oracle A)

    @staticmethod
    def init(seed=None):
        if seed is None:
            import secrets
            seed = secrets.randbits(64)  # std.posix.getrandom stand-in (Scene.zig:33-37)
        return Scene(seed)

    def generateWorld(self):
        lib = load()
        n = C.c_size_t()
        check("rt_scene_final", lib.rt_scene_final(self.seed, None, 0, C.byref(n), None))
        arr = (RtSphere * n.value)()
        st = (C.c_uint64 * 4)()
        check("rt_scene_final", lib.rt_scene_final(self.seed, arr, n.value, C.byref(n), st))
        self.world = _concat(self.world, arr)
        self.prng_state = list(st)
        return self

    def generateChapter13(self):
        lib = load()
        n = C.c_size_t()
        arr = (RtSphere * 8)()
        check("rt_scene_chapter13", lib.rt_scene_chapter13(arr, 8, C.byref(n)))
        self.world = _concat(self.world, (RtSphere * n.value).from_buffer_copy(arr))
        return self

    def add(self, center, radius, material, albedo=(1, 1, 1), fuzz=0.0, refraction_index=1.0):
        s = RtSphere(center=D3(*center), radius=max(0.0, radius), material=material,
                     albedo=D3(*albedo), fuzz=fuzz, refraction_index=refraction_index)
        self.world = _concat(self.world, (RtSphere * 1)(s))
        return self

    def hit(self, origins, directions, t_min=1e-3, t_max=INF, intervals=None, device=0):
        """world.hit (hittable.zig:64-77) for (n, 3) arrays of rays, on the GPU: trace_rays' dict."""
        return trace_rays(self.world, origins, directions, t_min=t_min, t_max=t_max, intervals=intervals,
                          device=device)

    def occluded(self, origins, ends, t_min=1e-3, t_max=INF, intervals=None, targets=False, device=0):
        """Does world.hit return true?  One bool per ray, on the GPU (rtzig.occluded)."""
        return occluded(self.world, origins, ends, t_min=t_min, t_max=t_max, intervals=intervals, targets=targets,
                        device=device)

    def radiance(self, origins, directions, samples=1, bounce_max=50, ray_base=0, t_min=1e-3, t_max=INF, states=None,
                 device=0):
        """rayColor of (n, 3) arrays of rays in this world, on the GPU: the (n, 3) unscaled sums of
        `samples` samples per ray, streams keyed with the scene's seed (rtzig.radiance)."""
        return radiance(self.world, origins, directions, samples=samples, bounce_max=bounce_max, seed=self.seed,
                        ray_base=ray_base, t_min=t_min, t_max=t_max, states=states, device=device)

    def visible(self, a, b, eps=1e-3, device=0):
        """Line of sight: no sphere has a root in the open segment (eps, 1) from a[q] to b[q]."""
        return ~occluded(self.world, a, b, t_min=eps, t_max=1.0, targets=True, device=device)


def _concat(a, b):
    out = (RtSphere * (len(a) + len(b)))()
    C.memmove(out, a, C.sizeof(a))
    C.memmove(C.addressof(out) + C.sizeof(a), b, C.sizeof(b))
    return out


class CameraBuilder:
    """camera.zig:233-346 (defaults camera.zig:218-232)."""

    def __init__(self, width, aspect_ratio):
        self.p = RtCameraParams(image_width=width, samples_per_pixel=100, bounce_max=50,
                                aspect_ratio=aspect_ratio, look_from=D3(0, 0, 0),
                                look_at=D3(0, 0, -1), v_up=D3(0, 1, 0), vfov=90.0,
                                defocus_angle=0.0, focus_dist=10.0, t_min=1e-3, t_max=INF,
                                seed=0)
        self.scene = None

    def setScene(self, scene):
        self.scene = scene
        self.p.seed = scene.seed
        self.p.t_min, self.p.t_max = scene.interval
        return self

    def setFocusDist(self, d):
        self.p.focus_dist = d
        return self

    def setDefocusAngle(self, a):
        self.p.defocus_angle = a
        return self

    def setViewport(self, look_from, look_at, vfov):
        self.p.look_from = D3(*look_from)
        self.p.look_at = D3(*look_at)
        self.p.vfov = vfov
        return self

    def setSamplesPerPixel(self, spp):
        self.p.samples_per_pixel = spp
        return self

    def setBounceMax(self, b):
        self.p.bounce_max = b
        return self

    def setVUp(self, v):
        self.p.v_up = D3(*v)
        return self

    def build(self):
        cam = RtCamera()
        check("rt_camera_build", load().rt_camera_build(C.byref(self.p), C.byref(cam)))
        return Camera(cam, self.scene if self.scene is not None else Scene.init(None))


class Camera:
    """camera.zig:82-216.  `cam` holds the flattened fields that cross the C ABI."""

    def __init__(self, cam, scene):
        self.cam = cam
        self.scene = scene

    @staticmethod
    def builder(width, aspect_ratio):
        return CameraBuilder(width, aspect_ratio)

    @property
    def width(self):
        return self.cam.image_width

    @property
    def height(self):
        return self.cam.image_height

    def render(self, n_gpus=0, device=0, output="linear", stats=None, precision="f64"):
        """Camera.render (camera.zig:123-145) on the GPU(s).  Returns a PPM."""
        return PPM(self.width, self.height,
                   render(self.cam, self.scene.world, n_gpus=n_gpus, device=device,
                          output=output, stats=stats, precision=precision))

    def render_progressive(self, passes, device=0, output="linear", precision="f64"):
        """Generator over (samples_done, PPM) after each pass of `passes` samples (render_progressive);
        samplesPerPixel of the camera is not used."""
        for done, img in render_progressive(self.cam, self.scene.world, passes, device=device, output=output,
                                            precision=precision):
            yield done, PPM(self.width, self.height, img)

    def render_adaptive(self, min_spp, max_spp, step, tolerance, floor=0.01, device=0, output="linear",
                        precision="f64", on_round=None):
        """(PPM, counts) of render_adaptive: samples go where the noise estimate asks for them;
        samplesPerPixel of the camera is not used."""
        img, counts = render_adaptive(self.cam, self.scene.world, min_spp, max_spp, step, tolerance, floor=floor,
                                      device=device, output=output, precision=precision, on_round=on_round)
        return PPM(self.width, self.height, img), counts

    def render_features(self, spp, device=0):
        """The dict of render_features: first-hit albedo, normal, depth, coverage and hits per pixel
        at `spp` samples; samplesPerPixel of the camera is not used."""
        return render_features(self.cam, self.scene.world, spp, device=device)

    def render_denoised(self, spp, feature_spp=4, params=None, adaptive=None, device=0, output="linear",
                        precision="f64"):
        """The dict of render_denoised: `spp` samples per pixel (more where adaptive= asks for them),
        `feature_spp` feature samples, then rt_denoise; samplesPerPixel of the camera is not used."""
        return render_denoised(self.cam, self.scene.world, spp, feature_spp=feature_spp, params=params,
                               adaptive=adaptive, device=device, output=output, precision=precision)


_PRECISION = {"f64": abi.RT_PRECISION_F64, "f32": abi.RT_PRECISION_F32}


def render(cam, spheres, n_gpus=0, device=0, output="linear", stats=None, precision="f64"):
    """rt_render: whole image into host memory.  linear -> (H, W, 3) f64; rgb8 -> (H, W, 3) u8.
    precision: "f64" (parity, bit-exact) or "f32" (fast mode, statistical parity)."""
    lib = load()
    W, H = cam.image_width, cam.image_height
    if output == "linear":
        out = np.zeros((H, W, 3), np.float64)
        fmt = abi.RT_OUT_LINEAR_F64
    elif output == "rgb8":
        out = np.zeros((H, W, 3), np.uint8)
        fmt = abi.RT_OUT_RGB8
    else:
        raise ValueError(output)
    st = (C.c_uint64 * 2)()
    opts = RtOptions(n_gpus=n_gpus, device=device, pixel_stride=3, output_format=fmt,
                     precision=_PRECISION[precision], stats_out=C.cast(st, C.POINTER(C.c_uint64)))
    n = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * n)(*spheres)
    check("rt_render", lib.rt_render(C.byref(cam), arr, n, C.byref(opts),
                                     out.ctypes.data_as(C.c_void_p)))
    if stats is not None:
        stats["rays"] = st[0]
        stats["samples"] = st[1]
    return out


def render_progressive(cam, spheres, passes, device=0, output="linear", precision="f64"):
    """Progressive render on one GPU: a generator that renders `passes` (a sequence of sample counts)
    one after the other onto one device accumulator and yields (samples_done, image) after each —
    the image a one-pass render at spp = samples_done gives, bit for bit (linear -> (H, W, 3) f64,
    rgb8 -> (H, W, 3) u8).  cam.samples_per_pixel is not used.  Stopping the generator early stops
    the render; the device buffers are torch tensors (imported here, not with the package)."""
    if output not in ("linear", "rgb8"):
        raise ValueError(output)
    passes = [int(n) for n in passes]
    if any(n < 0 for n in passes):
        raise ValueError("passes must be sample counts >= 0")
    import torch

    W, H = cam.image_width, cam.image_height
    n = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * n)(*spheres)
    r = DeviceRenderer(device)
    try:
        r.set_scene(arr)
        r.set_precision(precision)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            accum = torch.empty((H * W, 3), dtype=torch.float64, device=dev)
            out = torch.empty((H, W, 3), dtype=torch.float64 if output == "linear" else torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            done = 0
            for count in passes:
                r.accumulate(cam, accum.data_ptr(), done, count, stream_ptr=stream)
                done += count
                if done == 0:
                    continue  # nothing accumulated yet: no image to show
                r.resolve(accum.data_ptr(), H * W, done, out.data_ptr(), output=output, stream_ptr=stream)
                img = out.cpu().numpy()  # waits for the stream
                r.sync()  # reports a failure the kernel recorded
                yield done, img
    finally:
        r.close()


def _adaptive_args(min_spp, max_spp, step, tolerance, floor, output):
    """render_adaptive's argument checks (host only): the values as (min_spp, max_spp, step,
    tolerance, floor)."""
    if output not in ("linear", "rgb8"):
        raise ValueError(output)
    min_spp, max_spp, step = int(min_spp), int(max_spp), int(step)
    tolerance, floor = float(tolerance), float(floor)
    if min_spp < 2:
        raise ValueError("min_spp must be at least 2 (the noise estimate needs two samples)")
    if max_spp < min_spp:
        raise ValueError("max_spp must be at least min_spp")
    if max_spp >= 2 ** 32:
        raise ValueError("max_spp must be below 2^32")
    if step < 1:
        raise ValueError("step must be at least 1")
    if math.isnan(tolerance) or tolerance < 0:
        raise ValueError("tolerance must be a number >= 0")
    if not floor > 0:
        raise ValueError("floor must be > 0")
    return min_spp, max_spp, step, tolerance, floor


def _adaptive_rounds(r, cam, accum, m2, counts, lst, n_sel, min_spp, max_spp, step, tolerance, floor, stream,
                     on_round=None):
    """render_adaptive's loop on the caller's device tensors (counts zeroed): min_spp samples for every
    pixel, then rounds of selection and `step` more samples until nothing is selected."""
    n_pix = counts.numel()
    r.accumulate_pixels(cam, None, min_spp, accum.data_ptr(), m2.data_ptr(), counts.data_ptr(), stream_ptr=stream)
    rnd = 0
    while True:
        r.select(accum.data_ptr(), m2.data_ptr(), counts.data_ptr(), n_pix, min_spp, max_spp, tolerance, floor,
                 lst.data_ptr(), n_sel.data_ptr(), stream_ptr=stream)
        k = int(n_sel.item())  # the round's host sync
        if on_round is not None:
            on_round(rnd, lst[:k], accum, m2, counts)
        if k == 0:
            break
        # a pixel selected now was selected in every round before: all of the list stand at
        # min_spp + rnd * step samples, so one clamp keeps every pixel within max_spp
        more = min(step, max_spp - (min_spp + rnd * step))
        r.accumulate_pixels(cam, lst.data_ptr(), more, accum.data_ptr(), m2.data_ptr(), counts.data_ptr(),
                            n_pixels=k, stream_ptr=stream)
        rnd += 1


def render_adaptive(cam, spheres, min_spp, max_spp, step, tolerance, floor=0.01, device=0, output="linear",
                    precision="f64", on_round=None):
    """Adaptive render on one GPU: every pixel gets min_spp samples; then, round after round, the
    pixels whose noise estimate is still above `tolerance` (rt_accum_select: the standard error of
    the pixel's mean luminance r + g + b, relative to max(mean, floor)) get `step` more — fewer in the
    round that would pass max_spp — until none is selected.  Returns (image, counts): the image
    (linear -> (H, W, 3) f64, rgb8 -> (H, W, 3) u8) and the (H, W) uint32 samples each pixel got.
    Every pixel is, bit for bit, the pixel of a one-pass render at spp = its own count.

    Each round reads the number of selected pixels back: one 4-byte copy and host sync per round.
    on_round(round, list, accum, m2, counts) is called after each selection (the last one, which
    selects nothing, included) with device tensors: the selected indices (int32, ascending), the
    unscaled sums (W*H, 3), the squared-luminance sums (W*H) and the counts (W*H, int32) at that point.
    cam.samples_per_pixel is not used."""
    min_spp, max_spp, step, tolerance, floor = _adaptive_args(min_spp, max_spp, step, tolerance, floor, output)
    import torch

    W, H = cam.image_width, cam.image_height
    n = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * n)(*spheres)
    r = DeviceRenderer(device)
    try:
        r.set_scene(arr)
        r.set_precision(precision)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            accum = torch.empty((H * W, 3), dtype=torch.float64, device=dev)
            m2 = torch.empty(H * W, dtype=torch.float64, device=dev)
            counts = torch.zeros(H * W, dtype=torch.int32, device=dev)  # u32 on the device
            lst = torch.empty(H * W, dtype=torch.int32, device=dev)
            n_sel = torch.zeros(1, dtype=torch.int32, device=dev)
            out = torch.empty((H, W, 3), dtype=torch.float64 if output == "linear" else torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _adaptive_rounds(r, cam, accum, m2, counts, lst, n_sel, min_spp, max_spp, step, tolerance, floor, stream,
                             on_round)
            r.resolve_counts(accum.data_ptr(), counts.data_ptr(), H * W, out.data_ptr(), output=output, stream_ptr=stream)
            img = out.cpu().numpy()  # waits for the stream
            cnt = counts.cpu().numpy().view(np.uint32).reshape(H, W)
            r.sync()  # reports a failure the kernel recorded
        return img, cnt
    finally:
        r.close()


def render_features(cam, spheres, spp, device=0):
    """Feature buffers of the whole image on one GPU (rt_render_rows_features at `spp` samples): a dict
    of numpy arrays for a denoiser or compositor —
        albedo   (H, W, 3) f64  first-hit albedo, the sums resolved with rt_accum_resolve at spp
        normal   (H, W, 3) f64  shading normal, likewise (not renormalised)
        depth    (H, W)    f64  depth_sum / hits, inf where no sample hit
        coverage (H, W)    f64  hits / spp
        hits     (H, W)    u32  samples whose camera ray hit a sphere
    Samples that miss contribute nothing to albedo and normal.  cam.samples_per_pixel is not used."""
    spp = int(spp)
    if spp < 1 or spp >= 2 ** 32:
        raise ValueError("spp must be in [1, 2^32)")
    import torch

    W, H = cam.image_width, cam.image_height
    n = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * n)(*spheres)
    r = DeviceRenderer(device)
    try:
        r.set_scene(arr)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            sums = torch.empty((2, H * W, 3), dtype=torch.float64, device=dev)  # albedo, normal
            depth = torch.empty(H * W, dtype=torch.float64, device=dev)
            hits = torch.empty(H * W, dtype=torch.int32, device=dev)  # u32 on the device
            out = torch.empty((2, H, W, 3), dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            r.features(cam, 0, spp, sums[0].data_ptr(), sums[1].data_ptr(), depth.data_ptr(), hits.data_ptr(),
                       stream_ptr=stream)
            r.resolve(sums[0].data_ptr(), H * W, spp, out[0].data_ptr(), stream_ptr=stream)
            r.resolve(sums[1].data_ptr(), H * W, spp, out[1].data_ptr(), stream_ptr=stream)
            res = out.cpu().numpy()  # waits for the stream
            dsum = depth.cpu().numpy().reshape(H, W)
            cnt = hits.cpu().numpy().view(np.uint32).reshape(H, W)
            r.sync()  # reports a failure the kernel recorded
    finally:
        r.close()
    mean_depth = np.full((H, W), np.inf)
    np.divide(dsum, cnt, out=mean_depth, where=cnt != 0)
    return {"albedo": res[0], "normal": res[1], "depth": mean_depth, "coverage": cnt / float(spp), "hits": cnt}


def trace_rays(spheres, origins, directions, t_min=1e-3, t_max=INF, intervals=None, device=0):
    """HittableList.hit of caller-supplied rays on one GPU (rt_trace_rays), bit for bit the reference's
    f64 result.  origins, directions: (n, 3) arrays; intervals: None or (n, 2), per-ray (t_min, t_max).
    Returns a dict of numpy arrays:
        index  (n,)   i32  the sphere hit (its index in `spheres`), -1 on a miss
        t      (n,)   f64  the accepted root, inf on a miss
        point  (n, 3) f64  origin + direction * t, 0 on a miss
        normal (n, 3) f64  the normal after setFaceNormal, 0 on a miss
        front  (n,)   bool the ray hit the outside of the sphere"""
    import torch

    o = np.ascontiguousarray(origins, np.float64)
    d = np.ascontiguousarray(directions, np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError("origins and directions must both be (n, 3)")
    n = o.shape[0]
    iv = None
    if intervals is not None:
        iv = np.ascontiguousarray(intervals, np.float64)
        if iv.shape != (n, 2):
            raise ValueError("intervals must be (n, 2)")
    if n == 0:
        return {"index": np.zeros(0, np.int32), "t": np.zeros(0), "point": np.zeros((0, 3)),
                "normal": np.zeros((0, 3)), "front": np.zeros(0, bool)}
    ns = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * ns)(*spheres)
    r = DeviceRenderer(device)
    try:
        r.set_scene(arr)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            d_o = torch.from_numpy(o).to(dev)
            d_d = torch.from_numpy(d).to(dev)
            d_iv = torch.from_numpy(iv).to(dev) if iv is not None else None
            idx = torch.empty(n, dtype=torch.int32, device=dev)
            t = torch.empty(n, dtype=torch.float64, device=dev)
            vec = torch.empty((2, n, 3), dtype=torch.float64, device=dev)  # point, normal
            front = torch.empty(n, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            r.trace_rays(d_o.data_ptr(), d_d.data_ptr(), n, t_min, t_max, idx.data_ptr(), t.data_ptr(),
                         vec[0].data_ptr(), vec[1].data_ptr(), front.data_ptr(),
                         d_intervals_ptr=d_iv.data_ptr() if d_iv is not None else None, stream_ptr=stream)
            res = {"index": idx.cpu().numpy(), "t": t.cpu().numpy()}  # waits for the stream
            v = vec.cpu().numpy()
            res.update(point=v[0], normal=v[1], front=front.cpu().numpy().astype(bool))
            r.sync()  # reports a failure the kernel recorded
    finally:
        r.close()
    return res


def occluded(spheres, origins, ends, t_min=1e-3, t_max=INF, intervals=None, targets=False, device=0):
    """Occlusion of caller-supplied rays on one GPU (rt_occluded_rays): (n,) bool, True where
    HittableList.hit returns true in the reference's f64 arithmetic — trace_rays' index >= 0, from a walk
    that stops at the first accepted root.  origins, ends: (n, 3) arrays; `ends` holds directions, or
    with targets=True end points (the direction is end - origin, and (eps, 1.0) is the open segment);
    intervals: None or (n, 2), per-ray (t_min, t_max)."""
    import torch

    o = np.ascontiguousarray(origins, np.float64)
    e = np.ascontiguousarray(ends, np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or e.shape != o.shape:
        raise ValueError("origins and ends must both be (n, 3)")
    n = o.shape[0]
    iv = None
    if intervals is not None:
        iv = np.ascontiguousarray(intervals, np.float64)
        if iv.shape != (n, 2):
            raise ValueError("intervals must be (n, 2)")
    if n == 0:
        return np.zeros(0, bool)
    ns = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * ns)(*spheres)
    r = DeviceRenderer(device)
    try:
        r.set_scene(arr)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            d_o = torch.from_numpy(o).to(dev)
            d_e = torch.from_numpy(e).to(dev)
            d_iv = torch.from_numpy(iv).to(dev) if iv is not None else None
            occ = torch.empty(n, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            r.occluded_rays(d_o.data_ptr(), d_e.data_ptr(), n, t_min, t_max, d_occluded_ptr=occ.data_ptr(),
                            d_intervals_ptr=d_iv.data_ptr() if d_iv is not None else None, targets=targets,
                            stream_ptr=stream)
            res = occ.cpu().numpy().astype(bool)  # waits for the stream
            r.sync()  # reports a failure the kernel recorded
    finally:
        r.close()
    return res


def radiance(spheres, origins, directions, samples=1, bounce_max=50, seed=0xdeadbeef, ray_base=0, t_min=1e-3, t_max=INF,
             states=None, device=0):
    """Camera.rayColor of caller-supplied rays on one GPU (rt_radiance_rays), bit for bit the reference's
    f64 result: the (n, 3) unscaled sums of `samples` samples per ray, added in sample order (divide by
    `samples` for the mean).  origins, directions: (n, 3) arrays, directions used as given.  Sample s of
    ray q draws from the stream rt_sample_key(seed, ray_base + q, s).  states: None, or (n, 4) uint64
    Xoshiro256++ states the one sample of each ray continues (samples must be 1)."""
    import torch

    o = np.ascontiguousarray(origins, np.float64)
    d = np.ascontiguousarray(directions, np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError("origins and directions must both be (n, 3)")
    n = o.shape[0]
    samples, bounce_max, ray_base = int(samples), int(bounce_max), int(ray_base)
    if samples < 0 or samples >= 2 ** 32 or bounce_max < 0 or bounce_max >= 2 ** 32:
        raise ValueError("samples and bounce_max must be in [0, 2^32)")
    if ray_base < 0 or ray_base + n > 2 ** 32:
        raise ValueError("ray_base + n must be at most 2^32")
    st = None
    if states is not None:
        st = np.ascontiguousarray(states, np.uint64)
        if st.shape != (n, 4):
            raise ValueError("states must be (n, 4) uint64")
        if samples != 1:
            raise ValueError("states need samples == 1")
    if n == 0 or samples == 0:
        return np.zeros((n, 3))
    ns = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * ns)(*spheres)
    r = DeviceRenderer(device)
    try:
        r.set_scene(arr)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            d_o = torch.from_numpy(o).to(dev)
            d_d = torch.from_numpy(d).to(dev)
            d_st = torch.from_numpy(st.view(np.int64)).to(dev) if st is not None else None
            sums = torch.empty((n, 3), dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            r.radiance_rays(d_o.data_ptr(), d_d.data_ptr(), n, sums.data_ptr(), sample_count=samples,
                            bounce_max=bounce_max, seed=seed, ray_base=ray_base, t_min=t_min, t_max=t_max,
                            d_states_ptr=d_st.data_ptr() if d_st is not None else None, stream_ptr=stream)
            res = sums.cpu().numpy()  # waits for the stream
            r.sync()  # reports a failure the kernel recorded
    finally:
        r.close()
    return res


def denoise_params(**overrides):
    """rt_denoise_params: the library's defaults (rt_denoise_default_params: levels 2, sigma_l 4,
    sigma_n 32, sigma_a 32, sigma_z 0.05, sigma_h 4, epsilon 1e-6) with the given fields replaced."""
    p = abi.RtDenoiseParams()
    check("rt_denoise_default_params", load().rt_denoise_default_params(C.byref(p)))
    names = [n for n, _ in abi.RtDenoiseParams._fields_]
    for k, v in overrides.items():
        if k not in names:
            raise TypeError(f"denoise_params: no field {k!r}")
        setattr(p, k, v)
    return p


def render_denoised(cam, spheres, spp, feature_spp=4, params=None, adaptive=None, device=0, output="linear",
                    precision="f64"):
    """A denoised render on one GPU: every pixel gets `spp` samples (a gather pass over every pixel,
    which also fills the squared-luminance sums); with adaptive=dict(max_spp=, step=, tolerance=,
    floor=0.01) render_adaptive's rounds then add samples from min_spp = spp; then `feature_spp`
    feature samples (rt_render_rows_features) and rt_denoise (params: denoise_params(), None for the
    defaults).  Returns a dict of numpy arrays:
        image    (H, W, 3)  the denoised image, linear f64 or rgb8 u8
        noisy    (H, W, 3)  the input image (rt_accum_resolve_counts), same format
        variance (H, W) f64 the filtered variance of the mean luminance
        counts   (H, W) u32 the samples each pixel got
    cam.samples_per_pixel is not used."""
    if output not in ("linear", "rgb8"):
        raise ValueError(output)
    spp, feature_spp = int(spp), int(feature_spp)
    if spp < 2 or spp >= 2 ** 32:
        raise ValueError("spp must be in [2, 2^32) (the variance estimate needs two samples)")
    if feature_spp < 1 or feature_spp >= 2 ** 32:
        raise ValueError("feature_spp must be in [1, 2^32)")
    if adaptive is not None:
        extra = set(adaptive) - {"max_spp", "step", "tolerance", "floor"}
        if extra or not {"max_spp", "step", "tolerance"} <= set(adaptive):
            raise ValueError("adaptive: a dict of max_spp, step, tolerance and optionally floor")
        _, max_spp, step, tolerance, floor = _adaptive_args(spp, adaptive["max_spp"], adaptive["step"],
                                                            adaptive["tolerance"], adaptive.get("floor", 0.01), output)
    import torch

    W, H = cam.image_width, cam.image_height
    n = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * n)(*spheres)
    r = DeviceRenderer(device)
    try:
        r.set_scene(arr)
        r.set_precision(precision)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            accum = torch.empty((H * W, 3), dtype=torch.float64, device=dev)
            m2 = torch.empty(H * W, dtype=torch.float64, device=dev)
            counts = torch.zeros(H * W, dtype=torch.int32, device=dev)  # u32 on the device
            sums = torch.empty((2, H * W, 3), dtype=torch.float64, device=dev)  # albedo, normal
            depth = torch.empty(H * W, dtype=torch.float64, device=dev)
            hits = torch.empty(H * W, dtype=torch.int32, device=dev)  # u32 on the device
            odt = torch.float64 if output == "linear" else torch.uint8
            out = torch.empty((2, H, W, 3), dtype=odt, device=dev)  # denoised, noisy
            var = torch.empty((H, W), dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            if adaptive is None:
                r.accumulate_pixels(cam, None, spp, accum.data_ptr(), m2.data_ptr(), counts.data_ptr(), stream_ptr=stream)
            else:
                lst = torch.empty(H * W, dtype=torch.int32, device=dev)
                n_sel = torch.zeros(1, dtype=torch.int32, device=dev)
                _adaptive_rounds(r, cam, accum, m2, counts, lst, n_sel, spp, max_spp, step, tolerance, floor, stream)
            r.features(cam, 0, feature_spp, sums[0].data_ptr(), sums[1].data_ptr(), depth.data_ptr(), hits.data_ptr(),
                       stream_ptr=stream)
            r.denoise(W, H, accum.data_ptr(), m2.data_ptr(), counts.data_ptr(), out[0].data_ptr(),
                      d_albedo_ptr=sums[0].data_ptr(), d_normal_ptr=sums[1].data_ptr(), d_depth_ptr=depth.data_ptr(),
                      d_hits_ptr=hits.data_ptr(), feature_samples=feature_spp, params=params, output=output,
                      d_var_out_ptr=var.data_ptr(), stream_ptr=stream)
            r.resolve_counts(accum.data_ptr(), counts.data_ptr(), H * W, out[1].data_ptr(), output=output, stream_ptr=stream)
            res = out.cpu().numpy()  # waits for the stream
            v = var.cpu().numpy()
            cnt = counts.cpu().numpy().view(np.uint32).reshape(H, W)
            r.sync()  # reports a failure the kernel recorded
        return {"image": res[0], "noisy": res[1], "variance": v, "counts": cnt}
    finally:
        r.close()


def temporal_params(**overrides):
    """rt_temporal_params: the library's defaults (rt_temporal_default_params: max_history 64, sigma_z 0.05,
    tau_n 0.1, tau_a 0.05, tau_h 0.5, min_weight 0.25) with the given fields replaced."""
    p = abi.RtTemporalParams()
    check("rt_temporal_default_params", load().rt_temporal_default_params(C.byref(p)))
    names = [n for n, _ in abi.RtTemporalParams._fields_]
    for k, v in overrides.items():
        if k not in names:
            raise TypeError(f"temporal_params: no field {k!r}")
        setattr(p, k, v)
    return p


def render_sequence(cams, spheres, spp, feature_spp=4, temporal=None, denoise=None, seed_step=1, device=0,
                    output="linear", precision="f64"):
    """A generator over the frames of a camera path through a static scene, on one GPU.  Frame f renders
    cams[f] with seed = cams[f].seed + f * seed_step (mod 2^64) — a sample's stream is keyed by (seed,
    pixel, sample), so frames that shared a seed would repeat their random numbers and the history would
    add no information — as a gather pass of `spp` samples and a feature pass of `feature_spp`; then
    rt_temporal_accumulate merges the previous frame's merged buffers into it (temporal: temporal_params(),
    None for the defaults, False to render every frame on its own), and rt_denoise (denoise:
    denoise_params(), None for the defaults) filters the result.  Two buffer sets take turns.  Yields one
    dict of numpy arrays per frame:
        image    (H, W, 3)  the denoised image, linear f64 or rgb8 u8
        noisy    (H, W, 3)  the merged sums resolved (rt_accum_resolve_counts), same format
        variance (H, W) f64 the filtered variance of the mean luminance
        counts   (H, W) u32 samples plus pseudo-samples of each pixel
        history  (H, W) u32 the pseudo-samples the pixel took over from the previous frame (0 in frame 0)
    The arguments are checked at the call, before any device work.  samples_per_pixel of the cameras is
    not used."""
    if output not in ("linear", "rgb8"):
        raise ValueError(output)
    if precision not in _PRECISION:
        raise ValueError(precision)
    spp, feature_spp, seed_step = int(spp), int(feature_spp), int(seed_step)
    if spp < 2 or spp >= 2 ** 32:
        raise ValueError("spp must be in [2, 2^32) (the variance estimate needs two samples)")
    if feature_spp < 1 or feature_spp >= 2 ** 32:
        raise ValueError("feature_spp must be in [1, 2^32)")
    cams = list(cams)
    if not cams:
        raise ValueError("cams: at least one camera")
    if any(not isinstance(c, RtCamera) for c in cams):
        raise ValueError("cams: a list of RtCamera")
    if any((c.image_width, c.image_height) != (cams[0].image_width, cams[0].image_height) for c in cams):
        raise ValueError("cams: every camera must have the same image size")
    if cams[0].image_width == 0 or cams[0].image_height == 0:
        raise ValueError("cams: an empty image")
    if temporal is True:
        temporal = None
    if temporal is not None and temporal is not False and not isinstance(temporal, abi.RtTemporalParams):
        raise ValueError("temporal: temporal_params(), None or False")
    if denoise is not None and not isinstance(denoise, abi.RtDenoiseParams):
        raise ValueError("denoise: denoise_params() or None")
    return _sequence(cams, spheres, spp, feature_spp, temporal, denoise, seed_step, device, output, precision)


def _sequence(cams, spheres, spp, feature_spp, temporal, denoise, seed_step, device, output, precision):
    import torch

    W, H = cams[0].image_width, cams[0].image_height
    P = W * H
    n = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (RtSphere * n)(*spheres)
    r = DeviceRenderer(device)
    try:
        r.set_scene(arr)
        r.set_precision(precision)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            sets = []
            for _ in range(1 if temporal is False else 2):
                sets.append(dict(accum=torch.empty((P, 3), dtype=torch.float64, device=dev),
                                 m2=torch.empty(P, dtype=torch.float64, device=dev),
                                 counts=torch.zeros(P, dtype=torch.int32, device=dev),  # u32 on the device
                                 albedo=torch.empty((P, 3), dtype=torch.float64, device=dev),
                                 normal=torch.empty((P, 3), dtype=torch.float64, device=dev),
                                 depth=torch.empty(P, dtype=torch.float64, device=dev),
                                 hits=torch.empty(P, dtype=torch.int32, device=dev)))  # u32 on the device
            ptrs = [dict({k: v.data_ptr() for k, v in s.items()}, feature_samples=feature_spp) for s in sets]
            odt = torch.float64 if output == "linear" else torch.uint8
            out = torch.empty((2, H, W, 3), dtype=odt, device=dev)  # denoised, noisy
            var = torch.empty((H, W), dtype=torch.float64, device=dev)
            hist = torch.zeros((H, W), dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            prev_cam = None
            for f, cam0 in enumerate(cams):
                cam = RtCamera.from_buffer_copy(cam0)
                cam.seed = (cam0.seed + f * seed_step) % 2 ** 64
                k = f % len(sets)
                t, d = sets[k], ptrs[k]
                t["counts"].zero_()  # a new image: the gather pass starts every pixel from 0
                r.accumulate_pixels(cam, None, spp, d["accum"], d["m2"], d["counts"], stream_ptr=stream)
                r.features(cam, 0, feature_spp, d["albedo"], d["normal"], d["depth"], d["hits"], stream_ptr=stream)
                if temporal is not False and f > 0:
                    r.temporal_accumulate(cam, d, prev_cam, ptrs[1 - k], params=temporal,
                                          d_history_ptr=hist.data_ptr(), stream_ptr=stream)
                r.denoise(W, H, d["accum"], d["m2"], d["counts"], out[0].data_ptr(), d_albedo_ptr=d["albedo"],
                          d_normal_ptr=d["normal"], d_depth_ptr=d["depth"], d_hits_ptr=d["hits"],
                          feature_samples=feature_spp, params=denoise, output=output, d_var_out_ptr=var.data_ptr(),
                          stream_ptr=stream)
                r.resolve_counts(d["accum"], d["counts"], P, out[1].data_ptr(), output=output, stream_ptr=stream)
                res = out.cpu().numpy()  # waits for the stream
                frame = {"image": res[0], "noisy": res[1], "variance": var.cpu().numpy(),
                         "counts": t["counts"].cpu().numpy().view(np.uint32).reshape(H, W),
                         "history": hist.cpu().numpy().view(np.uint32).reshape(H, W)}
                r.sync()  # reports a failure the kernel recorded
                prev_cam = cam
                yield frame
    finally:
        r.close()


class DeviceRenderer:
    """Device-resident renderer for one GPU (rt_context): scene uploaded once, rows rendered into
    device memory (e.g. a torch tensor's data_ptr) on a caller-provided HIP stream."""

    def __init__(self, device=0):
        self.lib = load()
        self.ctx = C.c_void_p()
        check("rt_context_create", self.lib.rt_context_create(device, C.byref(self.ctx)))
        self.device = device
        self._pixels_keep = None  # the device copy of accumulate_pixels' last list

    def set_scene(self, spheres):
        n = len(spheres)
        check("rt_context_set_scene", self.lib.rt_context_set_scene(self.ctx, spheres, n))

    def render_rows_async(self, cam, d_out_ptr, row0=0, row_step=1, n_rows=None, output="linear",
                          d_stats_ptr=None, stream_ptr=None, out_stream_ptr=None, deferred=False):
        """out_stream_ptr: complete the output on that stream instead (rt_render_rows_async_split:
        direct mode's reduce pass runs there, over two per-sample buffers taken in turn, so it
        overlaps the next call's sample kernel on stream_ptr).  deferred (with out_stream_ptr):
        rt_render_rows_async_deferred — this call's output completes after the NEXT deferred call (or
        flush() / sync()), its reduce pass folded by that call's drained waves."""
        if n_rows is None:
            n_rows = (cam.image_height - row0 + row_step - 1) // row_step
        fmt = abi.RT_OUT_LINEAR_F64 if output == "linear" else abi.RT_OUT_RGB8
        if deferred:  # out_stream_ptr 0 is the HIP null stream (torch's default stream)
            check("rt_render_rows_async_deferred",
                  self.lib.rt_render_rows_async_deferred(self.ctx, C.byref(cam), fmt, row0, row_step, n_rows,
                                                         C.c_void_p(d_out_ptr), C.c_void_p(d_stats_ptr or 0),
                                                         C.c_void_p(stream_ptr or 0), C.c_void_p(out_stream_ptr or 0)))
            return
        if out_stream_ptr is not None:
            check("rt_render_rows_async_split",
                  self.lib.rt_render_rows_async_split(self.ctx, C.byref(cam), fmt, row0, row_step, n_rows,
                                                      C.c_void_p(d_out_ptr), C.c_void_p(d_stats_ptr or 0),
                                                      C.c_void_p(stream_ptr or 0), C.c_void_p(out_stream_ptr or 0)))
            return
        check("rt_render_rows_async",
              self.lib.rt_render_rows_async(self.ctx, C.byref(cam), fmt, row0, row_step, n_rows,
                                            C.c_void_p(d_out_ptr), C.c_void_p(d_stats_ptr or 0),
                                            C.c_void_p(stream_ptr or 0)))

    def accumulate(self, cam, d_accum_ptr, sample_begin, sample_count, row0=0, row_step=1, n_rows=None,
                   d_stats_ptr=None, stream_ptr=None):
        """rt_render_rows_accumulate: samples [sample_begin, sample_begin + sample_count) added, in
        sample order, to the unscaled per-pixel sums at d_accum_ptr (n_rows * W x 3 f64 on the device).
        sample_begin == 0 starts a new image (the buffer need not be initialised); any split of
        [0, n) into consecutive passes resolves to the bits of a one-pass render at n samples."""
        if n_rows is None:
            n_rows = (cam.image_height - row0 + row_step - 1) // row_step
        check("rt_render_rows_accumulate",
              self.lib.rt_render_rows_accumulate(self.ctx, C.byref(cam), row0, row_step, n_rows, sample_begin,
                                                 sample_count, C.c_void_p(d_accum_ptr or 0),
                                                 C.c_void_p(d_stats_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def resolve(self, d_accum_ptr, n_pixels, n_samples, d_out_ptr, output="linear", stream_ptr=None):
        """rt_accum_resolve: d_out = d_accum * (1 / n_samples), linear f64 or Color.toRgb bytes; the
        accumulator is left as it is (a preview; accumulation can go on)."""
        fmt = abi.RT_OUT_LINEAR_F64 if output == "linear" else abi.RT_OUT_RGB8
        check("rt_accum_resolve",
              self.lib.rt_accum_resolve(self.ctx, C.c_void_p(d_accum_ptr or 0), n_pixels, n_samples, fmt,
                                        C.c_void_p(d_out_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def features(self, cam, sample_begin, sample_count, d_albedo_ptr=None, d_normal_ptr=None, d_depth_ptr=None,
                 d_hits_ptr=None, row0=0, row_step=1, n_rows=None, stream_ptr=None):
        """rt_render_rows_features: the first hit of the camera rays of samples [sample_begin,
        sample_begin + sample_count), added in sample order to the unscaled per-pixel sums on the device:
        albedo and normal (n_rows * W x 3 f64 each), depth (n_rows * W f64), hits (n_rows * W u32).  A
        pointer left None skips that buffer.  sample_begin == 0 starts a new image (the buffers need not
        be initialised); any split of [0, n) into consecutive passes leaves the bits of one pass.  Always
        parity arithmetic, whatever set_precision says."""
        if n_rows is None:
            n_rows = (cam.image_height - row0 + row_step - 1) // row_step
        check("rt_render_rows_features",
              self.lib.rt_render_rows_features(self.ctx, C.byref(cam), row0, row_step, n_rows, sample_begin,
                                               sample_count, C.c_void_p(d_albedo_ptr or 0),
                                               C.c_void_p(d_normal_ptr or 0), C.c_void_p(d_depth_ptr or 0),
                                               C.c_void_p(d_hits_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def trace_rays(self, d_origins_ptr, d_directions_ptr, n_rays, t_min=1e-3, t_max=INF, d_index_ptr=None,
                   d_t_ptr=None, d_point_ptr=None, d_normal_ptr=None, d_front_ptr=None, d_intervals_ptr=None,
                   d_stats_ptr=None, ray_stride=3, stream_ptr=None):
        """rt_trace_rays: HittableList.hit of n_rays rays on the device, bit for bit.  Origins and
        directions are f64, ray q at [q * ray_stride + 0..2]; d_intervals_ptr (n x 2 f64) replaces
        (t_min, t_max) per ray.  Outputs, each skipped when None: index (n i32, -1: miss), t (n f64, inf:
        miss), point and normal (n x 3 f64), front (n u8).  d_stats_ptr: 2 x u64, incremented by {rays,
        rays answered by the list scan}.  Always parity arithmetic."""
        hits = abi.RtRayHits(d_index_ptr or None, d_t_ptr or None, d_point_ptr or None, d_normal_ptr or None,
                             d_front_ptr or None)
        check("rt_trace_rays",
              self.lib.rt_trace_rays(self.ctx, C.c_void_p(d_origins_ptr or 0), C.c_void_p(d_directions_ptr or 0),
                                     ray_stride, n_rays, t_min, t_max, C.c_void_p(d_intervals_ptr or 0),
                                     C.byref(hits), C.c_void_p(d_stats_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def occluded_rays(self, d_origins_ptr, d_ends_ptr, n_rays, t_min=1e-3, t_max=INF, d_occluded_ptr=None,
                      d_mask_ptr=None, d_intervals_ptr=None, d_stats_ptr=None, ray_stride=3, targets=False,
                      stream_ptr=None):
        """rt_occluded_rays: is ray q occluded (HittableList.hit true), for n_rays rays on the device.
        Rays and intervals as trace_rays; with targets=True d_ends_ptr holds end points and the direction
        is end - origin.  Outputs, each skipped when None: occluded (n u8, 1 / 0), mask (ceil(n / 64) u64,
        bit q & 63 of word q >> 6).  d_stats_ptr: 3 x u64, incremented by {rays, rays answered by the list
        scan, occluded rays}.  Always parity arithmetic."""
        check("rt_occluded_rays",
              self.lib.rt_occluded_rays(self.ctx, C.c_void_p(d_origins_ptr or 0), C.c_void_p(d_ends_ptr or 0),
                                        ray_stride, n_rays, t_min, t_max, C.c_void_p(d_intervals_ptr or 0),
                                        abi.OCCLUSION_TARGETS if targets else 0, C.c_void_p(d_occluded_ptr or 0),
                                        C.c_void_p(d_mask_ptr or 0), C.c_void_p(d_stats_ptr or 0),
                                        C.c_void_p(stream_ptr or 0)))

    def radiance_rays(self, d_origins_ptr, d_directions_ptr, n_rays, d_sum_ptr=None, sample_begin=0, sample_count=1,
                      bounce_max=50, seed=0xdeadbeef, ray_base=0, t_min=1e-3, t_max=INF, d_states_ptr=None,
                      d_stats_ptr=None, ray_stride=3, stream_ptr=None):
        """rt_radiance_rays: Camera.rayColor of n_rays rays on the device, bit for bit.  Rays as trace_rays.
        Samples [sample_begin, sample_begin + sample_count) of ray q, each on the stream
        rt_sample_key(seed, ray_base + q, s), are added in sample order to the unscaled sums d_sum_ptr
        (n x 3 f64; sample_begin == 0 overwrites, > 0 continues).  d_states_ptr (n x 4 u64): the one
        sample continues these Xoshiro256++ states instead (sample_count must be 1).  d_stats_ptr: 3 x
        u64, incremented by {paths, segments, segments answered by the list scan}.  Always parity
        arithmetic."""
        prm = abi.RtRadianceParams(seed=seed, ray_base=ray_base, sample_begin=sample_begin, sample_count=sample_count,
                                   bounce_max=bounce_max, reserved=0, t_min=t_min, t_max=t_max)
        check("rt_radiance_rays",
              self.lib.rt_radiance_rays(self.ctx, C.c_void_p(d_origins_ptr or 0), C.c_void_p(d_directions_ptr or 0),
                                        ray_stride, n_rays, C.byref(prm), C.c_void_p(d_states_ptr or 0),
                                        C.c_void_p(d_sum_ptr or 0), C.c_void_p(d_stats_ptr or 0),
                                        C.c_void_p(stream_ptr or 0)))

    def origin_bound(self):
        """rt_context_origin_bound: rays starting within it (max |o_k|) may use the tree; 0: the list walk."""
        b = C.c_double()
        check("rt_context_origin_bound", self.lib.rt_context_origin_bound(self.ctx, C.byref(b)))
        return b.value

    def reserve_origin_bound(self, bound):
        """rt_context_reserve_origin_bound: rebuilds the tree for ray origins up to `bound` (no result bit
        changes; a trained tree is dropped)."""
        check("rt_context_reserve_origin_bound", self.lib.rt_context_reserve_origin_bound(self.ctx, float(bound)))

    def _pixel_list(self, cam, pixels, n_pixels):
        """(device pointer, length) of a pixel list for accumulate_pixels.  None: every pixel.  An int is
        a raw device pointer to uint32 indices, taken on trust (n_pixels gives its length).  A host
        array / sequence or a torch tensor is validated first — every index in [0, W*H), no index
        twice — and, if it is not a 32-bit integer tensor on this device already, copied there."""
        wh = cam.image_width * cam.image_height
        if pixels is None:
            return 0, wh if n_pixels is None else int(n_pixels)
        if isinstance(pixels, int):
            if n_pixels is None:
                raise ValueError("a raw pixel-list pointer needs n_pixels")
            return pixels, int(n_pixels)
        import torch

        if isinstance(pixels, torch.Tensor):
            t = pixels.reshape(-1)
            if t.dtype not in (torch.int32, torch.int64):
                raise TypeError("pixel list: an int32 or int64 tensor")
        else:
            a = np.asarray(pixels).reshape(-1)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise TypeError("pixel list: integers")
            t = torch.from_numpy(a.astype(np.int64))
        n = t.numel()
        if n_pixels is not None and int(n_pixels) != n:
            raise ValueError("n_pixels differs from the list's length")
        if n:
            if int(t.min()) < 0 or int(t.max()) >= wh:
                raise ValueError("pixel list: an index outside [0, image_width * image_height)")
            if torch.unique(t).numel() != n:
                raise ValueError("pixel list: an index appears twice")
        dev = torch.device("cuda", self.device)
        if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
            t = t.to(device=dev, dtype=torch.int32).contiguous()
        self._pixels_keep = t  # alive until the next list replaces it (the pass is asynchronous)
        return t.data_ptr(), n

    def accumulate_pixels(self, cam, pixels, sample_count, d_accum_ptr, d_m2_ptr, d_counts_ptr, n_pixels=None,
                          d_stats_ptr=None, stream_ptr=None):
        """rt_render_pixels_accumulate: sample_count more samples for the listed pixels (`pixels`: None
        for every pixel, a host array or torch tensor of indices j*W + i — validated: in range, no
        duplicates — or a raw device pointer with n_pixels, taken on trust), each continuing at its own
        count d_counts[p]; their colours are added in sample order to d_accum[p] (W*H x 3 f64), their
        squared luminances to d_m2[p] (W*H f64, or None), and d_counts[p] (W*H u32) advances.  Every
        pixel then holds the sums of a one-pass render at its own count."""
        ptr, n = self._pixel_list(cam, pixels, n_pixels)
        if n == 0 and pixels is not None:
            return  # an empty list: nothing to do (a null pointer would mean every pixel)
        check("rt_render_pixels_accumulate",
              self.lib.rt_render_pixels_accumulate(self.ctx, C.byref(cam), C.c_void_p(ptr), n, sample_count,
                                                   C.c_void_p(d_accum_ptr or 0), C.c_void_p(d_m2_ptr or 0),
                                                   C.c_void_p(d_counts_ptr or 0), C.c_void_p(d_stats_ptr or 0),
                                                   C.c_void_p(stream_ptr or 0)))

    def select(self, d_accum_ptr, d_m2_ptr, d_counts_ptr, n_pixels, min_count, max_count, tolerance, floor,
               d_list_ptr, d_n_ptr, d_err_ptr=None, stream_ptr=None):
        """rt_accum_select: the pixels that need more samples (count < min_count, or count < max_count
        and not err <= tolerance; err = standard error of the mean luminance / max(mean, floor)), in
        ascending order into d_list (n_pixels u32), their number into d_n (one u32); d_err (n_pixels
        f64, optional) receives every pixel's err.  All device pointers; asynchronous."""
        check("rt_accum_select",
              self.lib.rt_accum_select(self.ctx, C.c_void_p(d_accum_ptr or 0), C.c_void_p(d_m2_ptr or 0),
                                       C.c_void_p(d_counts_ptr or 0), n_pixels, min_count, max_count, tolerance,
                                       floor, C.c_void_p(d_list_ptr or 0), C.c_void_p(d_n_ptr or 0),
                                       C.c_void_p(d_err_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def resolve_counts(self, d_accum_ptr, d_counts_ptr, n_pixels, d_out_ptr, output="linear", stream_ptr=None):
        """rt_accum_resolve_counts: d_out[p] = d_accum[p] * (1 / d_counts[p]) (0 without samples)."""
        fmt = abi.RT_OUT_LINEAR_F64 if output == "linear" else abi.RT_OUT_RGB8
        check("rt_accum_resolve_counts",
              self.lib.rt_accum_resolve_counts(self.ctx, C.c_void_p(d_accum_ptr or 0), C.c_void_p(d_counts_ptr or 0),
                                               n_pixels, fmt, C.c_void_p(d_out_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def denoise(self, width, height, d_accum_ptr, d_m2_ptr, d_counts_ptr, d_out_ptr, d_albedo_ptr=None,
                d_normal_ptr=None, d_depth_ptr=None, d_hits_ptr=None, feature_samples=0, params=None, output="linear",
                d_var_out_ptr=None, stream_ptr=None):
        """rt_denoise: the variance- and feature-guided à-trous filter over whole-image device buffers —
        the colour sums, squared-luminance sums and counts of accumulate_pixels, guided by the sums of
        features() at `feature_samples` samples (a pointer left None: that guide is 0) — into d_out
        (width * height x 3, linear f64 or rgb8) and, optionally, the filtered variance of the mean
        luminance into d_var_out (width * height f64).  params: denoise_params(), None for the defaults.
        The inputs are not modified; asynchronous."""
        fmt = abi.RT_OUT_LINEAR_F64 if output == "linear" else abi.RT_OUT_RGB8
        check("rt_denoise",
              self.lib.rt_denoise(self.ctx, width, height, C.c_void_p(d_accum_ptr or 0), C.c_void_p(d_m2_ptr or 0),
                                  C.c_void_p(d_counts_ptr or 0), C.c_void_p(d_albedo_ptr or 0),
                                  C.c_void_p(d_normal_ptr or 0), C.c_void_p(d_depth_ptr or 0),
                                  C.c_void_p(d_hits_ptr or 0), feature_samples,
                                  C.byref(params) if params is not None else None, fmt, C.c_void_p(d_out_ptr or 0),
                                  C.c_void_p(d_var_out_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def temporal_accumulate(self, cam, cur, cam_prev, prev, params=None, d_history_ptr=None, stream_ptr=None):
        """rt_temporal_accumulate: the previous frame's sums, reprojected through the two cameras and
        tested against the current frame's guides, merged into the current frame's sums as pseudo-samples.
        cur and prev: dicts of device pointers — accum, m2, counts (accumulate_pixels' buffers over every
        pixel), depth, hits and optionally albedo, normal (features()' buffers over all rows) — plus
        feature_samples.  cur is read and written, prev only read.  params: temporal_params(), None for the
        defaults.  d_history (W*H u32, optional) receives the pseudo-samples each pixel took over.
        Asynchronous."""
        frames = []
        for d in (cur, prev):
            extra = set(d) - {"accum", "m2", "counts", "albedo", "normal", "depth", "hits", "feature_samples"}
            if extra:
                raise TypeError(f"temporal_accumulate: no frame field {sorted(extra)[0]!r}")
            frames.append(abi.RtTemporalFrame(**{k: (int(v or 0) if k == "feature_samples" else (v or None))
                                                 for k, v in d.items()}))
        check("rt_temporal_accumulate",
              self.lib.rt_temporal_accumulate(self.ctx, C.byref(cam), C.byref(frames[0]), C.byref(cam_prev),
                                              C.byref(frames[1]), C.byref(params) if params is not None else None,
                                              C.c_void_p(d_history_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def flush(self):
        """Runs a pending deferred reduce pass (rt_context_flush)."""
        check("rt_context_flush", self.lib.rt_context_flush(self.ctx))

    def fold_pending(self):
        """True if the last deferred call left its output pending (its reduce pass not yet run)."""
        v = C.c_int()
        check("rt_context_fold_pending", self.lib.rt_context_fold_pending(self.ctx, C.byref(v)))
        return bool(v.value)

    def sync(self):
        """Waits for the last render; raises if the kernel recorded a failure."""
        check("rt_context_sync", self.lib.rt_context_sync(self.ctx))

    def set_precision(self, precision):
        """"f64" (parity kernel, default) or "f32" (fast mode) for later renders."""
        check("rt_context_set_precision", self.lib.rt_context_set_precision(self.ctx, _PRECISION[precision]))

    def kernel_name(self):
        return self.lib.rt_kernel_name(self.ctx).decode()

    def tree_info(self):
        """The walk the next render uses: {"bvh", "nodes", "leaves", "depth", "always", "trained"}."""
        info = (C.c_uint32 * 6)()
        check("rt_context_tree_info", self.lib.rt_context_tree_info(self.ctx, info))
        return dict(zip(("bvh", "nodes", "leaves", "depth", "always", "trained"), [int(x) for x in info]))

    def workspace_bytes(self):
        """Device bytes the context's render workspace holds (rt.h "Workspace")."""
        b = C.c_uint64()
        check("rt_context_workspace_bytes", self.lib.rt_context_workspace_bytes(self.ctx, C.byref(b)))
        return b.value

    def enable_timing(self, enable=True):
        check("rt_context_enable_timing", self.lib.rt_context_enable_timing(self.ctx, int(enable)))

    def enable_profile(self, enable=True):
        """Instrumented kernels: the stats buffer passed to render_rows_async must hold 32 u64."""
        check("rt_context_enable_profile", self.lib.rt_context_enable_profile(self.ctx, int(enable)))

    def kernel_times(self):
        """(sample_kernel_ms, reduce_kernel_ms) of the last render call (HIP events)."""
        a, b = C.c_double(), C.c_double()
        check("rt_context_kernel_times", self.lib.rt_context_kernel_times(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_times_total(self):
        """(sample_kernel_ms, reduce_kernel_ms, launches) summed since timing was enabled."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        check("rt_context_kernel_times_total",
              self.lib.rt_context_kernel_times_total(self.ctx, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def close(self):
        """rt_context_destroy: runs a pending deferred reduce pass and waits for every launch first."""
        if self.ctx:
            ctx, self.ctx = self.ctx, C.c_void_p()
            check("rt_context_destroy", self.lib.rt_context_destroy(ctx))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PPM:
    """ppm.zig:5-61: framebuffer + P6 (saveBinary) and P3 (save) writers."""

    def __init__(self, width, height, pixels):
        self.width, self.height, self.pixels = width, height, pixels

    def toRgb(self):
        if self.pixels.dtype == np.uint8:
            return self.pixels
        return to_rgb8(self.pixels)

    def encodeBinary(self):
        return encode_p6(self.toRgb(), self.width, self.height)

    def saveBinary(self, path):
        rgb = np.ascontiguousarray(self.toRgb())
        check("rt_ppm_save_p6", load().rt_ppm_save_p6(
            path.encode(), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), self.width, self.height))

    def encode(self):
        return encode_p3(self.toRgb(), self.width, self.height)

    def save(self, path):
        """PPM.save (ppm.zig:25-39): the P3 ASCII file."""
        rgb = np.ascontiguousarray(self.toRgb())
        check("rt_ppm_save_p3", load().rt_ppm_save_p3(
            path.encode(), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), self.width, self.height))


def to_rgb8(linear):
    """Color.toRgb (color.zig:63-80) over an (..., 3) f64 array (host C++)."""
    lin = np.ascontiguousarray(linear, dtype=np.float64)
    n = lin.size // 3
    rgb = np.zeros(lin.shape, np.uint8)
    check("rt_color_to_rgb8", load().rt_color_to_rgb8(
        lin.ctypes.data_as(C.POINTER(C.c_double)), n, 3, rgb.ctypes.data_as(C.POINTER(C.c_uint8))))
    return rgb


def encode_p6(rgb, width, height):
    lib = load()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    size = lib.rt_ppm_p6_size(width, height)
    buf = (C.c_uint8 * size)()
    check("rt_ppm_encode_p6", lib.rt_ppm_encode_p6(rgb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   width, height, buf, size))
    return bytes(buf)


def encode_p3(rgb, width, height):
    lib = load()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    ptr = rgb.ctypes.data_as(C.POINTER(C.c_uint8))
    size = lib.rt_ppm_p3_size(ptr, width, height)
    buf = (C.c_uint8 * size)()
    check("rt_ppm_encode_p3", lib.rt_ppm_encode_p3(ptr, width, height, buf, size))
    return bytes(buf)


def release_cached_contexts():
    """Frees rt_render's per-device cached contexts (the next render creates them again)."""
    check("rt_release_cached_contexts", load().rt_release_cached_contexts())


def sample_key(seed, pixel, sample):
    return load().rt_sample_key(seed, pixel, sample)


# ---- presets (BASELINE.json configs) --------------------------------------------------------------
def final_scene_camera(width=1200, aspect_ratio=1.5, spp=500, seed=0xDEADBEEF, bounce_max=50):
    """main.zig:20-31 preset on the final random-sphere scene (configs 4/5, and the golden test
    at width 400, aspect 16/9, spp 10)."""
    scene = Scene.init(seed).generateWorld()
    return (Camera.builder(width, aspect_ratio).setScene(scene).setDefocusAngle(0.6)
            .setFocusDist(10).setViewport((13, 2, 3), (0, 0, 0), 20).setSamplesPerPixel(spp)
            .setBounceMax(bounce_max).build())


def chapter13_camera(width=1200, aspect_ratio=16.0 / 9.0, spp=500, seed=0xDEADBEEF):
    """Config 3: generateChapter13 (Scene.zig:136-182) with the book's chapter-13 camera."""
    scene = Scene.init(seed).generateChapter13()
    return (Camera.builder(width, aspect_ratio).setScene(scene).setDefocusAngle(10.0)
            .setFocusDist(3.4).setViewport((-2, 2, 1), (0, 0, -1), 20).setSamplesPerPixel(spp)
            .build())


def chapter9_camera(width=400, aspect_ratio=16.0 / 9.0, spp=100, seed=0xDEADBEEF):
    """Config 2: two Lambertian spheres (albedo 0.5), vFov 90, no defocus, focus 1."""
    scene = Scene.init(seed)
    scene.add((0, 0, -1), 0.5, abi.RT_LAMBERTIAN, albedo=(0.5, 0.5, 0.5))
    scene.add((0, -100.5, -1), 100, abi.RT_LAMBERTIAN, albedo=(0.5, 0.5, 0.5))
    return (Camera.builder(width, aspect_ratio).setScene(scene).setDefocusAngle(0.0)
            .setFocusDist(1.0).setViewport((0, 0, 0), (0, 0, -1), 90).setSamplesPerPixel(spp)
            .build())

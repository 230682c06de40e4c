"""What the radiance-query tests share (include/rt.h rt_radiance_rays): the per-ray
reference.  A helper module, not a test: pytest does not rewrite its asserts, so every assert here
carries its own message.

The C oracle renders pixels; it has no entry point for "rayColor of this ray on this stream".  So the
reference is restated here in plain Python floats — IEEE f64, one rounding per operation, no
contraction — and in Python integers for the generator:

  Stream      Xoshiro256++ and Random.float(f64), with the state after any number of float draws;
  ray_color   Camera.rayColor (camera.zig:148-183) with Material.scatter, on oracle.world_hit,
              oracle.reflect and oracle.refract for the hits and the two vector formulas.

tests/test_radiance_model.py anchors both to the C oracle (its streams, oracle.render_b and
oracle.accumulate_b, bit for bit); tests/test_gpu_radiance.py then holds the device to them.  getRay
is gpu_support.get_ray; camera_rays feeds it from a Stream and reports the state it leaves behind."""
import collections
import math

import numpy as np

from gpu_support import get_ray, same_bits
from rtzig.abi import RT_LAMBERTIAN, RT_METAL

INF, NAN = math.inf, math.nan
MASK = (1 << 64) - 1

# bounce_max, t_min, t_max: Camera.bounceMax and Scene.interval
Params = collections.namedtuple("Params", "bounce_max t_min t_max")


# ---- the generator -------------------------------------------------------------------------------------
def rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & MASK


def clz64(w):
    return 64 - w.bit_length()


def splitmix(s):
    """SplitMix64.next: (the new state, the output)."""
    s = (s + 0x9E3779B97F4A7C15) & MASK
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return s, z ^ (z >> 31)


class Stream:
    """Xoshiro256++ (std.Random.DefaultPrng) on Python integers."""

    def __init__(self, state):
        self.s = [int(x) & MASK for x in state]
        assert len(self.s) == 4, "a Xoshiro256++ state has four words"

    @classmethod
    def from_key(cls, key):
        """DefaultPrng.init(key): the four words of SplitMix64 seeded with the key."""
        sm, words = int(key) & MASK, []
        for _ in range(4):
            sm, w = splitmix(sm)
            words.append(w)
        return cls(words)

    def copy(self):
        return Stream(self.s)

    def state(self):
        return list(self.s)

    def next_u64(self):
        s0, s1, s2, s3 = self.s
        r = (rotl((s0 + s3) & MASK, 23) + s0) & MASK
        t = (s1 << 17) & MASK
        s2 ^= s0
        s3 ^= s1
        s1 ^= s2
        s0 ^= s3
        s2 ^= t
        s3 = rotl(s3, 45)
        self.s = [s0, s1, s2, s3]
        return r

    def float64(self):
        """Random.float(f64): 52 mantissa bits of one word, the exponent from its leading zeros; with 12
        or more, further words extend the exponent (capped at 1022)."""
        rnd = self.next_u64()
        lz = clz64(rnd)
        if lz >= 12:
            lz = 12
            while True:
                add = clz64(self.next_u64())
                lz += add
                if add != 64:
                    break
                if lz >= 1022:
                    lz = 1022
                    break
        bits = ((1022 - lz) << 52) | (rnd & ((1 << 52) - 1))
        return float(np.array(bits, np.uint64).view(np.float64))

    def after_floats(self, k):
        """The state after k more float draws; this stream does not move."""
        c = self.copy()
        for _ in range(k):
            c.float64()
        return c.state()


class Draws:
    """The float draws of a stream as an indexable sequence, drawn on demand (gpu_support.get_ray reads
    u[0], u[1], ...); `used` is the number of draws read."""

    def __init__(self, stream):
        self.stream, self.u, self.used = stream.copy(), [], 0

    def __getitem__(self, k):
        while len(self.u) <= k:
            self.u.append(self.stream.float64())
        self.used = max(self.used, k + 1)
        return self.u[k]


def pixel_stream(oracle, seed, ident, sample):
    """The stream of rt_sample_key(seed, ident, sample): a pixel's, or a ray's id in the pixel's place."""
    return Stream.from_key(oracle.sample_key(seed, ident, sample))


def camera_rays(oracle, cam, sample=0):
    """getRay of every pixel's stream at `sample`: (origins (P, 3), directions (P, 3), states (P, 4) u64 —
    each stream after getRay's draws, where rayColor takes it over)."""
    W, H = cam.image_width, cam.image_height
    O, D, S = np.zeros((H * W, 3)), np.zeros((H * W, 3)), np.zeros((H * W, 4), np.uint64)
    for p in range(H * W):
        j, i = divmod(p, W)
        st = pixel_stream(oracle, cam.seed, p, sample)
        u = Draws(st)
        O[p], D[p] = get_ray(cam, i, j, u)
        S[p] = st.after_floats(u.used)
    return O, D, S


# ---- IEEE operations Python raises on ------------------------------------------------------------------
def fdiv(a, b):
    """a / b as IEEE 754 gives it (Python raises on a zero divisor)."""
    if b != 0:
        return a / b
    if a != a or a == 0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def fsqrt(x):
    """sqrt(x) as IEEE 754 gives it: NaN below zero (-0.0 stays), NaN for NaN."""
    if x != x or x < 0:
        return NAN
    return math.sqrt(x)


def fmin(a, b):
    """C's fmin: the other operand when one is NaN."""
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


# ---- Vec (vec.zig) -------------------------------------------------------------------------------------
def add(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def mul(a, b):
    return [a[0] * b[0], a[1] * b[1], a[2] * b[2]]


def neg(a):
    return [-a[0], -a[1], -a[2]]


def muls(a, s):
    return [a[0] * s, a[1] * s, a[2] * s]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # @reduce(.Add): (x + y) + z


def unit(a):
    return muls(a, fdiv(1.0, fsqrt(dot(a, a))))  # divScalar(v, len) = v * (1 / len)


def near_zero(v):
    return v[0] < 1e-8 and v[1] < 1e-8 and v[2] < 1e-8  # no abs (vec.zig:26-29)


def random_unit_vec(g):
    """Vec.randomUnitVec (vec.zig:71-80): rejection, then true divisions."""
    while True:
        p = [-1.0 + 2.0 * g.float64() for _ in range(3)]  # randomDoubleRange(-1, 1) = -1 + (1 - -1) * u
        ls = dot(p, p)
        if 1e-160 < ls <= 1:
            l = math.sqrt(ls)
            return [p[0] / l, p[1] / l, p[2] / l]


def pow5(x):
    """std.math.pow(f64, x, 5) as the oracle states it (rt_oracle.c zig_pow5)."""
    if x == 1.0:
        return 1.0
    if x == 0.0:
        return x
    x2 = x * x
    return x * (x2 * x2)


# ---- rayColor ------------------------------------------------------------------------------------------
def ray_color(oracle, spheres, ray, params, stream, on_segment=None):
    """Camera.rayColor (camera.zig:148-183) of `ray` = (origin, direction), drawing from `stream` (which
    moves): (colour [r, g, b], segments — the world.hit calls).  on_segment(origin, direction) is called
    for every segment before its world.hit."""
    orig, d = [float(x) for x in ray[0]], [float(x) for x in ray[1]]
    att = [1.0, 1.0, 1.0]
    segments = 0
    for _ in range(params.bounce_max):
        segments += 1
        if on_segment is not None:
            on_segment(orig, d)
        k, t = oracle.world_hit(spheres, orig, d, params.t_min, params.t_max)
        if k < 0:
            a = 0.5 * (unit(d)[1] + 1.0)  # sky (camera.zig:171-177)
            sky = add(muls([1.0, 1.0, 1.0], 1.0 - a), muls([0.5, 0.7, 1.0], a))
            return mul(att, sky), segments
        s = spheres[k]
        radius = s.radius if s.radius > 0 else 0.0  # Sphere.init: @max(0, r)
        # hit record (sphere.zig:44-53)
        p = add(orig, muls(d, t))
        outward = muls(sub(p, list(s.center)), fdiv(1.0, radius))
        front = dot(d, outward) < 0
        nrm = outward if front else neg(outward)
        if s.material == RT_LAMBERTIAN:  # material.zig:27-39
            nd = add(nrm, random_unit_vec(stream))
            if near_zero(nd):
                nd = nrm
            att = mul(att, list(s.albedo))
        elif s.material == RT_METAL:  # material.zig:55-68
            refl = unit(oracle.reflect(d, nrm))
            nd = add(refl, muls(random_unit_vec(stream), s.fuzz))
            if not dot(nd, nrm) > 0:
                return [0.0, 0.0, 0.0], segments
            att = mul(att, list(s.albedo))
        else:  # dielectric, material.zig:82-110
            ri = fdiv(1.0, s.refraction_index) if front else s.refraction_index
            ud = unit(d)
            cos_t = fmin(dot(neg(ud), nrm), 1.0)
            sin_t = fsqrt(1.0 - cos_t * cos_t)
            cannot = ri * sin_t > 1.0
            r0 = fdiv(1 - ri, 1 + ri)
            r0 = r0 * r0
            approx = r0 + (1 - r0) * pow5(1 - cos_t)
            # short-circuit `or`: the stream is drawn only when refraction is possible
            if cannot or approx > stream.float64():
                nd = oracle.reflect(ud, nrm)
            else:
                nd = oracle.refract(ud, nrm, ri)
        orig, d = p, nd
    return [0.0, 0.0, 0.0], segments


def radiance_ref(oracle, spheres, O, D, params, seed, ray_base=0, sample_begin=0, sample_count=1, sums=None,
                 states=None, on_segment=None):
    """rt_radiance_rays on the CPU: (sums (n, 3), segments).  Sample s of ray q runs on the stream of
    (seed, ray_base + q, s), or — `states` — its one sample continues states[q].  sample_begin == 0 starts
    from 0, else from `sums` (not modified)."""
    n = len(O)
    out = np.zeros((n, 3)) if sample_begin == 0 else np.array(sums, np.float64)
    assert out.shape == (n, 3), "sums must be (n, 3)"
    assert states is None or sample_count == 1, "states need sample_count == 1"
    segments = 0
    for q in range(n):
        acc = [float(x) for x in out[q]]
        for s in range(sample_begin, sample_begin + sample_count):
            g = Stream(states[q]) if states is not None else pixel_stream(oracle, seed, ray_base + q, s)
            col, segs = ray_color(oracle, spheres, (O[q], D[q]), params, g, on_segment)
            acc = add(acc, col)
            segments += segs
        out[q] = acc
    return out, segments


def same_or_nan(got, want):
    """The comparison rule: a component that is NaN in the reference is NaN on the device, and every
    other component has the reference's bits."""
    one_nan = lambda a: np.where(np.isnan(a), NAN, np.asarray(a, np.float64))  # every NaN the same bits
    return same_bits(one_nan(got), one_nan(want))

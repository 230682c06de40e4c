"""Synthetic accumulator values for the resolve kernels and the denoiser's sink: the inputs at which
Color.toRgb (color.zig:63-80: sqrt, clamp to [0, 0.999], trunc(256 x)) changes its byte, and the
values no render produces.  Shared by tests/test_gpu_domain.py and tests/test_gpu_denoise.py.  A
helper module, not a test."""
import numpy as np

INF = np.inf


def channel_values(finite_only=False):
    """The values one channel is given.  The byte boundaries sit at (k/256)^2, k = 1..255: whether the
    neighbour below rounds back up to byte k under sqrt depends on a correctly rounded sqrt.  Then
    the clamp's corner 0.999^2 and 1.0 with their neighbours, and zero, negative, huge, subnormal,
    infinite and NaN inputs."""
    sq = (np.arange(1, 256) / 256.0) ** 2
    vals = [sq, np.nextafter(sq, 0.0), np.nextafter(sq, 2.0)]
    for x in (0.999 * 0.999, 1.0):
        vals.append(np.array([np.nextafter(x, 0.0), x, np.nextafter(x, 2.0)]))
    vals.append(np.array([0.0, -0.0, -0.3, 1.5, 1e308, 5e-324, 1e-320]))
    if not finite_only:
        vals.append(np.array([INF, np.nan]))
    return np.concatenate(vals)


def pixels(n_pixels, repeat=1, finite_only=False):
    """(n_pixels, 3) f64: pixel i, channel c holds value (i // repeat + 263 * c) mod V, so the three
    channels of a pixel differ and every channel meets every value once i // repeat has gone through
    all V of them."""
    v = channel_values(finite_only)
    i = np.arange(n_pixels) // repeat
    return np.stack([v[(i + 263 * c) % len(v)] for c in range(3)], 1)


def same_bits_or_nan(got, want):
    """Bit-equal f64 arrays, a NaN compared by position (IEEE leaves its payload open)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)))

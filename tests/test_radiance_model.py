"""The per-ray reference of the radiance tests (tests/radiance_support.py) against the C oracle, on the
CPU: the Python generator against the oracle's streams, and getRay + ray_color on every (pixel,
sample) stream against oracle.render_b at one sample per pixel — where pixelSamplesScale is 1.0, so a
pixel is 0 + rayColor — and against oracle.accumulate_b for three samples summed in order.  Everything
is bit-equal; the segment counts equal the oracle's `rays`."""
import numpy as np
import pytest

import fast_scenes
import rtzig
from gpu_support import get_ray, same_bits
from radiance_support import Draws, Params, Stream, camera_rays, pixel_stream, radiance_ref, ray_color


# ---- the generator -------------------------------------------------------------------------------------
KEYS = [0, 1, 0xDEADBEEF, (1 << 63) + 12345, (1 << 64) - 1]


@pytest.mark.parametrize("key", KEYS)
def test_seeded_state_words_and_floats_equal_the_oracles(oracle, key):
    st = Stream.from_key(key)
    assert st.state() == [int(x) for x in oracle.seed_state(key)]
    words = _take(st.copy(), 300, "next_u64")
    assert words == [int(x) for x in oracle.random_u64_state(np.array(st.state(), np.uint64), 300)]
    assert words == [int(x) for x in oracle.random_u64(key, 300)]
    floats = np.array(_take(st.copy(), 300, "float64"))
    assert same_bits(floats, oracle.random_doubles_state(np.array(st.state(), np.uint64), 300))
    assert same_bits(floats, oracle.random_doubles(key, 300))


def _take(stream, n, what):
    return [getattr(stream, what)() for _ in range(n)]


def test_rare_floats_pull_further_words(oracle):
    """A word with 12 or more leading zeros extends the exponent from the next words: states whose next
    word is small, found by search, and one built to give zero words."""
    found = 0
    for key in range(1 << 40, (1 << 40) + 40000):
        st = Stream.from_key(key)
        if st.copy().next_u64() >> 52:
            continue
        found += 1
        got = np.array(_take(st.copy(), 8, "float64"))
        assert same_bits(got, oracle.random_doubles_state(np.array(st.state(), np.uint64), 8)), key
    assert found >= 3, "the search found %d rare first words" % found
    for state in ([0, 0, 0, 1], [1, 0, 0, 0], [0, 1 << 40, 0, 0]):  # runs of zero and tiny words
        st = Stream(state)
        got = np.array(_take(st.copy(), 16, "float64"))
        assert same_bits(got, oracle.random_doubles_state(np.array(state, np.uint64), 16)), state


@pytest.mark.parametrize("k", [0, 1, 2, 5, 64])
def test_state_after_k_draws_continues_as_the_tail(oracle, k):
    st = Stream.from_key(0xC0FFEE + k)
    whole = oracle.random_doubles_state(np.array(st.state(), np.uint64), k + 50)
    later = st.after_floats(k)
    assert st.state() == Stream.from_key(0xC0FFEE + k).state(), "after_floats moved the stream"
    assert same_bits(oracle.random_doubles_state(np.array(later, np.uint64), 50), whole[k:])
    assert same_bits(np.array(_take(Stream(later), 50, "float64")), whole[k:])


def test_draws_counts_what_get_ray_read(oracle):
    cam = fast_scenes.with_camera(rtzig.chapter13_camera(width=8, spp=1)).cam  # defocus: 2 + 2 per trip
    used = set()
    for p in range(cam.image_width * cam.image_height):
        u = Draws(pixel_stream(oracle, cam.seed, p, 0))
        get_ray(cam, p % cam.image_width, p // cam.image_width, u)
        assert u.used >= 4 and u.used % 2 == 0
        used.add(u.used)
    assert len(used) > 1, "no pixel needed a second rejection trip"


# ---- rayColor against the renderer ---------------------------------------------------------------------
def model_image(oracle, cam, spheres, sample=0):
    """(the (H, W, 3) image of 0 + rayColor(getRay) on every pixel's stream at `sample`, segments)."""
    O, D, S = camera_rays(oracle, cam, sample)
    prm = Params(cam.bounce_max, cam.t_min, cam.t_max)
    out, segs = radiance_ref(oracle, spheres, O, D, prm, cam.seed, states=S)
    return out.reshape(cam.image_height, cam.image_width, 3), segs


def materials32():
    """fast_scenes.materials()'s scene and view at 32 x 18."""
    scene = fast_scenes.materials().scene
    return (rtzig.Camera.builder(32, 16 / 9).setScene(scene).setDefocusAngle(2.0).setFocusDist(1.5)
            .setViewport((0, 0.3, 0.5), (0, 0, -1), 70).setSamplesPerPixel(1).build())


def cameras():
    ch13 = lambda **kw: fast_scenes.with_camera(rtzig.chapter13_camera(width=24, spp=1), **kw)
    final = lambda depth, **kw: fast_scenes.with_camera(fast_scenes.final(depth, width=24), **kw)
    return {
        "chapter13": ch13,                                    # all three materials, the list walk, defocus 10
        "chapter13_d2": lambda: ch13(bounce_max=2),
        "final_d1": lambda: final(1),
        "final_d2": lambda: final(2),
        "final_d50": lambda: final(50),                       # 24 x 16, defocus 0.6
        "final_d50_pinhole": lambda: final(50, defocus_angle=0.0),
        "materials": materials32,                             # fuzz > 1 absorption, zero radius, inside glass
    }


@pytest.mark.parametrize("name", list(cameras()))
def test_get_ray_and_ray_color_equal_render_b_at_one_sample(oracle, name):
    cam = cameras()[name]()
    c, world = cam.cam, cam.scene.world
    assert c.samples_per_pixel == 1 and c.pixel_samples_scale == 1.0
    ref, rays = oracle.render_b(c, world, threads=4)
    got, segs = model_image(oracle, c, world)
    assert same_bits(got, ref), "%d of %d pixels differ" % (int((got != ref).any(axis=2).sum()), got.size // 3)
    assert segs == rays
    assert np.isfinite(ref).all() and (ref > 0).any()


def test_three_samples_summed_in_order_equal_accumulate_b(oracle):
    cam = fast_scenes.final(50, width=24)
    c, world = cam.cam, cam.scene.world
    prm = Params(c.bounce_max, c.t_min, c.t_max)
    sums, segs = np.zeros((c.image_height * c.image_width, 3)), 0
    for s in range(3):  # one call per sample, each continuing the sums: sum = sum + colour
        O, D, S = camera_rays(oracle, c, s)
        sums, n = radiance_ref(oracle, world, O, D, prm, c.seed, sample_begin=s, sums=sums, states=S)
        segs += n
    ref, rays = oracle.accumulate_b(c, world, 0, 3, threads=4)
    assert same_bits(sums.reshape(ref.shape), ref) and segs == rays
    # and continuing the oracle's own first sample
    first, r1 = oracle.accumulate_b(c, world, 0, 1, threads=4)
    rest, r2 = oracle.accumulate_b(c, world, 1, 2, sums=first, threads=4)
    assert same_bits(rest, ref) and r1 + r2 == rays


def test_keyed_streams_are_the_pixel_streams_with_the_ray_id_in_the_pixels_place(oracle):
    """radiance_ref's keyed mode: sample s of ray q runs on the stream of (seed, ray_base + q, s), and the
    colours are added in sample order — the same as calling ray_color by hand on those streams."""
    final = fast_scenes.final(50, width=24)
    cam, world = final.cam, final.scene.world
    prm = Params(cam.bounce_max, cam.t_min, cam.t_max)
    O, D, _ = camera_rays(oracle, cam, 0)
    O, D = O[24:48], D[24:48]
    keyed, segs = radiance_ref(oracle, world, O, D, prm, cam.seed, ray_base=24, sample_count=2)
    by_hand, n = np.zeros((24, 3)), 0
    for q in range(24):
        for s in range(2):
            col, k = ray_color(oracle, world, (O[q], D[q]), prm, pixel_stream(oracle, cam.seed, 24 + q, s))
            by_hand[q] = [by_hand[q][c] + col[c] for c in range(3)]
            n += k
    assert same_bits(keyed, by_hand) and segs == n
    assert prm.bounce_max == 50 and segs > 2 * 24

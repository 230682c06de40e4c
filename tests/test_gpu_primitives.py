"""The kernel's hand-written f64 primitives (csrc/rt_device.h, csrc/rt_leaf_filter.h) value by value,
through the probe library (tests/hip/rt_probe.hip): sqrt_g, unit, the scatter finish, RayDiv, reflect,
refract, range_pm1, sample_key, the Xoshiro256++ draw and Random.float in both instruction forms, and the
leaf filter.  Every result is compared bit for bit with a correctly rounded numpy reference or with the
oracle's stream (tests/probe_support.py); the inputs sit on the guards, on rounding midpoints and in
single lanes of otherwise ordinary waves, where a whole render never puts them.  The f32 fast mode's bits
are unspecified and not probed."""
import numpy as np
import pytest

import probe_support as ps

pytestmark = pytest.mark.gpu
U64 = np.uint64
LAYOUTS = ("order", "one_special", "waves")


def check(op, ref, *cols):
    got = ps.run(op, *cols)
    want = np.atleast_2d(ref)
    bad = ps.mismatches(got, want)
    assert len(bad) == 0, f"{op}: " + ps.describe(bad, got, want, *cols)
    return got


# ---- division and sqrt, in the three lane layouts ------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_raydiv_is_the_correctly_rounded_division(layout):
    a, x = ps.div_layouts()[layout]
    check("raydiv", ps.div_ref(a, x), a, x)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sqrt_g_is_the_correctly_rounded_sqrt(layout):
    (x,) = ps.sqrt_layouts()[layout]
    check("sqrt", ps.sqrt_ref(x), x)


def test_control_mul_by_reciprocal_is_seen_to_differ():
    """x * (1.0 / a) on the device equals numpy's same expression, and differs from x / a in at least
    20% of the near-representable and near-midpoint elements: the pipeline resolves one ulp."""
    (a1, x1), (a2, x2) = ps.div_near_representable(), ps.div_near_midpoint()
    a, x = np.concatenate([a1, a2]), np.concatenate([x1, x2])
    got = check("mul_rcp", ps.mul_rcp_ref(a, x), a, x)
    differ = np.mean(got[0].view(np.int64) != ps.div_ref(a, x).view(np.int64))
    print(f"control differs from the division in {differ:.3f}")
    assert differ >= 0.20


# ---- vectors -------------------------------------------------------------------------------------------------
def test_unit():
    v = ps.unit_inputs()
    check("unit", ps.unit_ref(v), *v)


def test_unit_of_accepted_point(oracle):
    p = ps.unit_accepted_inputs(oracle)
    check("unit_accepted", ps.unit_accepted_ref(p), *p)


def test_reflect_and_refract():
    v, n, eta, _ = ps.refract_inputs()
    check("reflect", ps.reflect_ref(v, n), *v, *n)
    check("refract", ps.refract_ref(v, n, eta), *v, *n, eta)


def test_range_pm1(oracle):
    u = ps.range_pm1_inputs(oracle)
    check("range_pm1", ps.range_pm1_ref(u), u)


# ---- RNG -----------------------------------------------------------------------------------------------------
FORMS = ("lean", "full")  # RngT<true> (the shipped kernels) and RngT<false> (the instrumented ones)


def same_words(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} words differ, first at (step, lane) {bad[0].tolist()}: " \
                          f"device {int(got[tuple(bad[0])]):#018x} reference {int(want[tuple(bad[0])]):#018x}"


@pytest.fixture(scope="module")
def keyed(oracle):
    """4096 (seed, pixel, sample) cases and further keys with a rare word early on: their keys, states,
    words and Random.float draws from the oracle, computed once."""
    seeds, pix, smp = ps.key_cases()
    keys = np.array([oracle.sample_key(int(s), int(p), int(m)) for s, p, m in zip(seeds, pix, smp)], U64)
    all_keys = np.concatenate([keys, ps.rare_keys(oracle)])
    states = np.array([oracle.seed_state(int(k)) for k in all_keys])
    words = np.array([oracle.random_u64(int(k), 64) for k in all_keys])
    doubles = np.array([oracle.random_doubles(int(k), 64) for k in all_keys]).view(U64)
    return dict(seeds=seeds, pix=pix, smp=smp, keys=keys, all_keys=all_keys, states=states, words=words, doubles=doubles)


def test_sample_key(keyed):
    got = ps.run("sample_key", keyed["seeds"], keyed["pix"], keyed["smp"])
    same_words(got, keyed["keys"][None, :], "sample_key")


def test_seeded_words(keyed):
    got = ps.run("seed_words", keyed["all_keys"], k=64)
    same_words(got, keyed["words"].T, "Rng::seed + next()")
    assert ps.is_rare(keyed["words"]).any(axis=1).sum() >= 128, "streams with a rare word are among them"


@pytest.mark.parametrize("form", FORMS)
def test_seeded_streams_from_their_states(keyed, form):
    st = keyed["states"]
    cols = [np.ascontiguousarray(st[:, j]) for j in range(4)] + [ps.draw_masks("all", len(st), 64)]
    same_words(ps.run(f"state_words_{form}", *cols, k=64), keyed["words"].T, "next()")
    same_words(ps.run(f"state_uniform_{form}", *cols, k=64), keyed["doubles"].T, "Random.float")


@pytest.fixture(scope="module")
def injected(oracle):
    """The deep-path states alone (whole waves of them) and one per wave at lane 0, 31, 32, 63 among
    ordinary states, with the oracle's streams of every lane: 32 steps, so up to 32 draws."""
    deep, _ = ps.deep_states()
    special = tuple(np.ascontiguousarray(deep[:, j]) for j in range(4))
    ordinary = tuple(np.ascontiguousarray(c) for c in ps.ordinary_states(1024).T)
    planes, at = ps.one_special_lane(ordinary, special)
    alone = ps.whole_waves(special)
    states = np.stack([np.concatenate([p, q]) for p, q in zip(planes, alone)], axis=1)
    assert sorted(set(at % 64)) == list(ps.LANES), "every special lane position"
    # equal states share their streams (the ordinary ones repeat from wave to wave)
    uniq, inv = np.unique(states, axis=0, return_inverse=True)
    w, d = ps.state_streams(oracle, uniq, 32)
    return dict(states=states, words=w[inv.ravel()], doubles=d[inv.ravel()])


@pytest.mark.parametrize("mask", ("all", "trip", "random"))
@pytest.mark.parametrize("form", FORMS)
def test_injected_states_under_draw_masks(injected, form, mask):
    st = injected["states"]
    masks = ps.draw_masks(mask, len(st), 32)
    cols = [np.ascontiguousarray(st[:, j]) for j in range(4)] + [masks]
    sentinel = ps.no_draw()
    for op, stream in (("state_words", injected["words"]), ("state_uniform", injected["doubles"])):
        want = ps.masked_stream(stream, masks, 32, sentinel)
        same_words(ps.run(f"{op}_{form}", *cols, k=32), want, f"{op}_{form} under the {mask} mask")


def test_both_forms_give_identical_output(injected, keyed):
    """RngT<true> and RngT<false> write the same words and doubles, sentinels included."""
    for st, steps in ((injected["states"], 32), (keyed["states"], 64)):
        masks = ps.draw_masks("random", len(st), steps, seed=405)
        cols = [np.ascontiguousarray(st[:, j]) for j in range(4)] + [masks]
        for op in ("state_words", "state_uniform"):
            same_words(ps.run(f"{op}_lean", *cols, k=steps), ps.run(f"{op}_full", *cols, k=steps), f"{op}: lean against full")


# ---- leaf filter ---------------------------------------------------------------------------------------------
def test_leaf_filter_device_equals_host(tmp_path):
    exe = ps.build_leaf_filter_host(tmp_path)
    cases, host = ps.leaf_filter_cases(exe, tmp_path, 1 << 16)
    got = ps.run("leaf_behind", *cases)
    assert 0.1 < host.mean() < 0.9, "both answers are among the cases"
    bad = np.flatnonzero(got != host)
    assert len(bad) == 0, f"{len(bad)} of {len(host)} differ, first: case {bad[0]} " \
                          f"{[float(c[bad[0]]).hex() for c in cases]} device {got[bad[0]]} host {host[bad[0]]}"

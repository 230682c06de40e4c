"""The kernel's hand-written f64 primitives (csrc/rt_device.h, csrc/rt_leaf_filter.h) value by value,
through the probe library (tests/hip/rt_probe.hip): sqrt_g, unit, the scatter finish, RayDiv, reflect,
refract, range_pm1, sample_key, the Xoshiro256++ draw and Random.float in both instruction forms, the
leaf filter, and the BVH walk's f32 slab primitives (csrc/rt_slab.h).  Every result is compared bit for bit with a correctly rounded numpy reference or with the
oracle's stream (tests/probe_support.py); the inputs sit on the guards, on rounding midpoints and in
single lanes of otherwise ordinary waves, where a whole render never puts them.  The f32 fast mode's bits
are unspecified and not probed; the slab primitives are f32 in both modes, and their bits are what the
padding certificate of csrc/rt_bvh.cpp assumes."""
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


# ---- the walk's f32 slab primitives ----------------------------------------------------------------------------
def test_rcp_clamp():
    """v_rcp_f32 + v_med3: within 1 ulp of the correctly rounded 1 / x wherever 1 / x is normal and inside
    the clamp (the padding certificate's assumption); +-1e30 with the operand's sign for +-0, denormals and
    every operand below 2^-100; in the binade between, one or the other; +-0 for +-inf; at most 2^-126 in
    size, sign kept, where 1 / x is denormal; and for a NaN what rt_slab.h says."""
    x = ps.rcp_inputs()
    got = ps.f32_of(ps.run("rcp_clamp", ps.f32_plane(x))[0])
    normal, tiny, inf, nan = ps.rcp_classes(x)
    err = ps.rcp_ulp_error(got[normal], x[normal])
    worst = int(np.argmax(err))
    print(f"rcp_clamp: largest error {err.max():.4f} ulp at x = {float(x[normal][worst]).hex()}, "
          f"{(err > 0.5).mean():.3f} of the results not correctly rounded; NaN -> {sorted(set(map(hex, ps.bits32(got[nan]))))}")
    assert err.max() <= 1.0
    big = np.float32(1e30)
    assert np.array_equal(got[tiny], np.where(np.signbit(x[tiny]), -big, big)), "zeros, denormals, |x| < 2^-100: +-1e30, the operand's sign"
    edge = (np.abs(x) >= np.float32(2.0 ** -100)) & (np.abs(x) < np.float32(2.0 ** -99))  # the clamp sets in
    assert edge.sum() >= 24 and (np.abs(got[edge]) <= big).all() and np.array_equal(np.signbit(got[edge]), np.signbit(x[edge]))
    assert ((np.abs(got[edge]) == big) | (ps.rcp_ulp_error(got[edge], x[edge]) <= 1.0)).all()
    assert (np.abs(got[edge]) == big).any() and (np.abs(got[edge]) < big).any()
    assert (got[inf] == 0).all() and np.array_equal(np.signbit(got[inf]), np.signbit(x[inf])), "+-inf: +-0"
    rest = ~(normal | tiny | inf | nan | edge)  # 1 / x is denormal
    assert rest.sum() >= 32 and (np.abs(got[rest]) <= np.float32(2.0 ** -126)).all()
    assert ((got[rest] == 0) | (np.signbit(got[rest]) == np.signbit(x[rest]))).all()
    assert nan.sum() >= 26 and (got[nan] == -big).all(), "a NaN component, quiet or signalling, of either sign: -1e30 (rt_slab.h)"


def test_pk_fma_lo_is_two_single_rounded_fmas_of_the_low_halves():
    cols = ps.pk_fma_inputs()
    got = ps.run("pk_fma_lo", *[ps.f32_plane(c) for c in cols])
    for lane, want in zip("xy", ps.pk_fma_ref(*cols)):
        g = ps.f32_of(got["xy".index(lane)])
        bad = np.flatnonzero(ps.bits32(g) != ps.bits32(want))
        assert len(bad) == 0, f"pk_fma_lo.{lane}: {len(bad)} of {len(want)} differ, first at {bad[0]}: " \
                              f"b {[float(cols[j][bad[0]]).hex() for j in (0, 1)]} m.x {float(cols[2][bad[0]]).hex()} " \
                              f"a.x {float(cols[4][bad[0]]).hex()} device {float(g[bad[0]]).hex()} reference {float(want[bad[0]]).hex()}"
        assert np.isfinite(g).all(), "the high halves of m and a (NaN, inf, FLT_MAX) are never read"


def test_control_mul_then_add_is_seen_to_differ():
    """b * m + a in two roundings on the device equals numpy's same expression, and differs from the fma
    in at least 20% of the elements of each lane: the comparison resolves the fma's single rounding."""
    cols = ps.pk_fma_inputs()
    got = ps.run("pk_mul_add", *[ps.f32_plane(c) for c in cols])
    for j, (two, one) in enumerate(zip(ps.pk_mul_add_ref(*cols), ps.pk_fma_ref(*cols))):
        g = ps.f32_of(got[j])
        assert np.array_equal(ps.bits32(g), ps.bits32(two)), f"lane {j}: {int((ps.bits32(g) != ps.bits32(two)).sum())} differ"
        differ = np.mean(ps.bits32(g) != ps.bits32(one))
        print(f"control differs from the fma in {differ:.3f} of lane {j}")
        assert differ >= 0.20


@pytest.mark.parametrize("far", [False, True])
def test_slab_near_and_far_are_the_fmaxf_and_fminf_chains(far):
    x, y, z, w, _ = ps.slab_inputs()
    op = "slab_far" if far else "slab_near"
    got = ps.f32_of(ps.run(op, *[ps.f32_plane(c) for c in (x, y, z, w)])[0])
    want = ps.slab_ref(x, y, z, w, far)
    bad = ps.same_f32(got, want)
    assert len(bad) == 0, f"{op}: {len(bad)} of {len(want)} differ, first at {bad[0]}: " \
                          f"{[float(c[bad[0]]) for c in (x, y, z, w)]} device {got[bad[0]]} reference {want[bad[0]]}"

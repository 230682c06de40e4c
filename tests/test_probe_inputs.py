"""CPU checks of what the device-primitive tests stand on (tests/probe_support.py): the input generators
produce the operand classes they promise, the numpy restatements equal the oracle, the injected RNG
states give the words they are built for, the control expression differs from the division, the
oracle's state functions continue its seeded ones, the operands of the walk's f32 slab primitives cover
their classes, and the probe library builds and loads."""
import ctypes as C

import numpy as np

import probe_support as ps

U64 = np.uint64


def bexp(x):
    return (np.asarray(x, np.float64).view(U64) >> U64(52)) & U64(0x7ff)


def test_oracle_state_functions_continue_the_seeded_ones(oracle):
    rng = np.random.default_rng(7)
    keys = [0, 1, (1 << 64) - 1, 1 << 63] + [int(k) for k in rng.integers(0, 1 << 64, 60, dtype=U64)]
    assert len(keys) == 64
    for key in keys:
        st = oracle.seed_state(key)
        assert np.array_equal(oracle.random_u64_state(st, 80), oracle.random_u64(key, 80)), key
        assert np.array_equal(oracle.random_doubles_state(st, 80).view(U64), oracle.random_doubles(key, 80).view(U64)), key
        assert np.array_equal(st, oracle.seed_state(key)), "the state is not modified"


def test_probe_library_builds_and_loads():
    L = ps.load()
    assert C.cast(L.rt_probe_run, C.c_void_p).value
    for op in ps.OPS:
        n_in, n_out, per_draw, byte_out = ps.planes(op)
        assert n_in >= 1 and n_out >= 1, op
    assert ps.planes("raydiv") == (2, 1, False, False)
    assert ps.planes("leaf_behind") == (4, 1, False, True)
    assert ps.planes("state_uniform_lean") == (5, 1, True, False)
    assert ps.planes("rcp_clamp") == (1, 1, False, False) and ps.planes("slab_far") == (4, 1, False, False)
    assert ps.planes("pk_fma_lo") == ps.planes("pk_mul_add") == (6, 2, False, False)
    assert L.rt_probe_run(ps.OPS["pk_fma_lo"], 1, 6 * 256 * 8, 1, 2 * 256 * 8 - 1, 256, 0, None) == -4
    # refused before anything is launched: unknown op, ragged n, too many draws, short buffers
    assert L.rt_probe_run(99, 1, 8, 1, 8, 256, 0, None) == -1
    assert L.rt_probe_run(ps.OPS["sqrt"], 1, 1 << 20, 1, 1 << 20, 100, 0, None) == -2
    assert L.rt_probe_run(ps.OPS["seed_words"], 1, 1 << 20, 1, 1 << 20, 256, 65, None) == -3
    assert L.rt_probe_run(ps.OPS["sqrt"], 1, 256 * 8 - 1, 1, 256 * 8, 256, 0, None) == -4
    assert L.rt_probe_run(ps.OPS["unit"], 1, 3 * 256 * 8, 1, 3 * 256 * 8 - 1, 256, 0, None) == -4
    assert np.isnan(np.array([ps.no_draw()], U64).view(np.float64)[0]), "the sentinel is no Random.float result"


# ---- division ------------------------------------------------------------------------------------------------
def test_division_random_set_covers_the_stated_ranges():
    a, x = ps.div_random()
    assert len(a) == len(x) == 1 << 15
    ea, ex = bexp(a).astype(int) - 1023, bexp(x).astype(int) - 1023
    assert ea.min() == -100 and ea.max() == 100 and ex.min() == -600 and ex.max() == 599
    assert (a > 0).all() and (x < 0).any() and (x > 0).any()
    assert (a > 2.0 ** 100).any(), "e = 100 with m > 1 is past the guard: the slow path is in the set"


def test_division_guard_edge_set_is_the_full_cross_product():
    a, x, cls = ps.div_guard_edges()
    assert len(ps.DIV_A_EDGES) == 11 and len(set(cls)) == 11 * 8 * 3 * 2
    for ia, e, kind, s in set(cls):
        i = cls.index((ia, e, kind, s))
        av = ps.DIV_A_EDGES[ia]
        assert (np.isnan(a[i]) and np.isnan(av)) or a[i] == av
        bits = int(x[i:i + 1].view(U64)[0])
        assert bits >> 63 == s and (bits >> 52) & 0x7ff == e
        m = bits & ps.M52
        assert (kind == 0 and m == 0) or (kind == 1 and m == ps.M52) or (kind == 2 and 0 < m < ps.M52)
    ae = ps.DIV_A_EDGES
    assert ae[1] < ae[0] == 2.0 ** -100 and ae[3] > ae[2] == 2.0 ** 100
    assert ae[1].view(U64) + U64(1) == ae[0].view(U64) and ae[2].view(U64) + U64(1) == ae[3].view(U64)


def test_division_near_sets_sit_where_they_claim():
    """x = fl(a*q) has a relative error of at most 2^-53, so the exact quotient x / a lies within one
    ulp of the 53-bit q; in the midpoint set within one ulp of q + ulp(q)/2.  Exact rational arithmetic
    on a sample; the neighbours are consecutive doubles."""
    from fractions import Fraction as F
    for gen, width, centre, half in ((ps.div_near_representable, 5, 2, 0), (ps.div_near_midpoint, 3, 1, 1)):
        a, x, q = gen(with_q=True)
        n = len(q)
        assert len(a) == len(x) == width * n and n == 1 << 13
        xi = x.view(np.int64) & np.int64(0x7fffffffffffffff)  # magnitudes
        for i in range(0, n, 53):
            ulp = F(float(np.spacing(abs(q[i]))))
            target = F(float(q[i])) + (ulp / 2 if q[i] > 0 else -ulp / 2) * half
            assert abs(F(float(x[centre * n + i])) / F(float(a[i])) - target) <= ulp, i
            for k in range(width):
                assert int(xi[k * n + i]) - int(xi[centre * n + i]) == k - centre
        e = bexp(x).astype(int)
        assert ((a >= 2.0 ** -100) & (a <= 2.0 ** 100)).all() and e.min() >= 423 and e.max() < 1623, "all on the fast path"


def test_division_extreme_set_overflows_underflows_and_goes_subnormal():
    a, x = ps.div_extreme_results()
    q = ps.div_ref(a, x)
    sub = (q != 0) & (np.abs(q) < 2.0 ** -1022)
    assert np.isinf(q).sum() >= 50 and (q == 0).sum() >= 50 and sub.sum() >= 50
    assert np.isfinite(a).all() and np.isfinite(x).all() and (a != 0).all()
    in_guard = (a >= 2.0 ** -100) & (a <= 2.0 ** 100)
    assert in_guard.sum() >= len(a) // 4 and (~in_guard).sum() >= len(a) // 4


def test_control_differs_from_the_division():
    """x * (1.0 / a) has two roundings: on the near-representable and near-midpoint sets it must differ
    from x / a in at least 20% of the elements, or the comparison could not see one ulp."""
    a = np.concatenate([ps.div_near_representable()[0], ps.div_near_midpoint()[0]])
    x = np.concatenate([ps.div_near_representable()[1], ps.div_near_midpoint()[1]])
    differ = np.mean(ps.div_ref(a, x).view(np.int64) != ps.mul_rcp_ref(a, x).view(np.int64))
    print(f"control differs in {differ:.3f}")
    assert differ >= 0.20


# ---- sqrt ----------------------------------------------------------------------------------------------------
def test_sqrt_sets_cover_the_guard_and_the_specials():
    x = ps.sqrt_random()
    e = bexp(x)
    assert e.min() == 0 and e.max() == 2046 and len(np.unique(e)) > 2000
    edges = ps.sqrt_edges()
    b = edges.view(U64)
    g = ps.SQRT_GUARD
    assert int(g) == 0x1000000000000000 and ps.f64(np.array([g]))[0] == 2.0 ** -767
    for want in (g - U64(1), g, g + U64(1)):
        assert (b == want).any()
    assert (b == U64(0)).any() and (b == U64(1 << 63)).any() and np.isnan(edges).any()
    assert (edges == np.inf).any() and (edges == -np.inf).any() and (edges == ps.BIG).any()
    assert (edges == 2.0 ** -1022).any() and ((edges > 0) & (edges < 2.0 ** -1022)).sum() >= 4 and (edges < 0).sum() >= 4
    near = ps.sqrt_near_squares()
    n = len(near) // 8
    assert n == 1 << 13
    r = np.sqrt(near[2 * n:3 * n])
    assert (r * r == near[2 * n:3 * n]).mean() > 0.4, "fl(q*q): the root is q itself for most q"
    assert ((near > 0) & (near < 2.0 ** -767)).any() and (near > 2.0 ** 900).any()


def test_lane_layouts_place_every_special_at_every_lane():
    for lay in (ps.div_layouts(), ps.sqrt_layouts()):
        assert set(lay) == {"order", "one_special", "waves"}
        for name, planes in lay.items():
            assert len({len(p) for p in planes}) == 1
            assert name == "order" or len(planes[0]) % 64 == 0
    # division: exactly one element per wave is out of range, at lane 0, 31, 32, 63 equally often
    a, x = ps.div_layouts()["one_special"]
    edges = ps.div_guard_edges()[:2]
    extreme = ps.div_extreme_results()
    n_spec = len(edges[0]) + len(extreme[0])
    assert len(a) == 4 * n_spec * 64
    ex = bexp(x).astype(int)
    slow = ~((a >= 2.0 ** -100) & (a <= 2.0 ** 100)) | (ex < 423) | (ex >= 1623)
    w = slow.reshape(-1, 64)
    assert (w.sum(axis=1) <= 1).all(), "ordinary lanes are in range"
    lanes = np.nonzero(w)[1]
    assert set(lanes) == set(ps.LANES)
    counts = [int((lanes == l).sum()) for l in ps.LANES]
    assert len(set(counts)) == 1 and counts[0] >= 0.8 * n_spec, counts
    _, at = ps.one_special_lane(ps.div_ordinary(64), edges)
    assert sorted(set(at % 64)) == list(ps.LANES) and len(at) == 4 * len(edges[0])
    # sqrt likewise
    (sx,) = ps.sqrt_layouts()["one_special"]
    hi = (sx.view(U64) >> U64(32)).astype(np.int64)
    slow = ~((hi - 0x10000000 >= 0) & (hi - 0x10000000 < 0x6ff00000))
    w = slow.reshape(-1, 64)
    assert (w.sum(axis=1) <= 1).all() and set(np.nonzero(w)[1]) == set(ps.LANES)
    # whole waves of specials
    a, x = ps.div_layouts()["waves"]
    assert len(a) >= n_spec and len(a) % 64 == 0


# ---- vectors -------------------------------------------------------------------------------------------------
def test_unit_inputs_hold_the_guard_cases():
    v = ps.unit_inputs()
    with np.errstate(all="ignore"):
        ls = ps.len_sq(v)
    t = 2.0 ** -384
    col = lambda p: np.flatnonzero((v[0] == p[0]) & (v[1] == p[1]) & (v[2] == p[2]))
    for p in ((t, t, 0.0), (t, 0.0, 0.0), (0.0, 0.0, 0.0), (2.0 ** 600, 0.0, 0.0)):
        at = col(p)
        assert len(at) >= 4 and set(at % 64) >= set(ps.LANES), p
    assert ls[col((t, t, 0.0))[0]] == 2.0 ** -767 and ls[col((t, 0.0, 0.0))[0]] == 2.0 ** -768
    assert np.isinf(ls).any() and np.isinf(v).any() and (ls == 0).any()
    e = bexp(np.sqrt(ls[np.isfinite(ls) & (ls > 0)])).astype(int) - 1023
    assert e.min() <= -383 and e.max() >= 510


def test_unit_accepted_inputs_are_accepted_points(oracle):
    p = ps.unit_accepted_inputs(oracle)
    assert p.shape[0] == 3 and p.shape[1] >= (1 << 14) + 1000
    assert ps.accepted(p).all()
    ls = ps.len_sq(p)
    assert (ls == 1).sum() >= 6 and (p == 0).any() and (np.abs(p) == 2.0 ** -52).any()
    assert ls.min() < 1e-158, "the small end of the documented domain"
    # the first block is what range_pm1 gives for a real stream
    u = oracle.random_doubles(302, 3 * 2 * (1 << 14)).reshape(3, -1)
    real = -1.0 + 2.0 * u
    real = real[:, ps.accepted(real)][:, :1 << 14]
    assert real.shape[1] == 1 << 14 and np.array_equal(p[:, :1 << 14], real)


def test_reflect_and_refract_restatements_equal_the_oracle(oracle):
    v, n, eta, at = ps.refract_inputs()
    pick = np.concatenate([np.arange(96), at[:128], np.arange(len(eta) - 32, len(eta))])
    assert len(pick) == 256
    rl, rr = ps.reflect_ref(v, n), ps.refract_ref(v, n, eta)
    for i in pick:
        want = np.array(oracle.reflect(v[:, i], n[:, i]))
        assert np.array_equal(want.view(np.int64), rl[:, i].copy().view(np.int64)), i
        want = np.array(oracle.refract(v[:, i], n[:, i], eta[i]))
        assert len(ps.mismatches(rr[:, i].copy(), want)) == 0, (i, want, rr[:, i])


def test_refract_inputs_reach_the_branches():
    v, n, eta, at = ps.refract_inputs()
    assert sorted(set(at % 64)) == list(ps.LANES)
    with np.errstate(all="ignore"):
        cos_t = np.fmin(ps.dot(-v, n), 1.0)
        ls = ps.len_sq((v + n * cos_t) * eta)
    assert (ls == 1).sum() >= 16, "sqrt of exactly 0: sqrt_g's slow path"
    assert ((ls > 1) & (ls < 1 + 1e-6)).sum() >= 16, "just above 1: the fabs branch"
    assert (ls > 1.5).any() and (ls < 0.5).any()
    assert (eta.min() >= 0.4) and (eta.max() <= 2.5)
    q = len(eta) // 8
    assert np.array_equal(v[:, :q], -n[:, :q])


def test_range_pm1_inputs(oracle):
    u = ps.range_pm1_inputs(oracle)
    assert ((u >= 0) & (u < 1)).all() and (u == 0).any() and (u == 2.0 ** -1074).any() and (u == 0.5).any()
    ref = ps.range_pm1_ref(u)
    assert ((ref >= -1) & (ref < 1)).all()
    assert (ref == -1).sum() >= 2, "2u below half an ulp of 1 rounds away"
    assert (ref == 0).any() and not np.signbit(ref[ref == 0]).any(), "a zero of range_pm1 is +0.0, never -0.0"


# ---- RNG -----------------------------------------------------------------------------------------------------
def test_key_cases_cover_seed_pixel_sample_edges(oracle):
    seeds, pix, smp = ps.key_cases()
    assert len(seeds) == 4096
    hi = seeds >> U64(63)
    assert (hi == 1).sum() >= 1000 and (hi == 0).sum() >= 1000
    combos = set(zip(pix.tolist(), smp.tolist()))
    assert combos == {(p, s) for p in (0, 1, 1 << 31, (1 << 32) - 1) for s in (0, 1 << 31, (1 << 32) - 1)}
    keys = {oracle.sample_key(int(s), int(p), int(m)) for s, p, m in zip(seeds[:256], pix[:256], smp[:256])}
    assert len(keys) == 256


def test_rare_keys_hold_a_rare_word(oracle):
    keys = ps.rare_keys(oracle, want=32)
    assert len(keys) == 32
    for k in keys:
        w = oracle.random_u64(int(k), 64)
        assert ps.is_rare(w).any()
        # the rare word costs the stream of doubles at least one extra word
        d = oracle.random_doubles(int(k), 64)
        i = int(np.flatnonzero(ps.is_rare(w))[0])
        plain = lambda x: ((1022 - ps.clz64(x)) << 52) | (int(x) & ps.M52)
        assert all(int(d[j:j + 1].view(U64)[0]) == plain(w[j]) for j in range(i))
        assert int(d[i:i + 1].view(U64)[0]) & ps.M52 == int(w[i]) & ps.M52 and d[i] < 2.0 ** -12


def test_injected_states_give_the_words_they_are_built_for(oracle):
    states, words = ps.deep_states()
    assert len(states) == len(words) >= 60
    depth = []
    for st, w in zip(states, words):
        got = oracle.random_u64_state(st, max(len(w), 4))
        assert [int(x) for x in got[:len(w)]] == list(w), (st, w)
        # words Random.float consumes for its first draw
        k = 1
        if ps.clz64(got[0]) >= 12:
            stream = oracle.random_u64_state(st, 20)
            while k < 17 and stream[k] == 0:
                k += 1
            k = min(k + 1, 17)
        depth.append(k)
    assert depth[0] == 17 and oracle.random_doubles_state(states[0], 3).view(U64).tolist() == [0, 0, 0]
    assert depth.count(4) >= 20 and depth.count(3) >= 16 and depth.count(1) >= 8
    first = [w[0] for w in words]
    assert sum(ps.clz64(x) == 11 for x in first) >= 8 and sum(ps.clz64(x) == 12 for x in first) >= 8
    # T, 0, 0, w: 12 + 64 + 64 + clz(w) leading zeros; the exponent field is 1022 minus that
    st, w = states[1], words[1]
    d = int(oracle.random_doubles_state(st, 1).view(U64)[0])
    assert d >> 52 == 1022 - (12 + 128 + ps.clz64(w[3])) and d & ps.M52 == w[0]
    ends = {ps.clz64(w[-1]) for w in words if len(w) in (3, 4)}
    assert {11, 12} <= ends, "the word that ends the run of zeros has exactly 11 and exactly 12 leading zeros too"


def test_masks_and_masked_reference():
    for steps in (32, 64):
        full = (1 << steps) - 1
        assert (ps.draw_masks("all", 100, steps) == U64(full)).all()
        trip = ps.draw_masks("trip", 4096, steps)
        for k in range(steps):
            bit = (trip >> U64(k)) & U64(1)
            assert (bit == 1).all() if k % 3 != 2 else 0.3 < bit.mean() < 0.7, k
        rnd = ps.draw_masks("random", 4096, steps)
        assert (rnd <= U64(full)).all() and len(np.unique(rnd)) > 4000
    stream = np.arange(3 * 8, dtype=U64).reshape(3, 8) + U64(100)
    masks = np.array([0b11111111, 0b00100100, 0], U64)
    out = ps.masked_stream(stream, masks, 8, U64(7))
    assert out[:, 0].tolist() == list(range(100, 108))
    assert out[:, 1].tolist() == [7, 7, 108, 7, 7, 109, 7, 7]
    assert out[:, 2].tolist() == [7] * 8


# ---- the walk's f32 slab primitives ----------------------------------------------------------------------------
def test_rcp_inputs_cover_every_exponent_and_the_edges():
    x = ps.rcp_inputs()
    b = ps.bits32(x)
    e = (b >> np.uint32(23)) & np.uint32(0xff)
    for sign in (0, 1):
        assert len(np.unique(e[(b >> np.uint32(31)) == sign])) == 256, "every exponent, both signs"
    for edge in (0, 1, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, ps.QNAN32):
        assert (b == edge).any() and (b == (edge | 0x80000000)).any(), hex(edge)
    for k in (1, 127, 254):  # powers of two with both neighbours
        assert all((b == (k << 23) + d).any() for d in (-1, 0, 1))
    normal, tiny, inf, nan = ps.rcp_classes(x)
    assert normal.sum() >= 5000 and tiny.sum() >= 600 and inf.sum() == 2 and nan.sum() >= 26
    ax = np.abs(x[~nan].astype(np.float64))
    assert ((ax < ps.FLT_MIN) & (ax > 0)).sum() >= 24 and ((ax >= 2.0 ** -100) & (ax < 2.0 ** -99)).sum() >= 24
    assert (np.isfinite(ax) & (ax > 2.0 ** 126)).sum() >= 32, "operands whose reciprocal is denormal"
    # the error measure: 0 for the correctly rounded reciprocal, 1 for its neighbour next to a power of two
    ok = x[normal]
    want = (1.0 / ok.astype(np.float64)).astype(np.float32)
    assert ps.rcp_ulp_error(want, ok).max() <= 0.5
    assert 0.5 <= ps.rcp_ulp_error(np.nextafter(want, np.float32(np.inf)), ok).min() and \
        ps.rcp_ulp_error(np.nextafter(want, np.float32(np.inf)), ok).max() <= 1.5 + 1e-9
    # and the model's reciprocal (slab_support.rcp_clamp) obeys what the device test asks of the device
    model = ps.rcp_clamp(x)
    assert ps.rcp_ulp_error(model[normal], ok).max() <= 0.5
    assert np.array_equal(model[tiny], np.where(np.signbit(x[tiny]), np.float32(-1e30), np.float32(1e30)))


def test_pk_fma_inputs_cancel_and_the_control_differs():
    cols = ps.pk_fma_inputs()
    bx, by, mx, my, ax, ay = cols
    assert all(c.dtype == np.float32 and len(c) == 1 << 14 for c in cols)
    assert np.isfinite(np.stack([bx, by, mx, ax])).all()
    assert not np.isfinite(my).all() and not np.isfinite(ay).all() and np.isnan(my).any() and np.isnan(ay).any()
    assert (np.abs(my[np.isfinite(my)]) == ps.FLT_MAX).all(), "finite junk is large"
    one, two = ps.pk_fma_ref(*cols), ps.pk_mul_add_ref(*cols)
    third = len(bx) // 3
    with np.errstate(all="ignore"):
        small = np.abs(one[0][third:2 * third]) <= np.abs(bx * mx)[third:2 * third] * 2.0 ** -20
    assert small.all(), "the x lane's middle third cancels to a residual"
    for j in range(2):
        differ = np.mean(ps.bits32(one[j]) != ps.bits32(two[j]))
        print(f"lane {j}: two roundings differ from one in {differ:.3f}")
        assert differ >= 0.20
    # fma32 itself, against exact rational arithmetic on a sample
    from fractions import Fraction as F
    for i in list(range(0, len(bx), 97)) + list(range(third, third + 64)):
        exact = F(float(bx[i])) * F(float(mx[i])) + F(float(ax[i]))
        want = np.float32(exact.numerator / exact.denominator) if exact else np.float32(0)
        assert one[0][i] == want, (i, one[0][i], want)


def test_slab_inputs_hold_every_pattern_of_specials():
    x, y, z, w, at = ps.slab_inputs()
    assert len(at) == 6 ** 4 and sorted(set(at % 64)) == list(ps.LANES)
    cols = np.stack([x, y, z, w])[:, at]
    nans = np.isnan(cols).sum(axis=0)
    assert [int((nans == k).sum()) for k in range(5)] == [625, 500, 150, 20, 1]
    for k in (1, 2, 3):
        assert (np.isnan(cols[:3]).sum(axis=0) == k).any(), "%d of x, y, z NaN" % k
    assert (cols == np.inf).any(axis=1).all() and (cols == -np.inf).any(axis=1).all()
    zero = cols == 0
    assert (zero & np.signbit(cols)).any(axis=1).all() and (zero & ~np.signbit(cols)).any(axis=1).all()
    # the reference drops NaN operands: NaN only where all four are
    for far in (False, True):
        ref = ps.slab_ref(x, y, z, w, far)
        assert np.isnan(ref).sum() == 1 and np.isnan(ref[at][nans == 4]).all()
    assert len(ps.same_f32(np.float32([0.0, np.nan, 1.0]), np.float32([-0.0, np.nan, 1.0]))) == 0
    assert ps.same_f32(np.float32([1.0, np.inf]), np.float32([np.nextafter(np.float32(1), np.float32(2)), -np.inf])).tolist() == [0, 1]

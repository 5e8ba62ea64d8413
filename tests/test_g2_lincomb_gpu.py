"""GPU tests of G2 linear combinations (kzg_g2_lincomb / kzg_g2_lincomb_powers) and of what the facade
builds on them: lincomb_g2, commit_g2 and check_key(g2_chain="fold").  Every comparison is exact.  Expected sums come
from curve.Group.multiply / add (at most 92 products per curve, g2_lincomb_cases.lane_pool) or, for the calls of one
launch and more, from a known discrete logarithm: the points are [tau^j] G2 -- what setup_g2(count, tau, device=True)
computes, kept as arrays -- so the sum is [sum_j k_j tau^j mod r] G2, one host multiplication."""
import re

import numpy as np
import pytest

import g2_lincomb_cases as gl
import g_mul_cases as gm
from g2_bytes_cases import INF2
from g_mul_cases import GUARD, guard_ok, guarded, vp
from kzg_snark_amd import curve as C

pytestmark = pytest.mark.gpu

CURVES = gm.CURVES
TAU = 0x5eed0123456789abcdef
LIMIT = 1 << 21
G2_FAULT = "the G2 powers are not a chain of powers of the tau of [tau] G1"
G1_FAULT = "the G1 powers are not a chain of powers of the tau of [tau] G2"


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


def consts(native):
    ctx = native.Context
    return ctx.G2_LINCOMB_LANES, ctx.G2_LINCOMB_LAUNCH_LANES, ctx.G2_LINCOMB_FOLD_LANES, ctx.G2_LINCOMB_FOLD_SPAN


def one_point(native, out):
    return native.limbs_to_g2_points(out[0].reshape(1, -1), out[1])[0]


def last_error(native, ctx):
    msg = native.lib().kzg_last_error(ctx._h)
    return msg.decode() if msg else ""


# ---- sizes ---------------------------------------------------------------------------------------------------------------

def fold_sizes(native):
    """64 k + 1 for the smallest k that gives the fold a second step of each kind: a second point in a workgroup's sum
    (k = 1), a second point in a LANE's sum (k = the fold's lanes) and a second level (k = the fold's span)"""
    tb, _, fold_tb, span = consts(native)
    return [tb * 1 + 1, tb * fold_tb + 1, tb * span + 1]


@pytest.mark.parametrize("curve", CURVES)
def test_sizes_around_the_wave_and_the_steps_of_the_fold(kzgs, native, curve):
    kzg = kzgs[curve]
    sizes = [0, 1, 2, 63, 64, 65] + fold_sizes(native)
    assert sizes[-3:] == [65, 4097, 16385]
    shim = gl.build_shim()
    assert [gl.shim_plan(shim, curve, n)["levels"] for n in sizes[-3:]] == [1, 1, 2]
    for n in sizes:
        pts, ks, want = gl.lanes_and_sum(curve, n)
        assert kzg.lincomb_g2(pts, ks) == want, n


# ---- one launch and more, by discrete logarithm ---------------------------------------------------------------------------

_POWERS = {}


def tau_powers(kzg, native, n):
    """([tau^j] G2 for j < n as arrays, computed once per curve at the largest size the tests use)"""
    cap = consts(native)[1]
    if kzg.curve_type not in _POWERS:
        top = 2 * cap + 1
        xy, inf = kzg._g2_arrays([kzg.G2], "powers")
        _POWERS[kzg.curve_type] = kzg._context().g2_mul_powers(np.repeat(xy, top, axis=0), np.repeat(inf, top), TAU, 1)
    xy, inf = _POWERS[kzg.curve_type]
    assert n <= xy.shape[0]
    return xy[:n], inf[:n]


def dlog_point(kzg, weights):
    """[sum_j weights_j tau^j mod r] G2"""
    r = kzg.curve_order
    e, t = 0, 1
    for w in weights:
        e = (e + w * t) % r
        t = t * TAU % r
    G = kzg._g2
    return G.normalize(G.multiply(kzg.G2, e)) if e else INF2


def test_the_device_powers_are_setup_g2s(kzgs, native):
    for curve in CURVES:
        kzg = kzgs[curve]
        xy, inf = tau_powers(kzg, native, 5)
        assert native.limbs_to_g2_points(xy, inf) == kzg.setup_g2(5, TAU, device=True) == kzg.setup_g2(5, TAU)


@pytest.mark.parametrize("launches", [1, 2])
@pytest.mark.parametrize("curve", CURVES)
def test_one_launch_plus_one_and_two_launches_plus_one(kzgs, native, curve, launches):
    kzg = kzgs[curve]
    cap = consts(native)[1]
    n = launches * cap + 1
    assert gl.shim_plan(gl.build_shim(), curve, n)["launches"] == launches + 1
    xy, inf = tau_powers(kzg, native, n)
    k = gm.random_rows(0x6c + launches, n)
    got = one_point(native, kzg._context().g2_lincomb(xy, inf, k))
    assert got == dlog_point(kzg, native.limbs_to_ints(k))
    # the power form at the same size, s of odd order: both levels of the power table decide the scalars
    s, m = gm.odd_order_scalar(curve)
    c0 = 0x1234567
    r = kzg.curve_order
    cycle = [c0 * pow(s, j, r) % r for j in range(m)]
    got = one_point(native, kzg._context().g2_lincomb_powers(xy, inf, s, c0))
    assert got == dlog_point(kzg, (cycle[j % m] for j in range(n)))


# ---- exceptional sums ------------------------------------------------------------------------------------------------------

def named(curve):
    pts = {w: pt for pt, w in gm.points(curve, 2)}
    small = next(w for w in pts if w.startswith("order "))
    return pts, pts[small], int(small.split()[1])


@pytest.mark.parametrize("curve", CURVES)
def test_copies_of_one_point_with_one_scalar(kzgs, native, curve):
    """equal lanes: a doubling in every round of the wave sum; many equal workgroups: equal partial sums, doublings in the
    fold's lanes, waves and second level"""
    kzg, G = kzgs[curve], gm.group(curve, 2)
    pts, _, _ = named(curve)
    tb, _, _, span = consts(native)
    k = 0x123456789abcdef0fedcba9876543210
    for Q in (pts["random subgroup point 0"], pts["outside the subgroup"]):
        for n in (64, 65, tb * (span + 44)):
            assert kzg.lincomb_g2([Q] * n, [k] * n) == G.normalize(G.multiply(Q, n * k)), n


@pytest.mark.parametrize("curve", CURVES)
def test_opposite_points_multiples_of_r_and_small_orders(kzgs, native, curve):
    kzg, G = kzgs[curve], gm.group(curve, 2)
    r = C.CURVES[curve].r
    pts, small, q = named(curve)
    Q, R, out = pts["random subgroup point 0"], pts["G"], pts["outside the subgroup"]
    k = 0xfeedface
    # Q and -Q interleaved
    for n in (2, 64, 130):
        assert kzg.lincomb_g2([Q if i % 2 == 0 else G.neg(Q) for i in range(n)], [k] * n) == INF2
    assert kzg.lincomb_g2([Q if i % 2 == 0 else G.neg(Q) for i in range(129)], [k] * 129) == G.normalize(G.multiply(Q, k))
    # k = r and 2r on points of the subgroup: infinity in every lane
    sub = [Q, R, pts["-G"], pts["random subgroup point 1"]]
    assert kzg.lincomb_g2([sub[i % 4] for i in range(70)], [r if i % 3 else 2 * r for i in range(70)]) == INF2
    # ... and not on a point outside it
    want = G.normalize(G.multiply(out, r))
    assert want != INF2 and kzg.lincomb_g2([out], [r]) == want
    assert kzg.lincomb_g2([out, Q, out], [r, 2 * r, r]) == G.normalize(G.multiply(out, 2 * r))
    # q copies of the point of order q (13 on bls12_381, 10069 on bn254), and one fewer
    assert kzg.lincomb_g2([small] * q, [1] * q) == INF2
    assert kzg.lincomb_g2([small] * (q - 1), [1] * (q - 1)) == G.normalize(G.neg(small))
    assert kzg.lincomb_g2([small] * 13, [q + 1] * 13) == G.normalize(G.multiply(small, 13 % q))
    # every scalar 0
    assert kzg.lincomb_g2([Q, out, small] * 30, [0] * 90) == INF2


@pytest.mark.parametrize("curve", CURVES)
def test_infinite_points_with_and_without_the_flag_array(kzgs, native, curve):
    kzg, G = kzgs[curve], gm.group(curve, 2)
    ctx = kzg._context()
    L = ctx.fp_limbs
    n = 70
    k = gm.random_rows(3, n)
    zeros, ones = np.zeros((n, 4 * L), dtype=np.uint64), np.ones(n, dtype=np.uint8)
    assert one_point(native, ctx.g2_lincomb(zeros, ones, k)) == INF2
    assert one_point(native, ctx.g2_lincomb(gm.random_rows(4, n, 4 * L), ones, k)) == INF2      # the flag decides
    # no flag array: no point is infinity, and zeros are not a point of the twist
    with pytest.raises(native.NativeError, match=r"kzg_g2_lincomb: point 0 has a coordinate >= p or is not on the twist"):
        ctx.g2_lincomb(zeros, None, k)
    # finite points: a null array is an array of zeros, and a flagged lane drops out of the sum
    pts, ks, want = gl.lanes_and_sum(curve, n)
    xy, inf = kzg._g2_arrays(pts, "test")
    rows = native.ints_to_limbs(ks)
    assert not inf.any()
    assert one_point(native, ctx.g2_lincomb(xy, None, rows)) == want == one_point(native, ctx.g2_lincomb(xy, inf, rows))
    drop = inf.copy()
    drop[5] = 1
    assert one_point(native, ctx.g2_lincomb(xy, drop, rows)) == G.normalize(G.add(want, G.neg(G.multiply(pts[5], ks[5]))))


# ---- refusals --------------------------------------------------------------------------------------------------------------

def c_call(native, ctx, xy, inf, n, k=None, s=None, c0=None):
    """either entry point through the C ABI with guard bytes IN and behind both outputs -> (rc, out_xy, out_inf)"""
    width = 4 * ctx.fp_limbs * 8
    o_xy, o_inf = guarded(width), guarded(1)
    o_xy[:], o_inf[:] = GUARD, GUARD
    lib = native.lib()
    if s is None:
        rc = lib.kzg_g2_lincomb(ctx._h, vp(xy), None if inf is None else vp(inf), n, vp(k), vp(o_xy), vp(o_inf))
    else:
        rc = lib.kzg_g2_lincomb_powers(ctx._h, vp(xy), None if inf is None else vp(inf), n, vp(native.int_to_words(s)),
                                       vp(native.int_to_words(c0)), vp(o_xy), vp(o_inf))
    assert guard_ok(o_xy, width) and guard_ok(o_inf, 1)
    return rc, o_xy, o_inf


@pytest.mark.parametrize("curve", CURVES)
def test_a_bad_point_in_the_second_launch_is_named_and_nothing_is_written(kzgs, native, curve):
    kzg = kzgs[curve]
    ctx = kzg._context()
    cv = C.CURVES[curve]
    L = ctx.fp_limbs
    cap = consts(native)[1]
    n = cap + 1
    spans = [(b0 * 64, min(n, (b0 + g) * 64)) for b0, g in launch_grids(curve, n)]
    assert len(spans) == 2
    first = spans[1][0]                                               # the first lane of the second launch
    xy, inf = tau_powers(kzg, native, n)
    k = gm.random_rows(9, n)
    gen = gm.points(curve, 2)[1][0]
    off = (gen[0], (gen[1][0] ^ 1, gen[1][1]), (1, 0))
    off_row = native.g2_points_to_limbs([off], L)[0][0]
    big_row = xy[first].copy()                                        # x.c0 + p: the same point, a coordinate >= p
    x0 = sum(int(v) << (64 * i) for i, v in enumerate(xy[first][:L]))
    assert x0 + cv.p < 1 << (64 * L)                                  # p leaves headroom in its limbs on both curves
    big_row[:L] = [((x0 + cv.p) >> (64 * i)) & (2 ** 64 - 1) for i in range(L)]
    cases = [(off_row, "off the twist"), (big_row, "a coordinate >= p")]
    for row, what in cases:
        for behind in (first + 1, n - 1):
            bad = xy.copy()
            bad[first], bad[behind] = row, off_row
            rc, o_xy, o_inf = c_call(native, ctx, bad, inf, n, k=k)
            assert rc == -1, what
            assert last_error(native, ctx) == f"kzg_g2_lincomb: point {first} has a coordinate >= p or is not on the twist"
            assert (o_xy == GUARD).all() and (o_inf == GUARD).all()
            rc, o_xy, o_inf = c_call(native, ctx, bad, inf, n, s=3, c0=1)
            assert rc == -1 and re.fullmatch(r"kzg_g2_lincomb_powers: point %d .*" % first, last_error(native, ctx))
            assert (o_xy == GUARD).all() and (o_inf == GUARD).all()
    # the context lives, and a flagged lane may hold anything
    bad = xy.copy()
    bad[first] = off_row
    flags = inf.copy()
    flags[first] = 1
    k[first] = 0
    rc, o_xy, o_inf = c_call(native, ctx, bad, flags, n, k=k)
    assert rc == 0 and o_inf[0] == 0
    rc2, o_xy2, _ = c_call(native, ctx, xy, inf, n, k=k)
    assert rc2 == 0 and np.array_equal(o_xy, o_xy2)


def launch_grids(curve, n):
    p = gl.shim_plan(gl.build_shim(), curve, n)
    return [(b0, min(p["launch_blocks"], p["blocks"] - b0)) for b0 in range(0, p["blocks"], p["launch_blocks"])]


@pytest.mark.parametrize("curve", CURVES)
def test_scalars_not_below_r_and_too_many_points_are_refused(kzgs, native, curve):
    kzg = kzgs[curve]
    ctx = kzg._context()
    r, L = kzg.curve_order, ctx.fp_limbs
    xy, inf = tau_powers(kzg, native, 5)
    for n in (5, 0):
        for s, c0, name in ((r, 1, "s"), ((1 << 256) - 1, 1, "s"), (2, r, "c0")):
            rc, o_xy, o_inf = c_call(native, ctx, xy, inf, n, s=s, c0=c0)
            assert rc == -1 and last_error(native, ctx) == f"kzg_g2_lincomb_powers: {name} is not below the group order r"
            assert (o_xy == GUARD).all() and (o_inf == GUARD).all()
    n = LIMIT + 1
    xy, inf, k = np.zeros((n, 4 * L), dtype=np.uint64), np.ones(n, dtype=np.uint8), np.zeros((n, 4), dtype=np.uint64)
    for form, name in ((dict(k=k), "kzg_g2_lincomb"), (dict(s=1, c0=1), "kzg_g2_lincomb_powers")):
        rc, o_xy, o_inf = c_call(native, ctx, xy, inf, n, **form)
        assert rc == -1 and last_error(native, ctx) == name + ": more than 2^21 points"
        assert (o_xy == GUARD).all() and (o_inf == GUARD).all()
        rc, o_xy, o_inf = c_call(native, ctx, xy, inf, 0, **form)                      # the empty sum is infinity
        width = 4 * L * 8
        assert rc == 0 and not o_xy[:width].any() and o_inf[0] == 1


@pytest.mark.parametrize("curve", CURVES)
def test_the_power_form_is_mul_powers_summed(kzgs, native, curve):
    kzg, G = kzgs[curve], gm.group(curve, 2)
    ctx = kzg._context()
    pts, small, _ = named(curve)
    five = [pts["G"], pts["outside the subgroup"], INF2, small, pts["random subgroup point 2"]]
    xy, inf = kzg._g2_arrays(five, "test")
    r = kzg.curve_order
    for s, c0 in ((0, 7), (5, 0), (1, 9), (0, 0), (r - 1, r - 1), (3, 1)):
        acc = INF2
        for pt in native.limbs_to_g2_points(*ctx.g2_mul_powers(xy, inf, s, c0)):
            acc = G.add(acc, pt)
        assert one_point(native, ctx.g2_lincomb_powers(xy, inf, s, c0)) == G.normalize(acc), (s, c0)
        ks = [c0 * pow(s, j, r) % r for j in range(5)]
        assert kzg.lincomb_g2(five, ks) == G.normalize(acc)


# ---- the facade ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_lincomb_g2_against_the_host_and_what_it_refuses(kzgs, native, curve):
    kzg, G = kzgs[curve], gm.group(curve, 2)
    pts, ks, want = gl.lanes_and_sum(curve, 37)
    assert kzg.lincomb_g2(pts, ks) == want
    xy, inf = kzg._g2_arrays(pts, "test")
    assert kzg.lincomb_g2((xy, inf), native.ints_to_limbs(ks)) == want           # arrays in, still one point out
    assert kzg.lincomb_g2([], []) == INF2
    gen = gm.points(curve, 2)[1][0]
    off = (gen[0], (gen[1][0] ^ 1, gen[1][1]), (1, 0))
    with pytest.raises(ValueError, match=r"point 3 has a coordinate >= p or is not on the twist"):
        kzg.lincomb_g2([gen, gen, gen, off, gen, off], [1] * 6)
    with pytest.raises(ValueError, match=r"scalar 1 is not in \[0, 2\^256\)"):
        kzg.lincomb_g2([gen, gen], [1, 1 << 256])
    with pytest.raises(ValueError, match=r"1 scalars for 2 points"):
        kzg.lincomb_g2([gen, gen], [1])


@pytest.mark.parametrize("curve", CURVES)
def test_commit_g2_pairs_with_commit(kzgs, native, curve):
    kzg = kzgs[curve]
    r = kzg.curve_order
    n = 16
    ck = kzg.setup(n - 1, TAU)[0]
    g2 = kzg.setup_g2(n, TAU, device=True)
    rng = np.random.default_rng(5)
    rand = lambda m: [int.from_bytes(rng.bytes(40), "little") for _ in range(m)]       # not reduced: canonicalised like commit's
    polys = [[], [7], rand(3), [0, 0, 5, 0, 0], rand(n), rand(9) + [0] * 20]
    c1, c2 = kzg.commit(ck, polys), kzg.commit_g2(g2, polys)
    assert len(c2) == len(polys) and c2[0] == INF2 and c2[1] == kzg._g2.normalize(kzg._g2.multiply(kzg.G2, 7))
    for a, b in zip(c1, c2):
        assert kzg.pairing_check([(a, kzg._g2.neg(kzg.G2)), (kzg.G1, b)]) is True
    assert kzg.pairing_check([(c1[2], kzg._g2.neg(kzg.G2)), (kzg.G1, c2[4])]) is False
    assert c2[4] == dlog_point(kzg, [c % r for c in polys[4]])
    assert kzg.commit_g2(g2, []) == []
    with pytest.raises(ValueError, match=r"^Polynomial degree 16 exceeds maximum allowed degree 15$"):
        kzg.commit_g2(g2, [rand(3), rand(n + 1)])
    with pytest.raises(ValueError, match=r"^Polynomial degree 16 exceeds maximum allowed degree 15$"):
        kzg.commit(ck, [rand(3), rand(n + 1)])


def faults(kzg, ck, g2, r):
    return [kzg._key_fault(ck, g2, None, r, chain) for chain in ("links", "fold")]


@pytest.mark.parametrize("curve", CURVES)
def test_check_key_fold_gives_the_verdicts_and_the_names_of_links(kzgs, native, curve, tmp_path):
    kzg = kzgs[curve]
    G2 = kzg._g2
    setup, contribution = kzg.contribute(kzg.unit_setup(16, 10), 0xabcdef0123456789)
    ck, g2 = setup.monomial, list(setup.g2)
    assert kzg.check_key(ck, g2, setup.lagrange, r=7, g2_chain="fold") is True
    assert kzg.check_key(ck, g2, setup.lagrange, g2_chain="fold") is True               # a random rho
    assert kzg.check_key(ck, g2, setup.lagrange, r=7) is True
    assert kzg.verify_contribution(kzg.unit_setup(16, 10), setup, contribution, r=7, g2_chain="fold") is True
    assert kzg.verify_contributions(kzg.G1, [contribution], g2_chain="fold") == [True]
    stray = G2.multiply(kzg.G2, 0xbad)
    broken = {"a wrong generator": ([stray] + g2[1:], "the first G2 power is not the generator"),
              "a power in the middle": (g2[:5] + [stray] + g2[6:], G2_FAULT),
              "the last power": (g2[:-1] + [stray], G2_FAULT),
              "two powers swapped": (g2[:3] + [g2[4], g2[3]] + g2[5:], G2_FAULT),
              "a power that is infinity": (g2[:4] + [kzg.Z2] + g2[5:], G2_FAULT)}
    for what, (bad, name) in broken.items():
        assert faults(kzg, ck, bad, 7) == [name, name], what
        assert kzg.check_key(ck, bad, r=7, g2_chain="fold") is False
    # a broken G1 chain is named first by both
    pts = list(ck[:])
    pts[9] = kzg._g1.multiply(kzg.G1, 0xbad)
    assert faults(kzg, pts, g2, 7) == [G1_FAULT, G1_FAULT]
    # the chain of another tau
    assert faults(kzg, ck, kzg.setup_g2(10, 0x77, device=True), 7) == [G1_FAULT, G1_FAULT]   # [tau] G2 enters the G1 chain
    with pytest.raises(ValueError, match="g2_chain must be"):
        kzg.check_key(ck, g2, g2_chain="both")
    # the file route
    path = str(tmp_path / "setup.txt")
    kzg.save_trusted_setup(path, ck, g2)
    back = kzg.load_trusted_setup(path, r=5, g2_chain="fold")
    assert back.g2 == g2
    kzg.save_trusted_setup(path, ck, broken["the last power"][0])
    for chain in ("links", "fold"):
        with pytest.raises(ValueError, match="trusted setup: the sections do not describe one tau: " + re.escape(G2_FAULT)):
            kzg.load_trusted_setup(path, r=5, g2_chain=chain)


@pytest.mark.parametrize("m", [2, 9, 10, 65])
@pytest.mark.parametrize("curve", CURVES)
def test_fold_and_links_agree_at_every_length(kzgs, native, curve, m):
    kzg = kzgs[curve]
    ck = kzg.setup(3, TAU)[0]
    g2 = native.limbs_to_g2_points(*tau_powers(kzg, native, m))
    assert faults(kzg, ck, g2, 11) == [None, None]
    bad = g2[:-1] + [kzg._g2.multiply(g2[-1], 2)]
    name = G1_FAULT if m == 2 else G2_FAULT                          # [tau] G2 itself enters the G1 chain's equation
    assert faults(kzg, ck, bad, 11) == [name, name]

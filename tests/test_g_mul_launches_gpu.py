"""GPU tests of what surrounds the ladder of csrc/g_mul.hip: calls of more than one launch (the lane offset of a later
launch, the table shared by launches of unequal grids, one refusal word for all of them), the power forms beyond the
lower level of the power table, and what the entry points refuse.  Every comparison is exact.  No test does a Python
group operation per lane: whole arrays are compared with arrays from an independent kernel (srs_generate), with products
from curve.Group.multiply laid out by numpy indexing, or -- the G1 `each` form -- folded per launch into one commitment
whose discrete logarithm the host knows.

L1 / L2 are the lanes of one launch at the most, B1 / B2 the workgroup sizes.  n = L + 1 is two launches of unequal
grids, n = 2 L + 1 three; the launch ranges come from GmPlan through the host shim (g_mul_cases.launches)."""
import random
import re

import numpy as np
import pytest

import g_mul_cases as gm
from g_mul_cases import GUARD, guard_ok, guarded, vp
from kzg_snark_amd import curve as C

pytestmark = pytest.mark.gpu

CURVES = gm.CURVES
SIZES = [1, 2]                 # n = SIZES[i] * L + 1
LIMIT = 1 << 21


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


@pytest.fixture(scope="module")
def shim():
    return gm.build_shim()


def caps(native):
    ctx = native.Context
    return ctx.G1_MUL_LAUNCH_LANES, ctx.G2_MUL_LAUNCH_LANES, ctx.G1_MUL_LANES, ctx.G2_MUL_LANES


def spans_of(shim, native, n, g):
    """the launch ranges of a call, checked against what the sizes of this file are chosen for"""
    L1, L2, B1, B2 = caps(native)
    spans = gm.launches(shim, n, g)
    L, B = (L1, B1) if g == 1 else (L2, B2)
    assert len(spans) == (n - 1) // L + 1 >= 2 and all(f % B == 0 and f < e for f, e in spans)
    assert spans[0][0] == 0 and spans[-1][1] == n and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    return spans


def point_of(native, g, xy_row, flag):
    conv = native.limbs_to_points if g == 1 else native.limbs_to_g2_points
    return conv(xy_row.reshape(1, -1), np.array([flag], dtype=np.uint8))[0]


def last_error(native, ctx):
    msg = native.lib().kzg_last_error(ctx._h)
    return msg.decode() if msg else ""


def host_call(native, ctx, g, xy, inf, k):
    """kzg_g1_mul_each / kzg_g2_mul_each through the C ABI with guard bytes behind both outputs -> (rc, xy bytes, flags)"""
    xy, k = np.ascontiguousarray(xy), np.ascontiguousarray(k)
    inf = None if inf is None else np.ascontiguousarray(inf)
    n, width = xy.shape[0], xy.shape[1] * 8
    o_xy, o_inf = guarded(n * width), guarded(n)
    fn = native.lib().kzg_g1_mul_each if g == 1 else native.lib().kzg_g2_mul_each
    rc = fn(ctx._h, vp(xy), None if inf is None else vp(inf), n, vp(k), vp(o_xy), vp(o_inf))
    assert guard_ok(o_xy, n * width) and guard_ok(o_inf, n)
    return rc, o_xy, o_inf


def rows_of(o_xy, o_inf, n, width):
    return o_xy[:n * width * 8].view(np.uint64).reshape(n, width), o_inf[:n]


def device_call(native, ctx, xy, inf, k):
    """kzg_g1_mul_each_device on a stream of the caller's, guard bytes behind both outputs -> (rc, rows, flags)"""
    import torch
    n, width = xy.shape
    dev = f"cuda:{ctx.device}"
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            d_xy, d_k = (torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev) for a in (xy, k))
            d_inf = None if inf is None else torch.from_numpy(inf).to(dev)
            d_oxy, d_oinf = (torch.from_numpy(guarded(b)).to(dev) for b in (n * width * 8, n))
            rc = native.lib().kzg_g1_mul_each_device(ctx._h, d_xy.data_ptr(), None if d_inf is None else d_inf.data_ptr(), n,
                                                     d_k.data_ptr(), d_oxy.data_ptr(), d_oinf.data_ptr())
            stream.synchronize()
            o_xy, o_inf = d_oxy.cpu().numpy(), d_oinf.cpu().numpy()
    finally:
        ctx.set_stream(0)
    assert guard_ok(o_xy, n * width * 8) and guard_ok(o_inf, n)
    return (rc,) + rows_of(o_xy, o_inf, n, width)


# ---- (a) the G1 power form, key to key ----------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_scale_key_equals_the_setup_of_the_product_at_every_lane(kzgs, native, shim, curve, size):
    kzg = kzgs[curve]
    r, G = kzg.curve_order, kzg._g1
    n = size * caps(native)[0] + 1
    spans_of(shim, native, n, 1)
    rng = random.Random(0xa0 + 4 * gm.CURVE_IDS[curve] + size)
    tau, s, c0 = rng.randrange(2, r), rng.randrange(2, r), rng.randrange(2, r)
    ck = kzg.setup(n - 1, tau)[0]
    (xa, ia), (xb, ib) = kzg.scale_key(ck, s).srs.export(), kzg.setup(n - 1, tau * s % r)[0].srs.export()
    assert np.array_equal(xa, xb) and np.array_equal(ia, ib) and not ia.any()
    # c0 != 1: the commitment to a full-length random polynomial under the scaled key
    scaled = kzg.scale_key(ck, s, c0)
    rho = gm.rho_rows(0xa1 + size, n)
    total, t, st = 0, 1, s * tau % r
    for v in native.limbs_to_ints(rho):
        total += v * t
        t = t * st % r
    assert kzg.commit(scaled, [rho]) == [G.normalize(G.multiply(kzg.G1, c0 * total % r))]
    # the same scalars through kzg_g1_mul_powers on the exported points
    xy, inf = ck.srs.export()
    (xa, ia), (xc, ic) = scaled.srs.export(), kzg._context().g1_mul_powers(xy, inf, s, c0)
    assert np.array_equal(xa, xc) and np.array_equal(ia, ic)


# ---- (b) the G1 `each` form ---------------------------------------------------------------------------------------

class G1Each:
    """the inputs of one size on one curve: P_i = [tau^i] G with the flag set at a few lanes, unreduced scalars, the
    coefficients of the fold, and per launch range the discrete logarithm of the folded products"""

    def __init__(self, kzg, native, shim, n):
        curve = kzg.curve_type
        self.n, self.r = n, kzg.curve_order
        self.spans = spans_of(shim, native, n, 1)
        seed = 0xb00 + 16 * gm.CURVE_IDS[curve] + len(self.spans)
        rng = random.Random(seed)
        self.tau = rng.randrange(2, self.r)
        self.xy = kzg.setup(n - 1, self.tau)[0].srs.export()[0]
        self.k, self.special = gm.each_scalars(curve, n, self.spans, seed)
        self.ks = native.limbs_to_ints(self.k)
        self.inf = np.zeros(n, dtype=np.uint8)
        self.inf[[i for i in gm.edge_lanes(self.spans, n, (-2, 2), rng, 4) if i not in self.special]] = 1
        assert self.inf.sum() >= 2 * len(self.spans) - 1
        self.rho = gm.rho_rows(seed + 1, n)
        sums, t, j = [0] * len(self.spans), 1, 0
        for i, (v, k) in enumerate(zip(native.limbs_to_ints(self.rho), self.ks)):
            if i >= self.spans[j][1]:
                j += 1
            if not self.inf[i]:
                sums[j] += v * (k % self.r) * t
            t = t * self.tau % self.r
        self.sums = [v % self.r for v in sums]
        self.flags = (self.inf.astype(bool) | np.array([k % self.r == 0 for k in self.ks])).astype(np.uint8)
        B = native.Context.G1_MUL_LANES
        self.checked = sorted({0, B - 1, B, n - 1} | {f + d for f, _ in self.spans for d in (-1, 0, 1) if 0 <= f + d < n})
        self.valid = None

    def point(self, native, i, use_inf=True):
        return point_of(native, 1, self.xy[i], self.inf[i] if use_inf else 0)


_G1 = {}


def g1_each(kzg, native, shim, size):
    key = (kzg.curve_type, size)
    if key not in _G1:
        _G1[key] = G1Each(kzg, native, shim, size * caps(native)[0] + 1)
    return _G1[key]


def valid_run(kzg, native, d):
    """the host form on the valid inputs, once per size and curve"""
    if d.valid is None:
        rc, o_xy, o_inf = host_call(native, kzg._context(), 1, d.xy, d.inf, d.k)
        assert rc == 0, last_error(native, kzg._context())
        d.valid = rows_of(o_xy, o_inf, d.n, d.xy.shape[1])
    return d.valid


def check_g1_each(kzg, native, d, o_xy, o_inf):
    """every lane of an output of the valid inputs: flags and zero words directly, the finite products folded per
    launch range into one commitment each, chosen lanes against the host reference"""
    from kzg_snark_amd.kzg import CommitmentKey
    G, n = kzg._g1, d.n
    assert np.array_equal(o_inf, d.flags)
    assert not o_xy[d.flags == 1].any()
    ctx = kzg._context()
    key = CommitmentKey(ctx, ctx.srs_load_g1(np.ascontiguousarray(o_xy), np.ascontiguousarray(o_inf)))
    polys = []
    for f, e in d.spans:
        poly = np.zeros((n, 4), dtype=np.uint64)
        poly[f:e] = d.rho[f:e]
        polys.append(poly)
    got = kzg.commit(key, polys)
    key.srs.close()
    for j, (span, have, total) in enumerate(zip(d.spans, got, d.sums)):
        assert have == G.normalize(G.multiply(kzg.G1, total)), "launch %d, lanes [%d, %d)" % ((j,) + span)
    for i in d.checked:
        assert point_of(native, 1, o_xy[i], o_inf[i]) == G.normalize(G.multiply(d.point(native, i), d.ks[i])), i


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_g1_each_host_form_every_lane_of_every_launch(kzgs, native, shim, curve, size):
    kzg = kzgs[curve]
    d = g1_each(kzg, native, shim, size)
    check_g1_each(kzg, native, d, *valid_run(kzg, native, d))


@pytest.mark.parametrize("curve", CURVES)
def test_g1_each_without_flags_differs_at_the_flagged_lanes_only(kzgs, native, shim, curve):
    kzg = kzgs[curve]
    G = kzg._g1
    d = g1_each(kzg, native, shim, 1)
    v_xy, v_inf = valid_run(kzg, native, d)
    rc, o_xy, o_inf = host_call(native, kzg._context(), 1, d.xy, None, d.k)
    assert rc == 0
    o_xy, o_inf = rows_of(o_xy, o_inf, d.n, d.xy.shape[1])
    off = d.inf == 0
    assert np.array_equal(o_xy[off], v_xy[off]) and np.array_equal(o_inf[off], v_inf[off])
    for i in np.flatnonzero(d.inf):
        want = G.normalize(G.multiply(d.point(native, i, use_inf=False), d.ks[i]))
        assert point_of(native, 1, o_xy[i], o_inf[i]) == want, i


@pytest.mark.parametrize("with_inf", [True, False])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_g1_each_device_form_is_the_host_form_byte_for_byte(kzgs, native, shim, curve, size, with_inf):
    kzg = kzgs[curve]
    d = g1_each(kzg, native, shim, size)
    inf = d.inf if with_inf else None
    ctx = native.Context(curve)
    try:
        rc, h_xy, h_inf = host_call(native, ctx, 1, d.xy, inf, d.k)
        assert rc == 0
        h_xy, h_inf = rows_of(h_xy, h_inf, d.n, d.xy.shape[1])
        if with_inf:
            v_xy, v_inf = valid_run(kzg, native, d)
            assert np.array_equal(h_xy, v_xy) and np.array_equal(h_inf, v_inf)
        rc, o_xy, o_inf = device_call(native, ctx, d.xy, inf, d.k)
        assert rc == 0, last_error(native, ctx)
        assert o_xy.tobytes() == h_xy.tobytes() and o_inf.tobytes() == h_inf.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_a_small_call_is_right_before_and_after_the_workspace_grows(kzgs, native, shim, curve):
    kzg = kzgs[curve]
    G = kzg._g1
    d = g1_each(kzg, native, shim, 2)
    assert len(d.spans) == 3
    lanes = d.checked[-3:]
    xy, inf, k = (np.ascontiguousarray(a[lanes]) for a in (d.xy, d.inf, d.k))
    want = [G.normalize(G.multiply(d.point(native, i), d.ks[i])) for i in lanes]
    ctx = native.Context(curve)
    try:
        assert native.limbs_to_points(*ctx.g1_mul_each(xy, inf, k)) == want
        big = ctx.g1_mul_each(d.xy, d.inf, d.k)
        assert native.limbs_to_points(*ctx.g1_mul_each(xy, inf, k)) == want
    finally:
        ctx.close()
    check_g1_each(kzg, native, d, *big)


# ---- (c) the G2 `each` form ---------------------------------------------------------------------------------------

class G2Each:
    """lane i holds point a(i) and scalar b(i) of g_mul_cases.g2_pool, both from one seeded generator"""

    def __init__(self, native, shim, curve, n):
        L = gm.fp_words(C.CURVES[curve]) // 2
        pts, ks, prods = gm.g2_pool(curve)
        rng = random.Random(0xc00 + 8 * gm.CURVE_IDS[curve] + n % 5)
        picks = np.array([(rng.randrange(len(pts)), rng.randrange(len(ks))) for _ in range(n)])
        a, b = picks[:, 0], picks[:, 1]
        p_xy, p_inf = native.g2_points_to_limbs(pts, L)
        w_xy, w_inf = native.g2_points_to_limbs(prods, L)
        self.n, self.spans = n, spans_of(shim, native, n, 2)
        self.xy, self.inf = np.ascontiguousarray(p_xy[a]), np.ascontiguousarray(p_inf[a])
        self.k = np.ascontiguousarray(native.ints_to_limbs(ks)[b])
        self.want_xy, self.want_inf = w_xy[a * len(ks) + b], w_inf[a * len(ks) + b]


_G2 = {}


def g2_each(native, shim, curve, size):
    key = (curve, size)
    if key not in _G2:
        _G2[key] = G2Each(native, shim, curve, size * caps(native)[1] + 1)
    return _G2[key]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_g2_each_every_lane_of_every_launch(kzgs, native, shim, curve, size):
    ctx = kzgs[curve]._context()
    assert ctx.fp_limbs * 2 == gm.fp_words(C.CURVES[curve])
    d = g2_each(native, shim, curve, size)
    assert len(d.spans) == size + 1
    rc, o_xy, o_inf = host_call(native, ctx, 2, d.xy, d.inf, d.k)
    assert rc == 0, last_error(native, ctx)
    o_xy, o_inf = rows_of(o_xy, o_inf, d.n, d.xy.shape[1])
    assert np.array_equal(o_inf, d.want_inf)
    assert np.array_equal(o_xy, d.want_xy)


# ---- (d) the power forms across the levels of the power table -----------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_g2_powers_of_a_scalar_of_odd_order_at_every_lane(kzgs, native, shim, curve):
    kzg = kzgs[curve]
    r, G, L = kzg.curve_order, kzg._g2, kzg._context().fp_limbs
    s, m = gm.odd_order_scalar(curve)
    n = caps(native)[1] + 1
    assert len(spans_of(shim, native, n, 2)) == 2 and n > 4096
    c0 = random.Random(0xd0 + gm.CURVE_IDS[curve]).randrange(2, r)
    g_xy, g_inf = native.g2_points_to_limbs([kzg.G2], L)
    xy = np.ascontiguousarray(np.broadcast_to(g_xy, (n, 4 * L)))
    got_xy, got_inf = kzg._context().g2_mul_powers(xy, np.zeros(n, dtype=np.uint8), s, c0)
    w_xy, w_inf = native.g2_points_to_limbs([G.normalize(G.multiply(kzg.G2, c0 * pow(s, j, r) % r)) for j in range(m)], L)
    lane = np.arange(n) % m
    assert not got_inf.any() and not w_inf.any()
    assert np.array_equal(got_xy, w_xy[lane])
    # setup_g2 on the device is the same kernel with c0 = 1
    powers = kzg.setup_g2(n, s, device=True)
    assert len(powers) == n
    for j in (0, 1, 2047, 2048, 2049, 4096, n - 1):
        assert powers[j] == G.normalize(G.multiply(kzg.G2, pow(s, j % m, r))), j


@pytest.mark.parametrize("curve", CURVES)
def test_g1_powers_of_a_scalar_of_odd_order_at_every_lane(kzgs, native, shim, curve):
    kzg = kzgs[curve]
    r, G, L = kzg.curve_order, kzg._g1, kzg._context().fp_limbs
    s, m = gm.odd_order_scalar(curve)
    n = caps(native)[0] + 1
    assert len(spans_of(shim, native, n, 1)) == 2
    rng = random.Random(0xd8 + gm.CURVE_IDS[curve])
    c0 = rng.randrange(2, r)
    pts = [gm.points(curve, 1)[j][0] for j in (1, 3, 4)]                # G and two random points of the subgroup
    a = np.array([rng.randrange(3) for _ in range(n)])
    p_xy, p_inf = native.points_to_limbs(pts, L)
    got_xy, got_inf = kzg._context().g1_mul_powers(np.ascontiguousarray(p_xy[a]), np.zeros(n, dtype=np.uint8), s, c0)
    w_xy, w_inf = native.points_to_limbs([G.normalize(G.multiply(pt, c0 * pow(s, j, r) % r)) for pt in pts for j in range(m)], L)
    assert not got_inf.any() and not w_inf.any()
    assert np.array_equal(got_xy, w_xy[a * m + np.arange(n) % m])


# ---- (e) refusals ---------------------------------------------------------------------------------------------------

def off_curve_row(native, curve, g, row):
    """the words of a finite point with the lowest bit of y flipped: every coordinate below p, not on the curve"""
    cv = C.CURVES[curve]
    bad = row.copy()
    bad[bad.size // 2] ^= np.uint64(1)
    pt = point_of(native, g, bad, 0)
    ys = [pt[1]] if g == 1 else list(pt[1])
    assert all(c < cv.p for c in ys) and not (C.on_curve_g1 if g == 1 else C.on_curve_g2)(pt, cv)
    return bad


def with_bad_lanes(native, curve, g, xy, inf, good, lanes):
    xy, inf = xy.copy(), inf.copy()
    xy[sorted(lanes)] = off_curve_row(native, curve, g, good)
    inf[sorted(lanes)] = 0
    return xy, inf


def refusal_cases(spans, n):
    first = spans[1][0]
    return [({first + 3}, first + 3), ({first + 3, 5}, 5), ({n - 1}, n - 1)]


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("curve", CURVES)
def test_the_host_forms_name_the_smallest_bad_lane_of_any_launch(kzgs, native, shim, curve, g):
    kzg = kzgs[curve]
    ctx = kzg._context()
    if g == 1:
        d = g1_each(kzg, native, shim, 1)
        want_xy, want_inf = valid_run(kzg, native, d)
        good = d.xy[1]
    else:
        d = g2_each(native, shim, curve, 1)
        want_xy, want_inf = d.want_xy, d.want_inf
        good = native.g2_points_to_limbs([kzg.G2], ctx.fp_limbs)[0][0]
    assert len(d.spans) == 2
    for lanes, named in refusal_cases(d.spans, d.n):
        xy, inf = with_bad_lanes(native, curve, g, d.xy, d.inf, good, lanes)
        rc, o_xy, o_inf = host_call(native, ctx, g, xy, inf, d.k)
        with pytest.raises(native.NativeError, match=r"point \d+ has a coordinate >= p or is not on the") as e:
            ctx._check(rc)
        assert e.value.code == -1
        assert [int(v) for v in re.findall(r"point (\d+) ", str(e.value))] == [named]
        assert (o_xy == GUARD).all() and (o_inf == GUARD).all()
        # the context lives
        rc, o_xy, o_inf = host_call(native, ctx, g, d.xy[:3], d.inf[:3], d.k[:3])
        assert rc == 0
        o_xy, o_inf = rows_of(o_xy, o_inf, 3, d.xy.shape[1])
        assert np.array_equal(o_xy, want_xy[:3]) and np.array_equal(o_inf, want_inf[:3])


@pytest.mark.parametrize("curve", CURVES)
def test_the_device_form_marks_bad_lanes_and_finishes_the_rest(kzgs, native, shim, curve):
    kzg = kzgs[curve]
    d = g1_each(kzg, native, shim, 1)
    v_xy, v_inf = valid_run(kzg, native, d)
    ctx = native.Context(curve)
    try:
        for lanes, _ in refusal_cases(d.spans, d.n):
            xy, inf = with_bad_lanes(native, curve, 1, d.xy, d.inf, d.xy[1], lanes)
            rc, o_xy, o_inf = device_call(native, ctx, xy, inf, d.k)
            assert rc == 0, last_error(native, ctx)
            bad = np.zeros(d.n, dtype=bool)
            bad[sorted(lanes)] = True
            assert not o_xy[bad].any() and (o_inf[bad] == 2).all()
            assert np.array_equal(o_xy[~bad], v_xy[~bad]) and np.array_equal(o_inf[~bad], v_inf[~bad])
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_more_than_2_pow_21_points_are_refused_and_none_are_nothing(kzgs, native, curve):
    """n = 2^21 + 1 with arrays of that size (zeros, every flag 1: were the check missing, the call would write
    infinities over the guard bytes, not fault) through the three host entry points; n = 0 touches nothing."""
    ctx = kzgs[curve]._context()
    lib, L, n = native.lib(), ctx.fp_limbs, LIMIT + 1
    xy, inf, k = np.zeros((n, 4 * L), dtype=np.uint64), np.ones(n, dtype=np.uint8), np.zeros((n, 4), dtype=np.uint64)
    one = native.int_to_words(1)
    o_xy, o_inf = np.full(n * 4 * L * 8, GUARD, dtype=np.uint8), np.full(n, GUARD, dtype=np.uint8)
    calls = {"kzg_g1_mul_each": lambda m: lib.kzg_g1_mul_each(ctx._h, vp(xy), vp(inf), m, vp(k), vp(o_xy), vp(o_inf)),
             "kzg_g2_mul_each": lambda m: lib.kzg_g2_mul_each(ctx._h, vp(xy), vp(inf), m, vp(k), vp(o_xy), vp(o_inf)),
             "kzg_g1_mul_powers": lambda m: lib.kzg_g1_mul_powers(ctx._h, vp(xy), vp(inf), m, vp(one), vp(one), vp(o_xy),
                                                                  vp(o_inf))}
    for name, call in calls.items():
        assert call(n) == -1
        assert last_error(native, ctx) == name + ": more than 2^21 points"
        assert call(0) == 0
    assert (o_xy == GUARD).all() and (o_inf == GUARD).all()


@pytest.mark.parametrize("curve", CURVES)
def test_the_device_form_refuses_sizes_and_misaligned_pointers(kzgs, native, curve):
    import torch
    ctx = kzgs[curve]._context()
    lib, L, n = native.lib(), ctx.fp_limbs, LIMIT + 1
    dev = f"cuda:{ctx.device}"
    width = 2 * L * 8
    d_xy = torch.zeros(n * width + 16, dtype=torch.uint8, device=dev)
    d_k = torch.zeros(n * 32 + 16, dtype=torch.uint8, device=dev)
    d_inf = torch.ones(n, dtype=torch.uint8, device=dev)
    d_oxy = torch.full((n * width + 16,), GUARD, dtype=torch.uint8, device=dev)
    d_oinf = torch.full((n,), GUARD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(ctx.device)

    def call(m, xy=d_xy, k=d_k, oxy=d_oxy):
        return lib.kzg_g1_mul_each_device(ctx._h, xy.data_ptr(), d_inf.data_ptr(), m, k.data_ptr(), oxy.data_ptr(),
                                          d_oinf.data_ptr())

    assert call(n) == -1
    assert last_error(native, ctx) == "kzg_g1_mul_each_device: more than 2^21 points"
    assert call(0) == 0
    # a view one element into a real buffer, each pointer in turn
    for kw in ({"xy": d_xy[1:]}, {"k": d_k[1:]}, {"oxy": d_oxy[1:]}):
        assert next(iter(kw.values())).data_ptr() % 16 == 1
        assert call(3, **kw) == -1
        assert "misaligned" in last_error(native, ctx)
    ctx.synchronize()
    assert bool((d_oxy == GUARD).all()) and bool((d_oinf == GUARD).all())
    # the same three points, aligned, are taken
    assert call(3) == 0
    ctx.synchronize()
    assert not bool(d_oxy[:3 * width].any()) and bool((d_oxy[3 * width:] == GUARD).all())
    assert bool((d_oinf[:3] == 1).all()) and bool((d_oinf[3:] == GUARD).all())

"""GPU tests of the per-point scalar multiplication (csrc/g_mul.hip through the C ABI and the facade): out[i] = [k_i] P_i
in G1 and G2 of both curves.  Every expected point comes from curve.Group.multiply, exact for any point and integer
(KZG.multiply reduces modulo r and is not the reference).  B1 / B2 are the workgroup sizes of the two kernels."""
import random

import numpy as np
import pytest

import g_mul_cases as gm
from g_mul_cases import guard_ok, guarded, vp

pytestmark = pytest.mark.gpu

CURVES = gm.CURVES


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


@pytest.fixture(scope="module")
def lanes(native):
    return native.Context.G1_MUL_LANES, native.Context.G2_MUL_LANES


_POOL = {}


def pool(kzg, g, count):
    """`count` seeded random points of the subgroup with seeded random scalars below r, and the products from the host
    reference for the indices that ask for them: (points, scalars, want(i))"""
    key = (kzg.curve_type, g)
    if key not in _POOL:
        cv, G = kzg._cv, gm.group(kzg.curve_type, g)
        rng = random.Random(0x9a + 2 * gm.CURVE_IDS[kzg.curve_type] + g)
        gen = gm.points(kzg.curve_type, g)[1][0]
        pts = [G.multiply(gen, rng.randrange(1, cv.r)) for _ in range(count)]
        _POOL[key] = (pts, [rng.randrange(cv.r) for _ in range(count)], {})
    pts, ks, memo = _POOL[key]
    assert len(pts) >= count
    G = gm.group(kzg.curve_type, g)

    def want(i):
        if i not in memo:
            memo[i] = G.normalize(G.multiply(pts[i], ks[i]))
        return memo[i]

    return pts, ks, want


# ---- the case list ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("curve", CURVES)
def test_the_case_list_equals_the_host_reference(kzgs, curve, g):
    kzg = kzgs[curve]
    rows = gm.cases(curve, g)
    call = kzg.multiply_each if g == 1 else kzg.multiply_each_g2
    got = call([r[0] for r in rows], [r[1] for r in rows])
    assert len(got) == len(rows)
    for have, (pt, k, want, what) in zip(got, rows):
        assert have == want, (what, hex(k))


# ---- sizes, guards ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_g1_sizes_against_commit_with_guards(kzgs, native, lanes, curve):
    kzg = kzgs[curve]
    ctx, lib = kzg._context(), native.lib()
    B1, L = lanes[0], kzg._context().fp_limbs
    pts, ks, want = pool(kzg, 1, 2 * B1 + 1)
    for n in (0, 1, 63, 64, 65, B1 - 1, B1, B1 + 1, 2 * B1 + 1):
        xy, inf = native.points_to_limbs(pts[:n], L)
        k = native.ints_to_limbs(ks[:n]) if n else np.zeros((0, 4), dtype=np.uint64)
        o_xy, o_inf = guarded(n * 2 * L * 8), guarded(n)
        assert lib.kzg_g1_mul_each(ctx._h, vp(xy), vp(inf), n, vp(np.ascontiguousarray(k)), vp(o_xy), vp(o_inf)) == 0
        assert guard_ok(o_xy, n * 2 * L * 8) and guard_ok(o_inf, n)
        if n == 0:
            assert kzg.multiply_each([], []) == []
            continue
        got = native.limbs_to_points(o_xy[:n * 2 * L * 8].view(np.uint64).reshape(n, 2 * L), o_inf[:n])
        assert got == kzg.multiply_each(pts[:n], ks[:n])
        # call A: the sum of the products; call B: the commitment to the scalars under the points as a key
        assert native.g1_sum(curve, got) == kzg.commit(pts[:n], [ks[:n]])[0]
        assert got[0] == want(0) and got[n - 1] == want(n - 1)


@pytest.mark.parametrize("curve", CURVES)
def test_g2_sizes_against_the_host_reference_with_guards(kzgs, native, lanes, curve):
    kzg = kzgs[curve]
    ctx, lib = kzg._context(), native.lib()
    B2, L = lanes[1], kzg._context().fp_limbs
    pts, ks, want = pool(kzg, 2, B2 + 1)
    for n in (0, 1, 63, 64, 65, B2 + 1):
        xy, inf = native.g2_points_to_limbs(pts[:n], L)
        k = native.ints_to_limbs(ks[:n]) if n else np.zeros((0, 4), dtype=np.uint64)
        o_xy, o_inf = guarded(n * 4 * L * 8), guarded(n)
        assert lib.kzg_g2_mul_each(ctx._h, vp(xy), vp(inf), n, vp(np.ascontiguousarray(k)), vp(o_xy), vp(o_inf)) == 0
        assert guard_ok(o_xy, n * 4 * L * 8) and guard_ok(o_inf, n)
        got = native.limbs_to_g2_points(o_xy[:n * 4 * L * 8].view(np.uint64).reshape(n, 4 * L), o_inf[:n]) if n else []
        assert got == [want(i) for i in range(n)]
        assert got == kzg.multiply_each_g2(pts[:n], ks[:n])
    # the array form returns arrays, and a missing flag array means no point is infinity
    xy, inf = native.g2_points_to_limbs(pts[:3], L)
    o_xy, o_inf = kzg.multiply_each_g2((xy, None), ks[:3])
    assert native.limbs_to_g2_points(o_xy, o_inf) == [want(i) for i in range(3)]


# ---- the power form -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_scale_key_is_the_setup_of_the_product(kzgs, native, lanes, curve):
    kzg = kzgs[curve]
    r = kzg.curve_order
    n = 2 * lanes[0] + 1
    tau, s, c0 = 0x1234567 + 3 * n, 0xfeedc0de1f, 0xabcdef0123456789
    ck = kzg.setup(n - 1, tau)[0]
    want = kzg.setup(n - 1, tau * s % r)[0]
    got = kzg.scale_key(ck, s)
    assert len(got) == n
    (xa, ia), (xb, ib) = got.srs.export(), want.srs.export()
    assert np.array_equal(xa, xb) and np.array_equal(ia, ib)
    # the new handle is a key like any other: it commits
    poly = [5, 0, 7] + [0] * (n - 4) + [11]
    assert kzg.commit(got, [poly]) == kzg.commit(want, [poly])
    # c0 != 1, against multiply_each with the scalars from the host
    xy, inf = ck.srs.export()
    ks = [c0 * pow(s, i, r) % r for i in range(n)]
    (xa, ia), (xb, ib) = kzg.scale_key(ck, s, c0).srs.export(), kzg.multiply_each((xy, inf), ks)
    assert np.array_equal(xa, xb) and np.array_equal(ia, ib)
    # the same through kzg_g1_mul_powers on the exported points
    xc, ic = kzg._context().g1_mul_powers(xy, inf, s, c0)
    assert np.array_equal(xa, xc) and np.array_equal(ia, ic)
    # a Lagrange-tagged handle is scaled all the same, and the result is a plain key
    lk = kzg.setup_lagrange(2 * lanes[0], tau)[0]
    xy, inf = lk.srs.export()
    scaled = kzg.scale_key(lk, s, c0)
    assert type(scaled).__name__ == "CommitmentKey" and scaled.srs.basis is None
    (xa, ia), (xb, ib) = scaled.srs.export(), kzg.multiply_each((xy, inf), ks[:len(lk)])
    assert np.array_equal(xa, xb) and np.array_equal(ia, ib)


@pytest.mark.parametrize("curve", CURVES)
def test_g2_powers(kzgs, native, curve):
    kzg = kzgs[curve]
    r, L = kzg.curve_order, kzg._context().fp_limbs
    tau, s = 0x5eed5eed5eed, 0x77aa55
    xy, inf = native.g2_points_to_limbs(kzg.setup_g2(5, tau), L)
    got = native.limbs_to_g2_points(*kzg._context().g2_mul_powers(xy, inf, s, 1))
    assert got == kzg.setup_g2(5, tau * s % r)
    assert kzg.setup_g2(9, tau, device=True) == kzg.setup_g2(9, tau)
    assert kzg.setup_g2(0, tau, device=True) == [] and kzg.setup_g2(3, 0, device=True) == kzg.setup_g2(3, 0)


# ---- the device form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_the_device_form_on_a_caller_stream(kzgs, native, lanes, curve):
    import torch
    kzg = kzgs[curve]
    n = lanes[0] + 1
    pts, ks, want = pool(kzg, 1, 2 * lanes[0] + 1)
    ctx = native.Context(curve)
    try:
        L = ctx.fp_limbs
        xy, inf = native.points_to_limbs(pts[:n], L)
        inf[1] = 1
        k = np.ascontiguousarray(native.ints_to_limbs(ks[:n]))
        h_xy, h_inf = ctx.g1_mul_each(xy, inf, k)
        dev = f"cuda:{ctx.device}"
        stream = torch.cuda.Stream(device=dev)
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_xy, d_inf, d_k = (torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev) for a in (xy, inf, k))
            d_oxy, d_oinf = (torch.from_numpy(guarded(b)).to(dev) for b in (n * 2 * L * 8, n))
            ctx.g1_mul_each_device(d_xy.data_ptr(), d_inf.data_ptr(), n, d_k.data_ptr(), d_oxy.data_ptr(), d_oinf.data_ptr())
            stream.synchronize()
            o_xy, o_inf = d_oxy.cpu().numpy(), d_oinf.cpu().numpy()
        ctx.set_stream(0)
        assert guard_ok(o_xy, n * 2 * L * 8) and guard_ok(o_inf, n)
        assert np.array_equal(o_xy[:n * 2 * L * 8].view(np.uint64).reshape(n, 2 * L), h_xy)
        assert np.array_equal(o_inf[:n], h_inf) and h_inf[1] == 1 and not h_inf[0]
        assert native.limbs_to_points(h_xy[:1], h_inf[:1]) == [want(0)]
    finally:
        ctx.close()


# ---- bad input ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_bad_input_is_refused_by_name_and_the_context_lives(kzgs, native, curve):
    kzg = kzgs[curve]
    cv, r = kzg._cv, kzg.curve_order
    n = 70
    for g, call in ((1, kzg.multiply_each), (2, kzg.multiply_each_g2)):
        pts, ks, want = pool(kzg, g, 65 if g == 2 else 513)
        pts = (pts * 2)[:n]
        good = pts[3]
        if g == 1:
            big, off = (cv.p, good[1], 1), (good[0], good[1] ^ 1, 1)
        else:
            big, off = ((cv.p, good[0][1]), good[1], (1, 0)), (good[0], (good[1][0] ^ 1, good[1][1]), (1, 0))
        for index, bad in ((5, big), (0, off), (n - 1, off)):
            rows = list(pts)
            rows[index] = bad
            with pytest.raises(ValueError, match=r"point %d has a coordinate >= p or is not on the" % index):
                call(rows, [7] * n)
        with pytest.raises(ValueError, match=r"scalar 2 is not in \[0, 2\^256\)"):
            call(pts[:3], [1, 2, 1 << 256])
        assert call(pts[:2], [ks[0], ks[1]]) == [want(0), want(1)]                  # still usable
    ck = kzg.setup(3, 99)[0]
    xy, inf = ck.srs.export()
    for args in ((r, 1), (1, r)):
        with pytest.raises(ValueError, match="scale_key: (s|c0) must be"):
            kzg.scale_key(ck, *args)
        with pytest.raises(native.NativeError, match="(s|c0) is not below the group order") as e:
            kzg._context().g1_mul_powers(xy, inf, *args)
        assert e.value.code == -1
        with pytest.raises(native.NativeError, match="kzg_srs_mul_powers: (s|c0) is not below"):
            kzg._context().srs_mul_powers(ck.srs, *args)
    assert kzg.scale_key(ck, 2)[1] == kzg._g1.multiply(ck[1], 2)

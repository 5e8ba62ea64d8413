"""GPU parity of evaluation-form KZG (csrc/lagrange.hip through the C ABI and the facade).  Everything is exact:
the Lagrange key equals the inverse G1 DFT of the monomial key and [L_i(tau)] G1 from the oracle, a commitment to
values equals the coefficient commitment of their interpolant, an opening from values equals the coefficient opening
of the interpolants -- compared on canonical affine coordinates, bit for bit."""
import random

import numpy as np
import pytest

from oracle import c_oracle
from oracle import py_oracle as O

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


_KEYS = {}


def keys(kzg, log_n):
    """(monomial key of n points, Lagrange key from tau) for one curve and domain, cached for the module."""
    k = (kzg.curve_type, log_n)
    if k not in _KEYS:
        n = 1 << log_n
        ck, _ = kzg.setup(n - 1, tau=TAU)
        lk, _ = kzg.setup_lagrange(n, tau=TAU)
        _KEYS[k] = (ck, lk)
    return _KEYS[k]


def exported(key):
    """canonical affine points of a device key: (x, y) or None"""
    from kzg_snark_amd import _native
    xy, inf = key.srs.export()
    L = key._ctx.fp_limbs
    ints = _native.limbs_to_ints(xy.reshape(-1, L))
    return [None if inf[i] else (ints[2 * i], ints[2 * i + 1]) for i in range(len(inf))]


def aff(pt):
    return None if pt[2] == 0 else (pt[0], pt[1])


def rand_values(rng, n, r):
    return [rng.randrange(r) for _ in range(n)]


def interpolate(native, ctx, vals, log_n, w):
    """coefficients of the interpolant of len(vals) <= n values (zero-padded) over {w^i}: the device inverse NTT
    (tests/test_ntt_gpu.py pins it to the oracle), as a uint64[n, 4] buffer"""
    data = np.zeros((1 << log_n, 4), dtype=np.uint64)
    if len(vals):
        data[:len(vals)] = native.ints_to_limbs([int(v) for v in vals])
    ctx.ntt(data, log_n, native.int_to_words(w), True)
    return data


def lagrange_scalars(n, w, tau, r):
    """L_i(tau) = (tau^n - 1)/n * w^i / (tau - w^i), e_m for tau = w^m"""
    wi = [pow(w, i, r) for i in range(n)]
    if tau in wi:
        return [1 if x == tau else 0 for x in wi]
    c = (pow(tau, n, r) - 1) * pow(n, -1, r) % r
    return [c * x * pow(tau - x, -1, r) % r for x in wi]


# ---- 1. key from tau ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [2, 4, 16, 64])
def test_key_from_tau_matches_the_oracle(kzgs, native, curve, n):
    kzg, cv = kzgs[curve], O.curve(curve)
    w = cv.root_of_unity(n)
    lk, tau_g2 = kzg.setup_lagrange(n, tau=TAU)
    assert len(lk) == n and (lk.n, lk.w) == (n, w) and lk.srs.basis == (n.bit_length() - 1, w)
    assert tau_g2 == kzg.multiply(kzg.G2, TAU)
    L = native.lib().kzg_fp_limbs(native.CURVE_IDS[curve])
    gxy = native.ints_to_limbs(list(cv.g1), L).reshape(-1)
    want = []
    for s in lagrange_scalars(n, w, TAU % cv.r, cv.r):
        out, inf = c_oracle.g1_mul(curve, gxy, s)
        want.append(None if inf else tuple(native.limbs_to_ints(out.reshape(2, L))))
    assert exported(lk) == want


@pytest.mark.parametrize("curve", CURVES)
def test_key_from_tau_in_the_domain_is_a_unit_vector(kzgs, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    w = cv.root_of_unity(16)
    lk, _ = kzg.setup_lagrange(16, tau=pow(w, 3, cv.r))
    pts = exported(lk)
    assert pts[3] == tuple(cv.g1)
    assert all(p is None for i, p in enumerate(pts) if i != 3)


# ---- 2. key from a monomial key (inverse G1 NTT) -----------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [1, 6, 12, 16])
def test_key_from_a_monomial_key_equals_the_key_from_tau(kzgs, curve, log_n):
    kzg = kzgs[curve]
    n = 1 << log_n
    ck, lk = keys(kzg, log_n)
    want = exported(lk)
    assert exported(kzg.lagrange_key(ck, n)) == want
    longer, _ = kzg.setup(2 * n + 4, tau=TAU)                         # only the first n points are read
    assert exported(kzg.lagrange_key(longer, n)) == want


@pytest.mark.parametrize("curve", CURVES)
def test_key_from_loaded_random_points_is_their_inverse_dft(kzgs, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(7)
    n, r = 16, cv.r
    G = O.from_affine(cv.g1)
    pts = [O.multiply(G, rng.randrange(1, r), cv) for _ in range(n)]
    pts[5] = O.Z1()                                                   # infinity is a valid key point too
    pts[9] = pts[2]                                                   # and so are repeated ones
    w = cv.root_of_unity(n)
    lk = kzg.lagrange_key([(p[0], p[1], p[2]) for p in pts], n)       # list form: kzg_srs_load_g1, no tau
    winv, ninv = pow(w, -1, r), pow(n, -1, r)
    want = []
    for i in range(n):
        acc = O.Z1()
        for j in range(n):
            acc = O.add(acc, O.multiply(pts[j], ninv * pow(winv, i * j, r) % r, cv), cv)
        want.append(O.normalize(acc, cv))
    assert exported(lk) == want


# ---- 3. commit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [12, 16])
def test_commit_evaluations_equals_the_coefficient_commit(kzgs, native, curve, log_n):
    kzg, cv = kzgs[curve], O.curve(curve)
    n, r = 1 << log_n, cv.r
    ck, lk = keys(kzg, log_n)
    ctx = kzg._context()
    rng = random.Random(log_n)
    cases = [rand_values(rng, n, r), [0] * n, rand_values(rng, n // 3, r), [0] * 17 + [1] + [0] * (n - 18),
             [rng.randrange(r)] + [0] * (n - 1)]
    got = kzg.commit_evaluations(lk, cases)
    assert got[1] == kzg.Z1
    for vals, c in zip(cases, got):
        assert c == kzg.commit(ck, [interpolate(native, ctx, vals, log_n, lk.w)])[0]


def test_commit_evaluations_2_20_equals_the_coefficient_commit_and_the_trapdoor(kzgs, native):
    kzg, cv = kzgs["bls12_381"], O.curve("bls12_381")
    log_n, r = 20, cv.r
    n = 1 << log_n
    lk, _ = kzg.setup_lagrange(n, tau=TAU)
    rng = np.random.default_rng(20)
    vals = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    vals[:, 3] >>= 4                                                  # < 2^252 < r
    got = kzg.commit_evaluations(lk, [vals])[0]
    ints = native.limbs_to_ints(vals)
    lam = lagrange_scalars_fast(n, lk.w, TAU % r, r)
    ptau = sum(v * s for v, s in zip(ints, lam)) % r
    assert aff(got) == O.normalize(O.multiply(O.from_affine(cv.g1), ptau, cv), cv)
    ck, _ = kzg.setup(n - 1, tau=TAU)
    coeffs = vals.copy()
    kzg._context().ntt(coeffs, log_n, native.int_to_words(lk.w), True)
    assert got == kzg.commit(ck, [coeffs])[0]


def lagrange_scalars_fast(n, w, tau, r):
    """lagrange_scalars with one modular inversion (Montgomery's trick), for 2^20 points"""
    wi, x = [], 1
    for _ in range(n):
        wi.append(x)
        x = x * w % r
    d = [(tau - x) % r for x in wi]
    pre, acc = [], 1
    for v in d:
        pre.append(acc)
        acc = acc * v % r
    inv = pow(acc, -1, r)
    out = [0] * n
    c = (pow(tau, n, r) - 1) * pow(n, -1, r) % r
    for i in range(n - 1, -1, -1):
        out[i] = c * wi[i] % r * (inv * pre[i] % r) % r
        inv = inv * d[i] % r
    return out


# ---- 4. open -----------------------------------------------------------------------------------------------------
def _open_pair(native, ctx, ck, lk, vals, log_n, z, xi):
    """(coefficient opening of the interpolants, opening from values) through the C ABI: (xy, inf, eval) each"""
    n = 1 << log_n
    k = len(vals)
    arr = np.zeros((max(k, 1), n, 4), dtype=np.uint64)
    coeffs = np.zeros((max(k, 1), n, 4), dtype=np.uint64)
    for j, v in enumerate(vals):
        if len(v):
            arr[j, :len(v)] = v if isinstance(v, np.ndarray) else native.ints_to_limbs(v)
        coeffs[j] = arr[j]
        ctx.ntt(coeffs[j], log_n, native.int_to_words(lk.w), True)     # the interpolant (zero-padded values)
    lens = [len(v) for v in vals]
    zw, xw = native.int_to_words(z), native.int_to_words(xi)
    want = ctx.open(ck.srs, coeffs, [n] * k, n, zw, xw)
    got = ctx.open_evals(lk.srs, arr, lens, n, zw, xw)
    return want, got


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [1, 2, 10, 16])
def test_open_evaluations_equals_the_coefficient_open(kzgs, native, curve, log_n):
    kzg, cv = kzgs[curve], O.curve(curve)
    n, r = 1 << log_n, cv.r
    ck, lk = keys(kzg, log_n)
    ctx = kzg._context()
    rng = random.Random(100 + log_n)
    w = lk.w
    zs = [rng.randrange(r), 0, 1, w, pow(w, n - 1, r)]
    for k in (1, 6):
        vals = [rand_values(rng, n if j % 3 else max(1, n // 2), r) for j in range(k)]
        for z in zs:
            for xi in (0, 1, rng.randrange(r)):
                (wxy, winf, wev), (gxy, ginf, gev) = _open_pair(native, ctx, ck, lk, vals, log_n, z, xi)
                assert ginf[0] == winf[0] and np.array_equal(gxy, wxy), (k, z, xi)
                assert np.array_equal(gev, wev), (k, z, xi)
    # the facade: same point as open() on the interpolants
    z, xi = rng.randrange(r), rng.randrange(r)
    polys = [interpolate(native, ctx, v, log_n, w) for v in vals[:2]]
    assert kzg.open_evaluations(lk, vals[:2], z, xi) == kzg.open(ck, polys, z, xi)
    assert kzg.open_evaluations(lk, vals[:2], w, xi) == kzg.open(ck, polys, w, xi)


def test_open_evaluations_k6_at_2_20(kzgs, native):
    kzg, cv = kzgs["bls12_381"], O.curve("bls12_381")
    log_n = 20
    n, r = 1 << log_n, cv.r
    ck, _ = kzg.setup(n - 1, tau=TAU)
    lk = kzg.lagrange_key(ck, n)
    ctx = kzg._context()
    g = np.random.default_rng(6)
    vals = []
    for _ in range(6):
        v = g.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
        v[:, 3] >>= 4
        vals.append(v)
    rng = random.Random(6)
    for z in (rng.randrange(r), pow(lk.w, 12345, r)):
        (wxy, winf, wev), (gxy, ginf, gev) = _open_pair(native, ctx, ck, lk, vals, log_n, z, rng.randrange(r))
        assert ginf[0] == winf[0] and np.array_equal(gxy, wxy) and np.array_equal(gev, wev)


# ---- 5. pipelined ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_pipelined_open_evals_matches_the_synchronous_one(kzgs, native, curve):
    import torch
    kzg, cv = kzgs[curve], O.curve(curve)
    log_n = 12
    n, r = 1 << log_n, cv.r
    ck, lk = keys(kzg, log_n)
    ctx = native.Context(curve)
    stream = torch.cuda.Stream(device="cuda:0")
    ctx.bind_torch_stream(stream)
    L = ctx.fp_limbs
    lsrs = ctx.srs_generate_lagrange(native.int_to_words(TAU), log_n, lk.w)
    rng = random.Random(55)
    g = torch.Generator(device="cuda:0").manual_seed(55)
    w = lk.w
    cases = [[n, n - 1, 77], [n], [1, 1], [0, 0], [n] * 6, [5]]
    jobs = []
    with torch.cuda.stream(stream):
        buf = torch.zeros((6, n, 4), dtype=torch.int64, device="cuda:0")
        for i, lens in enumerate(cases):
            fresh = torch.randint(0, 1 << 62, (6, n, 4), generator=g, dtype=torch.int64, device="cuda:0")
            fresh[..., 3] >>= 3
            z = pow(w, i, r) if i % 2 else rng.randrange(r)
            zw, xw = native.int_to_words(z), native.int_to_words(rng.randrange(r))
            want = ctx.open_evals(lsrs, fresh.data_ptr(), lens, n, zw, xw, device=True)
            cwant = ctx.commit_device(lsrs, fresh.data_ptr(), [lens[0]], n)
            buf.copy_(fresh)
            out = (np.zeros(2 * L, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(4, dtype=np.uint64))
            ctx.open_evals_device_async(lsrs, buf.data_ptr(), lens, n, zw, xw, *out)
            cxy, cinf = np.zeros((1, 2 * L), dtype=np.uint64), np.zeros(1, dtype=np.uint8)
            ctx.commit_device_async(lsrs, buf.data_ptr(), [lens[0]], n, cxy, cinf)     # shares the slots
            buf.random_(0, 1 << 62)                                                      # overwritten at once
            jobs.append((want, out, (cxy, cinf), cwant))
        ctx.commit_flush()
    for (wxy, winf, wev), (xy, inf, ev), (cxy, cinf), (cwxy, cwinf) in jobs:
        assert inf[0] == winf[0] and np.array_equal(xy, wxy) and np.array_equal(ev, wev)
        assert cinf[0] == cwinf[0] and np.array_equal(cxy, cwxy)
    ctx.close()


# ---- 6. barycentric evaluation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [1, 4, 12])
def test_evaluate_evaluations_equals_the_interpolant_at_z(kzgs, native, curve, log_n):
    kzg, cv = kzgs[curve], O.curve(curve)
    n, r = 1 << log_n, cv.r
    w = cv.root_of_unity(n)
    rng = random.Random(log_n)
    for vals in (rand_values(rng, n, r), rand_values(rng, max(1, n // 2 + 1), r)):
        coeffs = O.ifft_ff([int(v) for v in vals] + [0] * (n - len(vals)), w, r)
        for z in (rng.randrange(r), 0, 1, w, pow(w, n - 1, r), pow(w, n // 2, r)):
            assert int(kzg.evaluate_evaluations(w, vals, z)) == O.poly_eval(coeffs, z, r), z
    assert int(kzg.evaluate_evaluations(w, [], 5)) == 0
    if log_n == 4:
        _, lk = keys(kzg, log_n)
        assert int(kzg.evaluate_evaluations(lk, vals, 7)) == O.poly_eval(coeffs, 7, r)


# ---- 7. verification ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_evaluation_form_proofs_verify(kzgs, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    n, r = 16, cv.r
    lk, tau_g2 = kzg.setup_lagrange(n, tau=TAU)
    rng = random.Random(77)
    vals = [rand_values(rng, n, r) for _ in range(3)]
    C = kzg.commit_evaluations(lk, vals)
    z, xi = rng.randrange(r), rng.randrange(r)
    ev = [kzg.evaluate_evaluations(lk, v, z) for v in vals]
    proof = kzg.open_evaluations(lk, vals, z, xi)
    assert kzg.check(tau_g2, C, z, ev, proof, xi)
    z2, xi2 = pow(lk.w, 5, r), rng.randrange(r)                       # z in the domain: the values themselves
    ev2 = [kzg.evaluate_evaluations(lk, v, z2) for v in vals[:2]]
    assert [int(e) for e in ev2] == [vals[0][5], vals[1][5]]
    proof2 = kzg.open_evaluations(lk, vals[:2], z2, xi2)
    assert kzg.check(tau_g2, C[:2], z2, ev2, proof2, xi2)
    assert kzg.batch_check(tau_g2, [C, C[:2]], [z, z2], [ev, ev2], [proof, proof2], [xi, xi2], r=12345)
    bad = list(ev2)
    bad[1] = bad[1] + 1
    assert not kzg.check(tau_g2, C[:2], z2, bad, proof2, xi2)
    assert not kzg.batch_check(tau_g2, [C, C[:2]], [z, z2], [ev, bad], [proof, proof2], [xi, xi2], r=12345)


# ---- 8. errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_errors(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    ck, lk = keys(kzg, 4)
    ctx = kzg._context()
    n = 16
    w = lk.w
    arr = native.ints_to_limbs(list(range(1, 2 * n + 1))).reshape(1, 2 * n, 4)
    zw, xw = native.int_to_words(3), native.int_to_words(5)

    def code(fn, *a):
        with pytest.raises(native.NativeError) as e:
            fn(*a)
        return e.value.code

    assert code(ctx.open_evals, ck.srs, arr, [n], 2 * n, zw, xw) == -1                  # monomial key
    assert code(ctx.open_evals, lk.srs, arr, [n + 1], 2 * n, zw, xw) == native.KZG_ERR_DEGREE
    tw = native.int_to_words(TAU)
    assert code(ctx.srs_generate_lagrange, tw, 4, w * w % r) == -1                      # w of order 8, not 16
    assert code(ctx.srs_generate_lagrange, tw, 4, 1) == -1
    assert code(ctx.srs_lagrange, ck.srs, 4, pow(w, 2, r)) == -1
    assert code(ctx.srs_lagrange, ck.srs, 5, cv.root_of_unity(32)) == -1                # key shorter than n
    assert code(ctx.srs_lagrange, lk.srs, 4, w) == -1                                   # source is no monomial key
    import torch
    d = torch.from_numpy(arr.view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert code(ctx.eval_lagrange, 4, w * w % r, n, d.data_ptr(), 3) == -1
    assert code(ctx.eval_lagrange, 4, w, n + 1, d.data_ptr(), 3) == native.KZG_ERR_DEGREE
    with pytest.raises(ValueError):
        kzg.commit_evaluations(lk, [list(range(n + 1))])
    with pytest.raises(ValueError):
        kzg.open_evaluations(lk, [list(range(n + 1))], 3, 5)


# ---- 9. profiler spans -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_one_open_evals_poly_span_per_opening(kzgs, native, curve):
    import torch
    kzg, cv = kzgs[curve], O.curve(curve)
    _, lk = keys(kzg, 12)
    ctx = kzg._context()
    n, k = 1 << 12, 3
    rng = random.Random(9)
    arr = native.ints_to_limbs([rng.randrange(cv.r) for _ in range(n * k)]).reshape(k, n, 4)
    d = torch.from_numpy(arr.view(np.int64)).cuda()
    torch.cuda.synchronize()
    zw, xw = native.int_to_words(rng.randrange(cv.r)), native.int_to_words(rng.randrange(cv.r))
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for _ in range(3):
            ctx.open_evals(lk.srs, d.data_ptr(), [n] * k, n, zw, xw, device=True)
        outs = [(np.zeros(2 * ctx.fp_limbs, np.uint64), np.zeros(1, np.uint8), np.zeros(4, np.uint64)) for _ in range(4)]
        for o in outs:
            ctx.open_evals_device_async(lk.srs, d.data_ptr(), [n] * k, n, zw, xw, *o)
        ctx.commit_flush()
        ms, cnt = ctx.prof_read("open_evals_poly")
        assert cnt == 7 and ms > 0
        assert ctx.prof_read("open_poly")[1] == 0
    finally:
        ctx.prof_enable(False)

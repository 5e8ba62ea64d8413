"""GPU parity of coset openings (csrc/domain.hip's coset FK20 and csrc/poly.hip's coset division, through the C ABI
and the facade): every coset proof equals the commitment of (p - rho) / (X^l - h^l) -- the oracle's, the trapdoor
form's, kzg_open_coset's and, for l = 1, kzg_open_domain's / kzg_open's -- compared on canonical affine coordinates
and infinity flags, bit for bit; the values equal p at the coset's points."""
import random

import numpy as np
import pytest

from coset_scan_profiles import coset_divide
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


def mono_key(kzg, n, tau=TAU):
    k = (kzg.curve_type, n, tau)
    if k not in _KEYS:
        _KEYS[k] = kzg.setup(n - 1, tau=tau)[0]
    return _KEYS[k]


def pack(native, polys, stride):
    arr = np.zeros((len(polys), max(stride, 1), 4), dtype=np.uint64)
    for j, p in enumerate(polys):
        if p:
            arr[j, :len(p)] = native.ints_to_limbs([int(c) for c in p])
    return arr


def points(native, L, xy, inf):
    """[b][c] device output -> nested lists of (x, y) / None"""
    b, n = inf.shape
    ints = native.limbs_to_ints(np.ascontiguousarray(xy).reshape(-1, L))
    return [[None if inf[j, i] else (ints[2 * (j * n + i)], ints[2 * (j * n + i) + 1]) for i in range(n)]
            for j in range(b)]


def one_point(native, L, xy, inf):
    return None if inf[0] else tuple(native.limbs_to_ints(np.asarray(xy).reshape(2, L)))


def coset_interpolate(values, h, zeta, r):
    """rho_j = h^-j l^-1 sum_k y_k zeta^(-jk)"""
    l = len(values)
    zi, hi, li = pow(zeta, -1, r), pow(h, -1, r), pow(l, -1, r)
    return [sum(y * pow(zi, j * k, r) for k, y in enumerate(values)) * li * pow(hi, j, r) % r for j in range(l)]


def g1_scalar(curve, cv, s):
    """[s] G1 through the C oracle, as (x, y) / None"""
    g = _xy_limbs(curve, cv.g1)
    xy, inf = c_oracle.g1_mul(curve, g, s % cv.r)
    return None if inf else tuple(_ints(xy))


def _xy_limbs(curve, xy):
    from kzg_snark_amd import _native
    L = _native.lib().kzg_fp_limbs(_native.CURVE_IDS[curve])
    return _native.ints_to_limbs(list(xy), L).reshape(-1)


def _ints(xy):
    from kzg_snark_amd import _native
    L = len(xy) // 2
    return _native.limbs_to_ints(np.asarray(xy).reshape(2, L))


def oracle_proof(curve, cv, coeffs, l, h, tau=TAU):
    """[q(tau)] G1, q = (p - rho) / (X^l - h^l) from the coefficients (valid for tau on the coset too)"""
    r = cv.r
    q, _ = coset_divide(coeffs, l, pow(h, l, r), r)
    return g1_scalar(curve, cv, O.poly_eval(q, tau, r))


def trapdoor_proof(curve, cv, p_tau, values, h, zeta, l, tau=TAU):
    """[(p(tau) - rho(tau)) / (tau^l - h^l)] G1 with rho interpolated from the values (tau off the coset)"""
    r = cv.r
    rho = coset_interpolate(values, h, zeta, r)
    s = (p_tau - O.poly_eval(rho, tau, r)) * pow((pow(tau, l, r) - pow(h, l, r)) % r, -1, r) % r
    return g1_scalar(curve, cv, s)


def edge_inputs(n, l, r, rng):
    return [[rng.randrange(r) for _ in range(n)], [r - 1] * n, [rng.randrange(r) for _ in range(max(1, l - 1))],
            [rng.randrange(r)], []]


def run(native, ctx, table, polys, log_N, w, evals=True):
    stride = max(max((len(p) for p in polys), default=1), 1)
    xy, inf, ev = ctx.open_cosets(table, pack(native, polys, stride), [len(p) for p in polys], stride, log_N, w,
                                  evals=evals)
    return points(native, ctx.fp_limbs, xy, inf), ev


def _values(native, ev_j):
    """[C][l][4] -> nested ints"""
    C, l = ev_j.shape[0], ev_j.shape[1]
    ints = native.limbs_to_ints(np.ascontiguousarray(ev_j).reshape(-1, 4))
    return [[ints[i * l + k] for k in range(l)] for i in range(C)]


# ---- 1. bit-exact against the oracle, n = 2 .. 16, every l, N in {n, 2n} --------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_every_coset_proof_and_value_equals_the_oracle(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(1)
    ctx = kzg._context()
    for log_n in range(1, 5):
        n = 1 << log_n
        ck = mono_key(kzg, n)
        for log_l in range(log_n):
            l = 1 << log_l
            table = ctx.coset_table(ck.srs, log_n, log_l)
            for log_N in (log_n, log_n + 1):
                N = 1 << log_N
                w = cv.root_of_unity(N)
                polys = edge_inputs(n, l, r, rng)
                got, ev = run(native, ctx, table, polys, log_N, w)
                for j, p in enumerate(polys):
                    vals = _values(native, ev[j])
                    for i in range(N // l):
                        h = pow(w, i, r)
                        assert vals[i] == [O.poly_eval(p, pow(w, i + k * (N // l), r), r) for k in range(l)]
                        assert got[j][i] == oracle_proof(curve, cv, p, l, h), (n, l, N, j, i)
                    if len(p) <= l:
                        assert all(q is None for q in got[j])


# ---- 2. l = 1 is open_domain -------------------------------------------------------------------------------------
def test_l1_equals_open_domain_at_2_12(kzgs, native):
    curve = "bls12_381"
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(2)
    n, log_n = 1 << 12, 12
    ctx = kzg._context()
    table = ctx.domain_table(mono_key(kzg, n).srs, log_n)
    w = cv.root_of_unity(n)
    polys = [[rng.randrange(cv.r) for _ in range(n)], [rng.randrange(cv.r) for _ in range(77)]]
    arr = pack(native, polys, n)
    dxy, dinf, dev = ctx.open_domain(table, arr, [n, 77], n, w)
    cxy, cinf, cev = ctx.open_cosets(table, arr, [n, 77], n, log_n, w)
    assert np.array_equal(dxy, cxy) and np.array_equal(dinf, cinf)
    assert np.array_equal(dev, cev.reshape(dev.shape))


# ---- 3. 2^12 and 2^16: trapdoor form per coset, values against kzg_ntt --------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n,l,sample", [(12, 16, None), (16, 64, 96)])
def test_trapdoor_and_values(kzgs, native, curve, log_n, l, sample):
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(log_n)
    n = 1 << log_n
    ctx = kzg._context()
    table = ctx.coset_table(mono_key(kzg, n).srs, log_n, l.bit_length() - 1)
    p = [rng.randrange(r) for _ in range(n)]
    p_tau = O.poly_eval(p, TAU, r)
    for log_N in (log_n, log_n + 1):
        N = 1 << log_N
        w = cv.root_of_unity(N)
        got, ev = run(native, ctx, table, [p], log_N, w)
        data = np.zeros((N, 4), dtype=np.uint64)
        data[:n] = native.ints_to_limbs(p)
        ctx.ntt(data, log_N, native.int_to_words(w), False)
        C = N // l
        assert np.array_equal(ev[0].reshape(C, l, 4).transpose(1, 0, 2).reshape(N, 4), data)
        vals = _values(native, ev[0])
        zeta = pow(w, C, r)
        idx = range(C) if sample is None else rng.sample(range(C), sample)
        for i in idx:
            assert got[0][i] == trapdoor_proof(curve, cv, p_tau, vals[i], pow(w, i, r), zeta, l), (log_N, i)


# ---- 4. 2^20 on BLS12-381 -------------------------------------------------------------------------------------------
def test_2_20_bls_sampled_cosets_equal_open_coset_and_trapdoor(kzgs, native):
    curve = "bls12_381"
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(20)
    log_n = 20
    n = 1 << log_n
    ctx = kzg._context()
    ck = mono_key(kzg, n)
    p = [rng.randrange(r) for _ in range(n)]
    arr = pack(native, [p], n)
    p_tau = O.poly_eval(p, TAU, r)
    for l in (16, 64):
        table = ctx.coset_table(ck.srs, log_n, l.bit_length() - 1)
        for log_N in (log_n, log_n + 1):
            N = 1 << log_N
            w = cv.root_of_unity(N)
            C = N // l
            got, ev = run(native, ctx, table, [p], log_N, w)
            zeta = pow(w, C, r)
            for i in [0, C - 1] + rng.sample(range(1, C - 1), 2):
                h = pow(w, i, r)
                ys = native.limbs_to_ints(np.ascontiguousarray(ev[0][i]))
                assert got[0][i] == trapdoor_proof(curve, cv, p_tau, ys, h, zeta, l), (l, log_N, i)
                xy, inf, cev = ctx.open_coset(ck.srs, arr, [n], n, l.bit_length() - 1, h, zeta, 1)
                assert got[0][i] == one_point(native, ctx.fp_limbs, xy, inf), (l, log_N, i)
                assert native.limbs_to_ints(cev) == ys
        table.close()


def test_2_16_cross_identity_over_open_domain(kzgs, native):
    """pi_i = sum_k (x_k / (l a_i)) pi(x_k) over open_domain's single-point proofs, at 8 random cosets"""
    curve = "bls12_381"
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(16)
    log_n, l = 16, 16
    n = 1 << log_n
    ctx = kzg._context()
    ck = mono_key(kzg, n)
    w = cv.root_of_unity(n)
    p = [rng.randrange(r) for _ in range(n)]
    single, _ = run_domain(native, ctx, ctx.domain_table(ck.srs, log_n), p, w)
    got, _ = run(native, ctx, ctx.coset_table(ck.srs, log_n, 4), [p], log_n, w, evals=False)
    C = n // l
    L = ctx.fp_limbs
    for i in rng.sample(range(C), 8):
        a = pow(w, i * l, r)
        terms = []
        for k in range(l):
            t = i + k * C
            s = pow(w, t, r) * pow(l * a, -1, r) % r
            pt = single[t]
            if pt is None:
                continue
            xy, inf = c_oracle.g1_mul(curve, native.ints_to_limbs(list(pt), L).reshape(-1), s)
            if not inf:
                terms.append((*_ints(xy), 1))
        want = kzg._sum_g1(terms)
        assert got[0][i] == (None if want[2] == 0 else (want[0], want[1])), i


def run_domain(native, ctx, table, p, w):
    n = table.n
    xy, inf, ev = ctx.open_domain(table, pack(native, [p], n), [len(p)], n, w, evals=False)
    return points(native, ctx.fp_limbs, xy, inf)[0], ev


# ---- 5. batches across chunk boundaries ---------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_batches_across_chunks(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(5)
    log_n, log_l = 6, 2
    n, l = 1 << log_n, 1 << log_l
    ctx = kzg._context()
    table = ctx.coset_table(mono_key(kzg, n).srs, log_n, log_l)
    lens = [n, 0, 3, 1, 40, n, 2, 17]
    polys = [[rng.randrange(r) for _ in range(m)] for m in lens]
    log_N = log_n + 2
    w = cv.root_of_unity(1 << log_N)
    whole, ev = run(native, ctx, table, polys, log_N, w)
    try:
        for chunk in (1, 3):
            ctx.set_tuning("open_cosets_chunk", chunk)
            got, ev2 = run(native, ctx, table, polys, log_N, w)
            assert got == whole and np.array_equal(ev, ev2), chunk
    finally:
        ctx.set_tuning("open_cosets_chunk", 0)
    C = (1 << log_N) // l
    for j, p in enumerate(polys):
        for i in (0, 5, C - 1):
            assert whole[j][i] == oracle_proof(curve, cv, p, l, pow(w, i, r)), (j, i)


# ---- 6. kzg_open_coset --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_open_coset_small_against_the_oracle(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(6)
    n = 40
    ctx = kzg._context()
    ck = mono_key(kzg, 64)
    w = cv.root_of_unity(64)
    for l in (1, 2, 4, 8):
        zeta = cv.root_of_unity(l) if l > 1 else 1
        for k in (1, 3):
            polys = [[rng.randrange(r) for _ in range(m)] for m in [n, 5, 1][:k]]
            xi = rng.randrange(r)
            arr = pack(native, polys, n)
            comb = O.combine(polys, xi, r)
            for h in (rng.randrange(1, r), pow(w, rng.randrange(64), r)):
                xy, inf, ev = ctx.open_coset(ck.srs, arr, [len(p) for p in polys], n, l.bit_length() - 1, h, zeta, xi)
                assert one_point(native, ctx.fp_limbs, xy, inf) == oracle_proof(curve, cv, comb, l, h), (l, k)
                assert native.limbs_to_ints(ev) == [O.poly_eval(comb, h * pow(zeta, q, r) % r, r) for q in range(l)]
                if l == 1:                                                # kzg_open at z = h
                    oxy, oinf, oev = ctx.open(ck.srs, arr, [len(p) for p in polys], n, native.int_to_words(h),
                                              native.int_to_words(xi))
                    assert np.array_equal(oxy[0] if oxy.ndim > 1 else oxy, xy) and oinf[0] == inf[0]


def test_open_coset_2_20_and_tau_on_the_coset(kzgs, native):
    curve = "bls12_381"
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(61)
    n = 1 << 20
    ctx = kzg._context()
    ck = mono_key(kzg, n)
    p = [rng.randrange(r) for _ in range(n)]
    arr = pack(native, [p], n)
    p_tau = O.poly_eval(p, TAU, r)
    for l in (16, 64, 4096):
        zeta = cv.root_of_unity(l)
        h = rng.randrange(1, r)
        xy, inf, ev = ctx.open_coset(ck.srs, arr, [n], n, l.bit_length() - 1, h, zeta, 1)
        ys = native.limbs_to_ints(ev)
        assert ys[0] == O.poly_eval(p, h, r) and ys[-1] == O.poly_eval(p, h * pow(zeta, l - 1, r) % r, r)
        assert one_point(native, ctx.fp_limbs, xy, inf) == trapdoor_proof(curve, cv, p_tau, ys, h, zeta, l), l
    # tau itself on the coset: the trapdoor form divides by zero, the coefficients' quotient does not
    small = 64
    tau_key = mono_key(kzg, small, tau=pow(cv.root_of_unity(8), 3, r) * 5 % r)
    l, zeta = 8, cv.root_of_unity(8)
    q = [rng.randrange(r) for _ in range(small)]
    xy, inf, _ = ctx.open_coset(tau_key.srs, pack(native, [q], small), [small], small, 3, 5, zeta, 1)
    assert one_point(native, ctx.fp_limbs, xy, inf) == oracle_proof(curve, cv, q, l, 5,
                                                                     tau=pow(cv.root_of_unity(8), 3, r) * 5 % r)


# ---- 7. facade round trip -----------------------------------------------------------------------------------------
def test_facade_round_trip_and_tampering(kzgs):
    curve = "bn254"
    kzg = kzgs[curve]
    r = kzg.curve_order
    rng = random.Random(7)
    n, l = 32, 4
    ck, _ = kzg.setup(n - 1, tau=TAU)
    rk = kzg.coset_verification_key(l, TAU)
    polys = [[rng.randrange(r) for _ in range(n)], [rng.randrange(r) for _ in range(9)]]
    comms = kzg.commit(ck, polys)
    proofs, values = kzg.open_cosets_each(ck, polys, l, N=2 * n, with_values=True)
    w = int(kzg.Fq.root_of_unity(2 * n))
    C = 2 * n // l
    zeta = pow(w, C, r)
    assert zeta == int(kzg.Fq.root_of_unity(l))
    i = 5
    assert kzg.check_coset(ck, rk, comms[:1], pow(w, i, r), values[0][i:i + 1], proofs[0][i], 1)
    xi = rng.randrange(r)
    pf = kzg.open_cosets(ck, polys, xi, l, N=2 * n)
    both = [values[0][i], values[1][i]]
    assert kzg.check_coset(ck, rk, comms, pow(w, i, r), both, pf[i], xi)
    assert pf[i] == kzg.open_coset(ck, polys, pow(w, i, r), l, xi)
    bad = [both[0][:], both[1][:]]
    bad[1][3] = (bad[1][3] + 1) % r
    assert not kzg.check_coset(ck, rk, comms, pow(w, i, r), bad, pf[i], xi)
    i2 = 11
    args = [[comms[:1], comms[:1]], [pow(w, i, r), pow(w, i2, r)], [values[0][i:i + 1], values[0][i2:i2 + 1]],
            [proofs[0][i], proofs[0][i2]], [1, 1]]
    assert kzg.batch_check_cosets(ck, rk, *args, r=99)
    args[2] = [values[0][i:i + 1], [[(values[0][i2][0] + 1) % r] + values[0][i2][1:]]]
    assert not kzg.batch_check_cosets(ck, rk, *args, r=99)


# ---- 8. robustness ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_loaded_key_errors_pipeline_and_spans(kzgs, native, curve, tmp_path):
    import torch
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(8)
    n, log_n, log_l = 256, 8, 3
    ctx = kzg._context()
    ck = mono_key(kzg, n)
    w = cv.root_of_unity(n)
    p = [rng.randrange(r) for _ in range(n)]
    table = ctx.coset_table(ck.srs, log_n, log_l)
    good, _ = run(native, ctx, table, [p], log_n, w)
    path = str(tmp_path / "key.srs")
    kzg.save_key(ck, path)
    loaded = kzg.load_key(path)
    got, _ = run(native, ctx, ctx.coset_table(loaded.srs, log_n, log_l), [p], log_n, w)
    assert got == good

    def code(fn, *a, **k):
        with pytest.raises(native.NativeError) as e:
            fn(*a, **k)
        return e.value.code

    arr = pack(native, [p], n)
    zeta = cv.root_of_unity(8)
    lk, _ = kzg.setup_lagrange(n, tau=TAU)
    assert code(ctx.coset_table, lk.srs, log_n, log_l) == -1                        # not a monomial key
    assert code(ctx.coset_table, ck.srs, log_n, log_n) == -1                        # l > n/2
    assert code(ctx.coset_table, ck.srs, 9, 1) == -1                                # key shorter than n
    assert code(ctx.open_cosets, table, arr, [n], n, log_n + 3, cv.root_of_unity(n << 3)) == -1   # N > 4n
    assert code(ctx.open_cosets, table, arr, [n], n, log_n, w * w % r) == -1       # not primitive
    assert code(ctx.open_cosets, table, arr, [n], n - 1, log_n, w) == -1           # lens > stride
    assert code(ctx.open_cosets, table, pack(native, [p + [1]], n + 1), [n + 1], n + 1, log_n, w) == \
        native.KZG_ERR_DEGREE
    assert code(ctx.open_domain, table, arr, [n], n, w) == -1                       # a coset table
    assert code(ctx.open_coset, lk.srs, arr, [n], n, 3, 7, zeta, 1) == -1          # Lagrange key
    assert code(ctx.open_coset, ck.srs, arr, [n], n, 3, 0, zeta, 1) == -1          # h = 0
    assert code(ctx.open_coset, ck.srs, arr, [n], n, 3, 7, zeta * zeta % r, 1) == -1   # not primitive
    assert code(ctx.open_coset, ck.srs, arr, [n], n, 13, 7, 1, 1) == -1            # log_l > 12
    assert code(ctx.open_coset, mono_key(kzg, 16).srs, arr, [n], n, 3, 7, zeta, 1) == native.KZG_ERR_DEGREE
    again, _ = run(native, ctx, table, [p], log_n, w)
    assert again == good
    # a pending async commit survives both new calls
    want_xy, want_inf = ctx.commit(ck.srs, arr, [n], n)
    d = torch.from_numpy(arr.reshape(n, 4).view(np.int64)).cuda()
    torch.cuda.synchronize()
    out_xy = np.zeros(2 * ctx.fp_limbs, dtype=np.uint64)
    out_inf = np.zeros(1, dtype=np.uint8)
    ctx.commit_device_async(ck.srs, d.data_ptr(), [n], n, out_xy, out_inf)
    run(native, ctx, table, [p], log_n, w)
    ctx.open_coset(ck.srs, arr, [n], n, 3, 7, zeta, 1)
    ctx.commit_flush()
    assert np.array_equal(out_xy, want_xy[0]) and out_inf[0] == want_inf[0]
    # one span per table and per call
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        t2 = ctx.coset_table(ck.srs, log_n, 2)
        for _ in range(3):
            run(native, ctx, t2, [p, [5]], log_n, w)
        for _ in range(2):
            ctx.open_coset(ck.srs, arr, [n], n, 2, 7, cv.root_of_unity(4), 1)
        assert ctx.prof_read("coset_table")[1] == 1
        assert ctx.prof_read("open_cosets")[1] == 3
        assert ctx.prof_read("open_coset_poly")[1] == 2
        t2.close()
    finally:
        ctx.prof_enable(False)

"""GPU parity of FK20 openings (csrc/domain.hip through the C ABI and the facade): every proof on the domain equals the
opening at that point -- the oracle's, the trapdoor form's and kzg_open's -- compared on canonical affine coordinates
and infinity flags, bit for bit."""
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
    """[b][n] device output -> nested lists of (x, y) / None"""
    b, n = inf.shape
    ints = native.limbs_to_ints(np.ascontiguousarray(xy).reshape(-1, L))
    return [[None if inf[j, i] else (ints[2 * (j * n + i)], ints[2 * (j * n + i) + 1]) for i in range(n)]
            for j in range(b)]


def trapdoor_proofs(curve, cv, coeffs, n, w, tau, ys=None):
    """[(p(tau) - p(w^i)) / (tau - w^i)] G1 for every i (tau outside the domain), through c_oracle.g1_mul; ys: the
    values p(w^i) when already known"""
    r = cv.r
    g = _xy_limbs(curve, cv.g1)
    pt = O.poly_eval(coeffs, tau, r)
    out = []
    for i in range(n):
        z = pow(w, i, r)
        y = O.poly_eval(coeffs, z, r) if ys is None else ys[i]
        k = (pt - y) * pow(tau - z, -1, r) % r
        xy, inf = c_oracle.g1_mul(curve, g, k)
        out.append(None if inf else tuple(_ints(xy)))
    return out


def _xy_limbs(curve, xy):
    from kzg_snark_amd import _native
    L = _native.lib().kzg_fp_limbs(_native.CURVE_IDS[curve])
    return _native.ints_to_limbs(list(xy), L).reshape(-1)


def _ints(xy):
    from kzg_snark_amd import _native
    L = len(xy) // 2
    return _native.limbs_to_ints(np.asarray(xy).reshape(2, L))


def edge_inputs(n, r, rng):
    return [[rng.randrange(r) for _ in range(n)], [r - 1] * n, [rng.randrange(r) for _ in range(max(1, n // 2))],
            [rng.randrange(r)], []]


def run(native, kzg, table, polys, n, w, evals=True):
    ctx = kzg._context()
    stride = max(max((len(p) for p in polys), default=1), 1)
    xy, inf, ev = ctx.open_domain(table, pack(native, polys, stride), [len(p) for p in polys], stride, w,
                                  evals=evals)
    return points(native, ctx.fp_limbs, xy, inf), ev


# ---- 1. exact against the oracle, log_n 1..8 -------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_every_proof_equals_the_oracle_opening(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(11)
    ctx = kzg._context()
    for log_n in range(1, 9):
        n = 1 << log_n
        ck = mono_key(kzg, n)
        table = ctx.domain_table(ck.srs, log_n)
        w = cv.root_of_unity(n)
        polys = edge_inputs(n, cv.r, rng)
        got, _ = run(native, kzg, table, polys, n, w, evals=False)
        for j, p in enumerate(polys):
            want = trapdoor_proofs(curve, cv, p, n, w, TAU)
            assert got[j] == want, (log_n, j)
            if log_n <= 2:                                            # the oracle's own opening, too
                ref_ck = O.setup(n - 1, TAU, cv)
                for i in range(n):
                    assert got[j][i] == O.normalize(O.open_(ref_ck, [p], pow(w, i, cv.r), 1, cv)[0], cv)
            if len(p) <= 1:
                assert all(q is None for q in got[j])


# ---- 2. trapdoor at 2^12, values against kzg_ntt ------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_trapdoor_and_values_at_2_12(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(12)
    n, log_n = 1 << 12, 12
    ctx = kzg._context()
    table = ctx.domain_table(mono_key(kzg, n).srs, log_n)
    w = cv.root_of_unity(n)
    p = [rng.randrange(cv.r) for _ in range(n)]
    got, ev = run(native, kzg, table, [p], n, w)
    data = native.ints_to_limbs(p).copy()
    ctx.ntt(data, log_n, native.int_to_words(w), False)
    assert np.array_equal(ev[0], data)
    ys = native.limbs_to_ints(ev[0])
    assert ys[1] == O.poly_eval(p, w, cv.r)
    assert got[0] == trapdoor_proofs(curve, cv, p, n, w, TAU, ys)


# ---- 3. 2^20 on BLS12-381 -------------------------------------------------------------------------------------------
def test_2_20_bls_matches_kzg_open_and_one_random_combination(kzgs, native):
    curve = "bls12_381"
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    rng = random.Random(20)
    log_n = 20
    n = 1 << log_n
    ctx = kzg._context()
    L = ctx.fp_limbs
    ck = kzg.setup(n - 1, tau=TAU)[0]
    table = ctx.domain_table(ck.srs, log_n)
    w = cv.root_of_unity(n)
    coeffs = native.ints_to_limbs([rng.randrange(r) for _ in range(n)]).copy()
    xy, inf, ev = ctx.open_domain(table, coeffs.reshape(1, n, 4), [n], n, w)
    assert not inf.any()
    idx = sorted({0, 1, n // 2, n - 1} | {rng.randrange(n) for _ in range(60)})
    for i in idx:
        z = pow(w, i, r)
        pxy, pinf, pev = ctx.open(ck.srs, coeffs.reshape(1, n, 4), [n], n, native.int_to_words(z),
                                  native.int_to_words(1))
        assert np.array_equal(xy[0, i], pxy) and inf[0, i] == pinf[0], i
        assert np.array_equal(ev[0, i], pev), i
    # sum_i r_i (tau - w^i) pi_i = (sum r_i) C - (sum r_i y_i) G
    proofs = ctx.srs_load_g1(np.ascontiguousarray(xy[0]), inf[0].copy())
    ys = native.limbs_to_ints(ev[0])
    rs = [rng.randrange(1, r) for _ in range(n)]
    sc, z = [], 1
    for i in range(n):
        sc.append(rs[i] * (TAU - z) % r)
        z = z * w % r
    lxy, linf = ctx.commit(proofs, native.ints_to_limbs(sc).reshape(1, n, 4), [n], n)
    cxy, cinf = ctx.commit(ck.srs, coeffs.reshape(1, n, 4), [n], n)
    s_r = sum(rs) % r
    s_ry = sum(a * b for a, b in zip(rs, ys)) % r
    g = _xy_limbs(curve, cv.g1)
    a_xy, a_inf = c_oracle.g1_mul(curve, cxy[0], s_r)
    b_xy, b_inf = c_oracle.g1_mul(curve, g, (-s_ry) % r)
    rhs = O.add(O.Z1() if a_inf else O.from_affine(_ints(a_xy)), O.Z1() if b_inf else O.from_affine(_ints(b_xy)), cv)
    assert not linf[0]
    assert tuple(_ints(lxy[0])) == O.normalize(rhs, cv)
    proofs.close()


# ---- 4. batches and chunks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_batch_with_mixed_lengths_across_chunks(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(4)
    n, log_n = 64, 6
    ctx = kzg._context()
    table = ctx.domain_table(mono_key(kzg, n).srs, log_n)
    w = cv.root_of_unity(n)
    polys = [[rng.randrange(cv.r) for _ in range(m)] for m in (64, 1, 0, 33, 17)]
    singles = [run(native, kzg, table, [p], n, w) for p in polys]
    ctx.set_tuning("open_domain_chunk", 2)
    try:
        got, ev = run(native, kzg, table, polys, n, w)
    finally:
        ctx.set_tuning("open_domain_chunk", 0)
    for j in range(len(polys)):
        assert got[j] == singles[j][0][0], j
        assert np.array_equal(ev[j], singles[j][1][0]), j


# ---- 5. facade ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_facade_open_domain_equals_open_at_every_point(kzgs, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(5)
    n = 64
    ck = mono_key(kzg, n)
    polys = [[rng.randrange(cv.r) for _ in range(m)] for m in (64, 40, 3)]
    xi = rng.randrange(cv.r)
    w = int(kzg.Fq.root_of_unity(n))
    got = kzg.open_domain(ck, polys, xi)
    assert len(got) == n
    each = kzg.open_domain_each(ck, polys)
    table = kzg.domain_table(ck, n)
    assert kzg.domain_table(ck, n) is table                              # cached per (key, n)
    assert kzg.open_domain(table, polys, xi) == got
    for i in range(n):
        z = pow(w, i, cv.r)
        assert got[i] == kzg.open(ck, polys, z, xi), i
        for j, p in enumerate(polys):
            assert each[j][i] == kzg.open(ck, [p], z, 1), (i, j)


# ---- 6. another root ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_another_primitive_root_permutes_the_proofs(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(6)
    n, log_n = 128, 7
    ctx = kzg._context()
    table = ctx.domain_table(mono_key(kzg, n).srs, log_n)
    w = cv.root_of_unity(n)
    p = [rng.randrange(cv.r) for _ in range(n)]
    a, _ = run(native, kzg, table, [p], n, w, evals=False)
    b, _ = run(native, kzg, table, [p], n, pow(w, 3, cv.r), evals=False)
    assert all(b[0][i] == a[0][3 * i % n] for i in range(n))


# ---- 7. tau in the domain; a loaded key ------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_tau_in_the_domain_and_a_loaded_key(kzgs, native, curve, tmp_path):
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(7)
    n, log_n = 32, 5
    ctx = kzg._context()
    w = cv.root_of_unity(n)
    ck = mono_key(kzg, n, tau=pow(w, 5, cv.r))
    table = ctx.domain_table(ck.srs, log_n)
    p = [rng.randrange(cv.r) for _ in range(n)]
    got, _ = run(native, kzg, table, [p], n, w, evals=False)
    arr = pack(native, [p], n)
    for i in range(n):
        pxy, pinf, _ = ctx.open(ck.srs, arr, [n], n, native.int_to_words(pow(w, i, cv.r)), native.int_to_words(1))
        want = None if pinf[0] else tuple(_ints(pxy))
        assert got[0][i] == want, i
    path = str(tmp_path / "key.srs")
    kzg.save_key(ck, path)
    loaded = kzg.load_key(path)
    got2, _ = run(native, kzg, ctx.domain_table(loaded.srs, log_n), [p], n, w, evals=False)
    assert got2 == got


# ---- 8. errors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_errors_leave_the_context_usable(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    r = cv.r
    n, log_n = 16, 4
    ctx = kzg._context()
    ck = mono_key(kzg, n)
    table = ctx.domain_table(ck.srs, log_n)
    w = cv.root_of_unity(n)
    p = list(range(1, n + 1))
    good, _ = run(native, kzg, table, [p], n, w)

    def code(fn, *a, **k):
        with pytest.raises(native.NativeError) as e:
            fn(*a, **k)
        return e.value.code

    lk, _ = kzg.setup_lagrange(n, tau=TAU)
    assert code(ctx.domain_table, lk.srs, log_n) == -1                           # not a monomial key
    assert code(ctx.domain_table, ck.srs, 5) == -1                               # key shorter than n
    assert code(ctx.domain_table, ck.srs, 0) == -1
    assert code(ctx.domain_table, ck.srs, 21) == -1
    other = kzgs["bn254" if curve == "bls12_381" else "bls12_381"]
    assert code(ctx.domain_table, mono_key(other, n).srs, log_n) == -1           # another curve
    arr = pack(native, [p + [1]], n + 1)
    assert code(ctx.open_domain, table, arr, [n + 1], n + 1, w) == native.KZG_ERR_DEGREE
    assert code(ctx.open_domain, table, pack(native, [p], n), [n], n - 1, w) == -1     # lens > stride
    assert code(ctx.open_domain, table, pack(native, [p], n), [n], n, w * w % r) == -1  # not primitive
    assert code(ctx.open_domain, table, pack(native, [p], n), [n], n, 1) == -1
    again, _ = run(native, kzg, table, [p], n, w)
    assert again == good


# ---- 9. the commit pipeline is left alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_pending_async_commit_survives_open_domain(kzgs, native, curve):
    import torch
    kzg, cv = kzgs[curve], O.curve(curve)
    rng = random.Random(9)
    n, log_n = 256, 8
    ctx = kzg._context()
    ck = mono_key(kzg, n)
    table = ctx.domain_table(ck.srs, log_n)
    c = [rng.randrange(cv.r) for _ in range(n)]
    arr = pack(native, [c], n)
    want_xy, want_inf = ctx.commit(ck.srs, arr, [n], n)
    d = torch.from_numpy(arr.reshape(n, 4).view(np.int64)).cuda()
    torch.cuda.synchronize()
    out_xy = np.zeros(2 * ctx.fp_limbs, dtype=np.uint64)
    out_inf = np.zeros(1, dtype=np.uint8)
    ctx.commit_device_async(ck.srs, d.data_ptr(), [n], n, out_xy, out_inf)
    run(native, kzg, table, [c], n, cv.root_of_unity(n))
    ctx.commit_flush()
    assert np.array_equal(out_xy, want_xy[0]) and out_inf[0] == want_inf[0]


# ---- 10. profiler spans ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_one_span_per_table_and_per_call(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    n, log_n = 16, 4
    ctx = kzg._context()
    ck = mono_key(kzg, n)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        t1 = ctx.domain_table(ck.srs, log_n)
        t2 = ctx.domain_table(ck.srs, log_n - 1)
        for _ in range(3):
            run(native, kzg, t1, [list(range(1, 17)), [5]], n, cv.root_of_unity(n))
        assert ctx.prof_read("domain_table")[1] == 2
        assert ctx.prof_read("open_domain")[1] == 3
        t2.close()
    finally:
        ctx.prof_enable(False)

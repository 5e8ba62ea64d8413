"""GPU tests of bulk verification (csrc/verify.hip through the C ABI and the facade): the two folded points equal the
plain-Python restatement (tests/verify_restated.py) coordinate for coordinate at small sizes; whole outputs of
kzg_open_cosets / kzg_open_domain up to 2^20 proofs satisfy L == tau^l R (one host scalar multiplication through the
trapdoor) and stop doing so after a single change; every argument error is refused and leaves the context usable; the
commit pipeline's pending results survive the call; the facade agrees with the host verifier on real pairings."""
import random

import numpy as np
import pytest

from oracle import c_oracle
from oracle import py_oracle as O
from verify_restated import restated_LR

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
KZG_ERR_ARG = -1


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
        if len(p):
            arr[j, :len(p)] = native.ints_to_limbs([int(c) for c in p])
    return arr


def to_point(native, L, xy, inf):
    """C layout -> oracle point"""
    if inf:
        return O.Z1()
    v = native.limbs_to_ints(np.ascontiguousarray(xy).reshape(2, L))
    return (v[0], v[1], 1)


def same_point(native, L, xy, inf, want, cv):
    """the library's affine point equals the oracle point `want`, coordinate for coordinate"""
    aff = O.normalize(want, cv)
    if aff is None:
        return bool(inf) and not np.asarray(xy).any()
    v = native.limbs_to_ints(np.ascontiguousarray(xy).reshape(2, L))
    return not inf and (v[0], v[1]) == aff


def trapdoor_holds(curve, cv, xy, inf, l, tau=TAU):
    """L == tau^l R with one scalar multiplication on the host (the C oracle)"""
    want_xy, want_inf = c_oracle.g1_mul(curve, np.ascontiguousarray(xy[1]), pow(tau, l, cv.r), inf=bool(inf[1]))
    if want_inf or inf[0]:
        return bool(want_inf) and bool(inf[0])
    return bool((np.asarray(xy[0]) == want_xy).all())


def random_polys(native, rng_seed, b, n, r):
    """b coefficient vectors of n reduced elements: uint64[b, n, 4]"""
    rng = np.random.default_rng(rng_seed)
    raw = rng.integers(0, 1 << 63, size=(b, n, 4), dtype=np.uint64)
    raw[..., 3] %= np.uint64(r >> 192)                     # top limb below the modulus' top limb: reduced
    return raw


# ---- 1. exact points at small sizes -----------------------------------------------------------------------------------
def _small_claims(native, ctx, kzg, cv, n, l, N, K, rng):
    """three commitments (random, the constant r - 1 -- shorter than l for l > 1, all values r - 1 --, zero) and K
    cells with repetition in random order, proofs and values from kzg_open_coset"""
    r, L = cv.r, ctx.fp_limbs
    ck = mono_key(kzg, n)
    w = cv.root_of_unity(N)
    zeta = pow(w, N // l, r)
    polys = [[rng.randrange(r) for _ in range(n - 1)] + [r - 1], [r - 1], []]
    cxy, cinf = ctx.commit(ck.srs, pack(native, polys, n), [len(p) for p in polys], n)
    comm_idx = [rng.randrange(3) for _ in range(K)]
    coset_idx = [rng.randrange(N // l) for _ in range(K)]
    pxy = np.zeros((K, 2 * L), dtype=np.uint64)
    pinf = np.zeros(K, dtype=np.uint8)
    vals = np.zeros((K, l, 4), dtype=np.uint64)
    log_l = l.bit_length() - 1
    for k, (c, i) in enumerate(zip(comm_idx, coset_idx)):
        p = polys[c]
        xy, inf, ev = ctx.open_coset(ck.srs, pack(native, [p], max(len(p), 1)), [len(p)], max(len(p), 1), log_l,
                                     pow(w, i, r), zeta, 1)
        pxy[k], pinf[k], vals[k] = xy, inf[0], ev
    return ck, w, polys, cxy, cinf, comm_idx, coset_idx, vals, pxy, pinf


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [16, 64])
def test_points_equal_the_restatement_coordinate_for_coordinate(kzgs, native, curve, n):
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    r, L = cv.r, ctx.fp_limbs
    rng = random.Random(n + len(curve))
    for l in (1, 4, 16):
        for N in (n, 2 * n):
            log_N, log_l = N.bit_length() - 1, l.bit_length() - 1
            if l >= N:
                # kzg_verify_cosets needs l < N (a coset is a proper subset of the domain): refused as documented
                w = cv.root_of_unity(2 * N)
                ck = mono_key(kzg, n)
                z = np.zeros((1, 2 * L), dtype=np.uint64)
                with pytest.raises(native.NativeError) as e:
                    ctx.verify_cosets(ck.srs, log_N, log_l, w, z, np.ones(1, np.uint8), [0], [0],
                                      np.zeros((1, l, 4), np.uint64), z, np.ones(1, np.uint8), 5)
                assert e.value.code == KZG_ERR_ARG
                continue
            runs = [(9, rng.randrange(1, r))]
            if n == 16:
                runs += [(1, rng.randrange(1, r)), (5, 1)]             # K = 1; rho = 1
            for K, rho in runs:
                ck, w, polys, cxy, cinf, comm_idx, coset_idx, vals, pxy, pinf = _small_claims(
                    native, ctx, kzg, cv, n, l, N, K, rng)
                assert all(pinf[k] for k, c in enumerate(comm_idx) if c != 0)      # short and zero polynomials: O
                if 1 in comm_idx:                                                   # values r - 1
                    k1 = comm_idx.index(1)
                    assert native.limbs_to_ints(vals[k1]) == [r - 1] * l
                xy, inf = ctx.verify_cosets(ck.srs, log_N, log_l, w, cxy, cinf, comm_idx, coset_idx, vals, pxy, pinf,
                                            rho)
                ck_pts = [ck[j] for j in range(l)]
                comms = [to_point(native, L, cxy[j], cinf[j]) for j in range(3)]
                proofs = [to_point(native, L, pxy[k], pinf[k]) for k in range(K)]
                values = [native.limbs_to_ints(vals[k]) for k in range(K)]
                wantL, wantR = restated_LR(ck_pts, comms, comm_idx, coset_idx, values, proofs, l, N, w, rho, cv)
                assert same_point(native, L, xy[0], inf[0], wantL, cv), (l, N, K, "L")
                assert same_point(native, L, xy[1], inf[1], wantR, cv), (l, N, K, "R")
                assert trapdoor_holds(curve, cv, xy, inf, l), (l, N, K)


# ---- 2. whole outputs at size, through the trapdoor ---------------------------------------------------------------
def _open_cosets_claims(native, ctx, kzg, cv, log_n, log_N, log_l, b, seed):
    """the complete output of kzg_open_cosets (with the values) for b random polynomials, laid out as claims"""
    n, N, l = 1 << log_n, 1 << log_N, 1 << log_l
    ck = mono_key(kzg, n)
    w = cv.root_of_unity(N)
    table = ctx.coset_table(ck.srs, log_n, log_l)
    polys = random_polys(native, seed, b, n, cv.r)
    cxy, cinf = ctx.commit(ck.srs, polys, [n] * b, n)
    pxy, pinf, ev = ctx.open_cosets(table, polys, [n] * b, n, log_N, w, evals=True)
    table.close()
    C = N // l
    comm_idx = np.repeat(np.arange(b, dtype=np.uint32), C)
    coset_idx = np.tile(np.arange(C, dtype=np.uint32), b)
    return (ck, w, cxy, cinf, comm_idx, coset_idx, ev.reshape(b * C, l, 4), pxy.reshape(b * C, -1),
            pinf.reshape(b * C))


@pytest.mark.parametrize("curve", CURVES)
def test_whole_peerdas_output_verifies(kzgs, native, curve):
    """n = 2^12, N = 2^13, l = 64, 32 blobs: 4096 cells"""
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    ck, w, cxy, cinf, ci, ki, vals, pxy, pinf = _open_cosets_claims(native, ctx, kzg, cv, 12, 13, 6, 32, 1)
    xy, inf = ctx.verify_cosets(ck.srs, 13, 6, w, cxy, cinf, ci, ki, vals, pxy, pinf, 0x1234567 ** 7 % cv.r)
    assert not inf[1]
    assert trapdoor_holds(curve, cv, xy, inf, 64)


@pytest.mark.parametrize("curve", CURVES)
def test_whole_2_16_output_verifies_and_single_changes_are_caught(kzgs, native, curve):
    """n = N = 2^16, l = 64, two polynomials: 2048 cells; then one limb of one value, two proofs swapped, one coset
    index, one commitment index"""
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    ck, w, cxy, cinf, ci, ki, vals, pxy, pinf = _open_cosets_claims(native, ctx, kzg, cv, 16, 16, 6, 2, 2)
    rho = 0xabcdef ** 9 % cv.r

    def holds(ci=ci, ki=ki, vals=vals, pxy=pxy, pinf=pinf):
        xy, inf = ctx.verify_cosets(ck.srs, 16, 6, w, cxy, cinf, ci, ki, vals, pxy, pinf, rho)
        return trapdoor_holds(curve, cv, xy, inf, 64)

    assert holds()
    bad = vals.copy()
    bad[777, 13, 2] ^= np.uint64(1 << 20)                                  # one limb of one value (still reduced)
    assert not holds(vals=bad)
    bad = pxy.copy()
    bad[[5, 1500]] = bad[[1500, 5]]                                        # two distinct proofs swapped
    assert (pxy[5] != pxy[1500]).any()
    assert not holds(pxy=bad)
    bad = ki.copy()
    bad[100] = (bad[100] + 1) % 1024                                       # one coset index
    assert not holds(ki=bad)
    bad = ci.copy()
    bad[2047] = 0                                                          # a cell of polynomial 1 claimed for 0
    assert not holds(ci=bad)


def test_whole_2_20_coset_output_verifies(kzgs, native):
    """BLS12-381, n = 2^20, N = 2^21, l = 16: 2^17 cells, 2^21 values"""
    kzg, cv = kzgs["bls12_381"], O.curve("bls12_381")
    ctx = kzg._context()
    ck, w, cxy, cinf, ci, ki, vals, pxy, pinf = _open_cosets_claims(native, ctx, kzg, cv, 20, 21, 4, 1, 3)
    xy, inf = ctx.verify_cosets(ck.srs, 21, 4, w, cxy, cinf, ci, ki, vals, pxy, pinf, 0x31415926 ** 8 % cv.r)
    assert not inf[1]
    assert trapdoor_holds("bls12_381", cv, xy, inf, 16)


@pytest.mark.parametrize("log_n", [16, 20])
def test_whole_open_domain_output_verifies(kzgs, native, log_n):
    """BLS12-381, every proof of kzg_open_domain: l = 1, K = n (2^16: 16-bit windows, 2^20: 20-bit windows)"""
    kzg, cv = kzgs["bls12_381"], O.curve("bls12_381")
    ctx = kzg._context()
    n = 1 << log_n
    ck = mono_key(kzg, n)
    w = cv.root_of_unity(n)
    table = ctx.domain_table(ck.srs, log_n)
    polys = random_polys(native, 4 + log_n, 1, n, cv.r)
    cxy, cinf = ctx.commit(ck.srs, polys, [n], n)
    pxy, pinf, ev = ctx.open_domain(table, polys, [n], n, w, evals=True)
    table.close()
    args = (cxy, cinf, np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), ev.reshape(n, 1, 4), pxy.reshape(n, -1),
            pinf.reshape(n))
    xy, inf = ctx.verify_cosets(ck.srs, log_n, 0, w, *args, 0x27182818 ** 8 % cv.r)
    assert not inf[1]
    assert trapdoor_holds("bls12_381", cv, xy, inf, 1)
    if log_n == 16:                                                        # and a changed value is caught at l = 1
        bad = ev.reshape(n, 1, 4).copy()
        bad[n // 3, 0, 0] ^= np.uint64(1)
        xy, inf = ctx.verify_cosets(ck.srs, log_n, 0, w, cxy, cinf, args[2], args[3], bad, args[5], args[6], 12345)
        assert not trapdoor_holds("bls12_381", cv, xy, inf, 1)


@pytest.mark.parametrize("log_l", [8, 10, 12])
def test_large_cosets_verify(kzgs, native, log_l):
    """l = 256, 1024, 4096 (tiles of more than one element per thread; 128 KiB of LDS at 4096) on N = 2^13, cells from
    kzg_open_coset of a random and a short polynomial"""
    curve = "bls12_381"
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    r, L = cv.r, ctx.fp_limbs
    n = N = 1 << 13
    l = 1 << log_l
    ck = mono_key(kzg, n)
    w = cv.root_of_unity(N)
    zeta = pow(w, N // l, r)
    polys = [random_polys(native, log_l, 1, n, r)[0], random_polys(native, log_l + 1, 1, 100, r)[0]]
    cxy, cinf = ctx.commit(ck.srs, pack_arrays(polys, n), [n, 100], n)
    ci, ki = [0, 1, 0], [1, 0, N // l - 1]
    pxy, pinf = np.zeros((3, 2 * L), dtype=np.uint64), np.zeros(3, dtype=np.uint8)
    vals = np.zeros((3, l, 4), dtype=np.uint64)
    for k, (c, i) in enumerate(zip(ci, ki)):
        p = polys[c]
        xy, inf, ev = ctx.open_coset(ck.srs, np.ascontiguousarray(p).reshape(1, -1, 4), [len(p)], len(p), log_l,
                                     pow(w, i, r), zeta, 1)
        pxy[k], pinf[k], vals[k] = xy, inf[0], ev
    assert pinf[1] and not pinf[0]
    xy, inf = ctx.verify_cosets(ck.srs, 13, log_l, w, cxy, cinf, ci, ki, vals, pxy, pinf, 0x5eed ** 15 % r)
    assert not inf[0] and not inf[1]
    assert trapdoor_holds(curve, cv, xy, inf, l)
    vals[2, l - 1, 0] ^= np.uint64(1)
    xy, inf = ctx.verify_cosets(ck.srs, 13, log_l, w, cxy, cinf, ci, ki, vals, pxy, pinf, 0x5eed ** 15 % r)
    assert not trapdoor_holds(curve, cv, xy, inf, l)


def pack_arrays(polys, stride):
    arr = np.zeros((len(polys), stride, 4), dtype=np.uint64)
    for j, p in enumerate(polys):
        arr[j, :len(p)] = p
    return arr


# ---- 3. argument errors ------------------------------------------------------------------------------------------
def _raw(native, ctx, srs, log_N, log_l, w, cxy, cinf, n_comm, ci, ki, vals, pxy, pinf, K, rho=7):
    """kzg_verify_cosets with every size given explicitly: -> return code"""
    vp = native._as_vp
    out_xy = np.zeros((2, 2 * ctx.fp_limbs), dtype=np.uint64)
    out_inf = np.zeros(2, dtype=np.uint8)
    return native.lib().kzg_verify_cosets(ctx._h, srs._h, log_N, log_l, vp(native.int_to_words(w)), vp(cxy), vp(cinf),
                                          n_comm, vp(ci), vp(ki), vp(vals), vp(pxy), vp(pinf), K,
                                          vp(native.int_to_words(rho)), vp(out_xy), vp(out_inf))


@pytest.mark.parametrize("curve", CURVES)
def test_argument_errors_are_refused_and_leave_the_context_usable(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    other = kzgs[[c for c in CURVES if c != curve][0]]
    ctx = kzg._context()
    L, r, p = ctx.fp_limbs, cv.r, cv.p
    ck, w, cxy, cinf, ci, ki, vals, pxy, pinf = _open_cosets_claims(native, ctx, kzg, cv, 16, 16, 0, 1, 5)   # 2^16 cells
    K = ci.size
    good = dict(srs=ck.srs, log_N=16, log_l=0, w=w, cxy=cxy, cinf=cinf, n_comm=1, ci=ci, ki=ki, vals=vals, pxy=pxy,
                pinf=pinf, K=K)

    def rc(**over):
        return _raw(native, ctx, **{**good, **over})

    def still_works():
        xy, inf = ctx.verify_cosets(ck.srs, 16, 0, w, cxy, cinf, ci, ki, vals, pxy, pinf, 99)
        assert trapdoor_holds(curve, cv, xy, inf, 1)

    still_works()
    lag = ctx.srs_lagrange(ck.srs, 4, cv.root_of_unity(16))
    short = mono_key(kzg, 2)
    foreign = mono_key(other, 16)
    bad_ci, bad_ki = ci.copy(), ki.copy()
    bad_ci[K // 2] = 1
    bad_ki[K // 2] = 1 << 16
    off_curve = pxy.copy()
    off_curve[K // 2, 0] ^= np.uint64(1)                                   # x changed: not on the curve
    assert not pinf[K // 2]
    big = pxy.copy()
    big[7, :L] = native.ints_to_limbs([int.from_bytes(pxy[7, :L].tobytes(), "little") + p], L)[0]    # x + p
    big_y = cxy.copy()
    big_y[0, L:] = native.ints_to_limbs([int.from_bytes(cxy[0, L:].tobytes(), "little") + p], L)[0]  # commitment y + p
    off_comm = cxy.copy()
    off_comm[0, L] ^= np.uint64(1)
    cases = {
        "a Lagrange key": dict(srs=lag),
        "a key of another curve": dict(srs=foreign.srs),
        "w not a primitive N-th root": dict(w=w * w % r),
        "w = 1": dict(w=1),
        "commitment index out of range": dict(ci=bad_ci),
        "coset index out of range": dict(ki=bad_ki),
        "log_l above 12": dict(log_l=13, log_N=16),
        "log_N not above log_l": dict(log_l=4, log_N=4),
        "log_N above 21": dict(log_N=22),
        "no commitments": dict(n_comm=0),
        "too many commitments": dict(n_comm=(1 << 16) + 1),
        "K above 2^21": dict(K=(1 << 21) + 1),
        "a proof off the curve in the middle of 2^16": dict(pxy=off_curve),
        "a proof coordinate >= p": dict(pxy=big),
        "a commitment coordinate >= p": dict(cxy=big_y),
        "a commitment off the curve": dict(cxy=off_comm),
    }
    for what, over in cases.items():
        assert rc(**over) == KZG_ERR_ARG, what
        assert native.lib().kzg_last_error(ctx._h), what
        still_works()
    # K * l above 2^24, and a key with fewer than l points (l = 4)
    assert rc(log_l=12, log_N=16, K=(1 << 12) + 1) == KZG_ERR_ARG
    assert rc(srs=short.srs, log_l=2, log_N=16, K=4) == KZG_ERR_ARG
    still_works()
    # K = 0: both points at infinity
    xy, inf = ctx.verify_cosets(ck.srs, 16, 0, w, cxy, cinf, ci[:0], ki[:0], vals[:0], pxy[:0], pinf[:0], 5)
    assert list(inf) == [1, 1] and not xy.any()
    lag.close()


# ---- 4. the commit pipeline's pending results survive the call --------------------------------------------------------
def test_pending_commits_stay_correct_across_a_verification(kzgs, native):
    import torch
    curve = "bls12_381"
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    L = ctx.fp_limbs
    n = 1 << 12
    ck = mono_key(kzg, n)
    polys = random_polys(native, 6, 2, n, cv.r)
    want_xy, want_inf = ctx.commit(ck.srs, polys, [n, n], n)
    _, w, cxy, cinf, ci, ki, vals, pxy, pinf = _open_cosets_claims(native, ctx, kzg, cv, 12, 12, 2, 1, 7)
    d = torch.from_numpy(polys.view(np.int64)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize(ctx.device)
    out_xy = np.zeros((2, 2 * L), dtype=np.uint64)
    out_inf = np.full(2, 9, dtype=np.uint8)
    ctx.commit_device_async(ck.srs, d.data_ptr(), [n, n], n, out_xy, out_inf)
    xy, inf = ctx.verify_cosets(ck.srs, 12, 2, w, cxy, cinf, ci, ki, vals, pxy, pinf, 31337)
    ctx.commit_flush()
    assert trapdoor_holds(curve, cv, xy, inf, 4)
    assert (out_xy == want_xy).all() and (out_inf == want_inf).all()


# ---- 5. facade: real pairings ---------------------------------------------------------------------------------------------
def test_facade_accepts_honest_outputs_and_rejects_tampering():
    from kzg_snark_amd.kzg import KZG
    kzg = KZG("bn254")
    r = kzg.curve_order
    rng = random.Random(11)
    n, l = 16, 4
    ck, rk = kzg.setup(n - 1, tau=TAU)
    rk_l = kzg.coset_verification_key(l, TAU)
    polys = [[rng.randrange(r) for _ in range(n)], [rng.randrange(r) for _ in range(3)]]
    comms = kzg.commit(ck, polys)
    proofs, values = kzg.open_cosets_each(ck, polys, l, n=n, with_values=True)
    C = n // l
    w = int(kzg.Fq.root_of_unity(n))
    ci = [j for j in range(2) for _ in range(C)]
    ki = [i for _ in range(2) for i in range(C)]
    flat_p = [p for row in proofs for p in row]
    flat_v = [v for row in values for v in row]
    rho = 424242
    assert kzg.verify_cosets(ck, rk_l, comms, ci, ki, flat_v, flat_p, l, n, r=rho)
    assert kzg.verify_cosets(ck, rk_l, comms, ci, ki, flat_v, flat_p, l, n)                 # rho sampled
    # the host verifier on the same claims and the same weight
    zeta = pow(w, n // l, r)
    host = kzg.batch_check_cosets(ck, rk_l, [[comms[c]] for c in ci], [pow(w, i, r) for i in ki],
                                  [[v] for v in flat_v], flat_p, [1] * len(ci), zeta=zeta, r=rho)
    assert host is True
    bad_v = [list(v) for v in flat_v]
    bad_v[3][1] = (bad_v[3][1] + 1) % r
    assert not kzg.verify_cosets(ck, rk_l, comms, ci, ki, bad_v, flat_p, l, n, r=rho)
    assert not kzg.batch_check_cosets(ck, rk_l, [[comms[c]] for c in ci], [pow(w, i, r) for i in ki],
                                      [[v] for v in bad_v], flat_p, [1] * len(ci), zeta=zeta, r=rho)
    bad_p = list(flat_p)
    bad_p[2] = kzg.add(bad_p[2], kzg.G1)
    assert not kzg.verify_cosets(ck, rk_l, comms, ci, ki, flat_v, bad_p, l, n, r=rho)
    assert not kzg.verify_cosets(ck, rk, comms, ci, ki, flat_v, flat_p, l, n, r=rho)        # the key of another l
    off = list(flat_p)
    off[1] = (off[1][0], (off[1][1] + 1) % kzg._cv.p, 1)
    assert kzg.verify_cosets(ck, rk_l, comms, ci, ki, flat_v, off, l, n, r=rho) is False    # off the curve: False
    # (xy, inf) arrays and a uint64 value array are taken as they are
    ctx = kzg._context()
    arr, lens, stride = kzg._pack([kzg._coeffs(p) for p in polys])
    table = kzg.coset_table(ck, n, l)
    pxy, pinf, ev = ctx.open_cosets(table.table, np.ascontiguousarray(arr), lens, stride, 4, w, evals=True)
    assert kzg.verify_cosets(ck, rk_l, comms, ci, ki, ev.reshape(-1, l, 4), (pxy.reshape(2 * C, -1), pinf.reshape(-1)),
                             l, n, r=rho)
    # l = 1: the whole output of open_domain
    dproofs = kzg.open_domain_each(ck, polys[:1], n=n)[0]
    dvalues = [O.poly_eval(polys[0], pow(w, i, r), r) for i in range(n)]
    assert kzg.verify_domain(ck, rk, comms[0], dvalues, dproofs, r=rho)
    assert kzg.verify_domain(ck, rk, comms[0], dvalues, dproofs)
    dvalues[5] = (dvalues[5] + 1) % r
    assert not kzg.verify_domain(ck, rk, comms[0], dvalues, dproofs, r=rho)


# ---- 6. one profiling span per call -----------------------------------------------------------------------------------
def test_one_span_per_call(kzgs, native):
    curve = "bn254"
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    ck, w, cxy, cinf, ci, ki, vals, pxy, pinf = _open_cosets_claims(native, ctx, kzg, cv, 8, 9, 3, 2, 8)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for _ in range(3):
            xy, inf = ctx.verify_cosets(ck.srs, 9, 3, w, cxy, cinf, ci, ki, vals, pxy, pinf, 77)
        ms, count = ctx.prof_read("verify_cosets")
        assert count == 3 and ms > 0
        nbytes, have = ctx.prof_read("verify_device_bytes")
        assert have == 1 and nbytes >= ci.size * (2 * 8 * ctx.fp_limbs + 3 * 32)
    finally:
        ctx.prof_enable(False)
    assert trapdoor_holds(curve, cv, xy, inf, 8)

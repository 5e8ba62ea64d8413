"""GPU tests of bulk verification at arbitrary points (csrc/verify_points.hip through the C ABI and the facade): the two
folded points equal the plain-Python restatement (tests/points_restated.py) coordinate for coordinate at the sizes
around a wave, at the edges of the window ladder and of the two sum trees (P + P, P - P and O in lanes the trees pair); they equal kzg_verify_cosets' points at
domain points around the workgroup and launch boundaries; honest openings satisfy L == tau R and stop doing so after a
single change; argument errors are refused and leave the context usable; pending results of the commit pipeline stay
pending and correct; the facade agrees on real pairings.  Equality of integers everywhere."""
import random

import numpy as np
import pytest

from oracle import c_oracle
from oracle import py_oracle as O
from points_restated import restated_LR_points

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
        ck = kzg.setup(n - 1, tau=tau)[0]
        _KEYS[k] = (ck, *ck.srs.export())
    return _KEYS[k]


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


def trapdoor_holds(curve, cv, xy, inf, tau=TAU):
    """L == tau R with one scalar multiplication on the host (the C oracle)"""
    want_xy, want_inf = c_oracle.g1_mul(curve, np.ascontiguousarray(xy[1]), tau % cv.r, inf=bool(inf[1]))
    if want_inf or inf[0]:
        return bool(want_inf) and bool(inf[0])
    return bool((np.asarray(xy[0]) == want_xy).all())


def limbs(native, ints):
    return native.ints_to_limbs([int(v) for v in ints]) if len(ints) else np.zeros((0, 4), dtype=np.uint64)


def agrees_with_the_restatement(native, ctx, cv, cxy, cinf, ci, zs, ys, pxy, pinf, rho):
    L = ctx.fp_limbs
    xy, inf = ctx.verify_points(cxy, cinf, ci, limbs(native, zs), limbs(native, ys), pxy, pinf, rho)
    comms = [to_point(native, L, cxy[j], cinf[j]) for j in range(len(cinf))]
    proofs = [to_point(native, L, pxy[k], pinf[k]) for k in range(len(pinf))]
    wantL, wantR = restated_LR_points(comms, ci, zs, ys, proofs, rho, cv)
    return same_point(native, L, xy[0], inf[0], wantL, cv) and same_point(native, L, xy[1], inf[1], wantR, cv)


# ---- 1. exact points around a wave ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_points_equal_the_restatement_coordinate_for_coordinate(kzgs, native, curve):
    """proofs and commitments are points of a small generated key: the fold is linear and needs no honest claims"""
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    r = cv.r
    rng = random.Random(len(curve))
    _, kxy, kinf = mono_key(kzg, 32)
    for K in (1, 2, 63, 64, 65):
        for n_comm in (1, 3):
            cxy, cinf = kxy[5:5 + n_comm].copy(), kinf[5:5 + n_comm].copy()
            pick = [rng.randrange(32) for _ in range(K)]
            pxy, pinf = kxy[pick].copy(), kinf[pick].copy()
            ci = [rng.randrange(n_comm) for _ in range(K)]
            zs = [rng.randrange(r) for _ in range(K)]
            ys = [rng.randrange(r) for _ in range(K)]
            assert agrees_with_the_restatement(native, ctx, cv, cxy, cinf, ci, zs, ys, pxy, pinf, rng.randrange(1, r)), \
                (K, n_comm)


# ---- 2. the edges of the ladder ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_ladder_edges(kzgs, native, curve):
    """rho = 1: every r_k = 1 and s_k = z_k, so the ladder runs on the scalars chosen here -- all digits zero, the
    digits around the sign change (7, 8, 9, 15, 16, 17), one bit far up, and r - 2, r - 1; then rho = 0 (every scalar
    zero: both points at infinity but for nothing) and rho = r - 1 (weights +-1)"""
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    r = cv.r
    _, kxy, kinf = mono_key(kzg, 32)
    zs = [0, 1, 2, 7, 8, 9, 15, 16, 17, 1 << 128, r - 2, r - 1]
    K = len(zs)
    ys = [0 if k % 2 else r - 1 for k in range(K)]
    cxy, cinf = kxy[1:3].copy(), kinf[1:3].copy()
    pxy, pinf = kxy[3:3 + K].copy(), kinf[3:3 + K].copy()
    ci = [k % 2 for k in range(K)]
    for rho in (1, 0, r - 1):
        assert agrees_with_the_restatement(native, ctx, cv, cxy, cinf, ci, zs, ys, pxy, pinf, rho), rho
    xy, inf = ctx.verify_points(cxy, cinf, ci, limbs(native, zs), limbs(native, ys), pxy, pinf, 0)
    assert list(inf) == [1, 1] and not xy.any()


# ---- 3. the edges of the sum ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_sum_edges(kzgs, native, curve):
    """The workgroup's tree adds lane t + s to lane t in rounds s = 128, 64, .. 1 (lanes beyond K hold O), so the
    special cases of the addition are reached by placing points in lanes the tree pairs.  With rho = 1 every weight
    is 1 and s_k = z_k, so equal proofs with equal z meet with equal scalars in both the R and the s segment.
      a proof at infinity among finite ones
      [P, P]            round 1: P + P -- the doubling branch of the full addition
      [P, Q, P, -Q]     round 2: P + P in lane 0 and Q - Q = O in lane 1; round 1: 2P + O
      [Q, -Q]           round 1: Q - Q; R and the proof term of L vanish
      129 claims, the proofs of lanes 0 and 128 equal: P + P in round 128, the first"""
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    r, p, L = cv.r, cv.p, ctx.fp_limbs
    _, kxy, kinf = mono_key(kzg, 256)
    cxy, cinf = kxy[1:2].copy(), kinf[1:2].copy()
    z = 0x1234567 ** 5 % r
    none = np.zeros(4, dtype=np.uint8)

    def neg(row):
        v = native.limbs_to_ints(row.reshape(2, L))
        return native.ints_to_limbs([v[0], p - v[1]], L).reshape(-1)

    def agrees(pxy, pinf, zs, ys, rho=1):
        return agrees_with_the_restatement(native, ctx, cv, cxy, cinf, [0] * len(zs), zs, ys, pxy, pinf, rho)

    pxy, pinf = kxy[3:8].copy(), kinf[3:8].copy()
    pxy[2], pinf[2] = 0, 1
    assert agrees(pxy, pinf, [z + k for k in range(5)], [7] * 5, rho=31337)
    P, Q = kxy[4], kxy[9]
    assert agrees(np.stack([P, P]), none[:2], [z, z], [1, 2])
    assert agrees(np.stack([P, Q, P, neg(Q)]), none, [z, z + 1, z, z + 1], [1, 2, 3, 4])
    pxy = np.stack([Q, neg(Q)])
    assert agrees(pxy, none[:2], [z, z], [5, 6])
    xy, inf = ctx.verify_points(cxy, cinf, [0, 0], limbs(native, [z, z]), limbs(native, [5, 6]), pxy, none[:2], 1)
    assert inf[1] == 1 and not inf[0]
    pxy, pinf = kxy[20:149].copy(), kinf[20:149].copy()
    pxy[128] = pxy[0]
    zs = [z + k for k in range(129)]
    zs[128] = zs[0]
    assert agrees(pxy, pinf, zs, list(range(129)))


@pytest.mark.parametrize("curve", CURVES)
def test_equal_workgroup_sums_double_in_the_fold(kzgs, native, curve):
    """K = 512, claim k + 256 a copy of claim k, rho = 1: the two workgroups of each scalar vector write the same
    partial point, and vpt_fold_kernel's tree adds them in its last round -- P + P there.  Claims at domain points;
    kzg_verify_cosets with l = 1 folds the same claims (no Python group operations)."""
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    r = cv.r
    log_N, half = 10, 256
    w = cv.root_of_unity(1 << log_N)
    ck, kxy, kinf = mono_key(kzg, 512)
    rng = np.random.default_rng(3)
    pick = np.tile(rng.integers(0, 512, size=half), 2)
    ki = np.tile(rng.integers(0, 1 << log_N, size=half), 2).astype(np.uint32)
    ys = np.tile(rng.integers(0, 1 << 62, size=(half, 4), dtype=np.uint64), (2, 1))
    ys[:, 3] %= np.uint64(r >> 192)
    ci = np.zeros(2 * half, dtype=np.uint32)
    cxy, cinf = kxy[7:8].copy(), kinf[7:8].copy()
    pxy, pinf = kxy[pick].copy(), kinf[pick].copy()
    zs = limbs(native, [pow(w, int(i), r) for i in ki])
    want_xy, want_inf = ctx.verify_cosets(ck.srs, log_N, 0, w, cxy, cinf, ci, ki, ys.reshape(-1, 1, 4), pxy, pinf, 1)
    xy, inf = ctx.verify_points(cxy, cinf, ci, zs, ys, pxy, pinf, 1)
    assert (inf == want_inf).all() and not inf.any()
    assert (xy == want_xy).all()


# ---- 4. wave, workgroup and launch boundaries against the existing verifier ---------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("K", [255, 256, 257, 513, 65792])
def test_domain_points_give_the_points_of_verify_cosets(kzgs, native, curve, K):
    """claims at z_k = w^(i_k), repeated and unordered: kzg_verify_cosets with l = 1 folds the same claims; 65,792 is
    257 workgroups of 256 per scalar vector, more than one ladder launch.  No Python group operations."""
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    r = cv.r
    log_N = 16
    N = 1 << log_N
    w = cv.root_of_unity(N)
    ck, kxy, kinf = mono_key(kzg, 512)
    rng = np.random.default_rng(K)
    cxy, cinf = kxy[100:103].copy(), kinf[100:103].copy()
    pick = rng.integers(0, 512, size=K)
    pxy, pinf = kxy[pick].copy(), kinf[pick].copy()
    ci = rng.integers(0, 3, size=K).astype(np.uint32)
    ki = rng.integers(0, N, size=K).astype(np.uint32)
    ki[:4] = [0, N - 1, N // 2, N - 1]
    wpow = [1] * N
    for i in range(1, N):
        wpow[i] = wpow[i - 1] * w % r
    zs = limbs(native, [wpow[i] for i in ki])
    ys = rng.integers(0, 1 << 63, size=(K, 4), dtype=np.uint64)
    ys[:, 3] %= np.uint64(r >> 192)                                        # reduced
    rho = 0xabcdef ** 9 % r
    want_xy, want_inf = ctx.verify_cosets(ck.srs, log_N, 0, w, cxy, cinf, ci, ki, ys.reshape(K, 1, 4), pxy, pinf, rho)
    xy, inf = ctx.verify_points(cxy, cinf, ci, zs, ys, pxy, pinf, rho)
    assert (inf == want_inf).all() and not inf.any()
    assert (xy == want_xy).all()


# ---- 5. truth and tampering -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_honest_openings_verify_and_single_changes_are_caught(kzgs, native, curve):
    """n = 256: all proofs of kzg_open_domain plus 8 proofs of kzg_open at random z (xi = 1), one commitment"""
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    r, L = cv.r, ctx.fp_limbs
    n, log_n = 256, 8
    ck, _, _ = mono_key(kzg, n)
    w = cv.root_of_unity(n)
    rng = random.Random(5)
    poly = limbs(native, [rng.randrange(r) for _ in range(n)]).reshape(1, n, 4)
    cxy, cinf = ctx.commit(ck.srs, poly, [n], n)
    table = ctx.domain_table(ck.srs, log_n)
    dxy, dinf, dev = ctx.open_domain(table, poly, [n], n, w, evals=True)
    table.close()
    zs = [pow(w, i, r) for i in range(n)] + [rng.randrange(r) for _ in range(8)]
    pxy = np.zeros((n + 8, 2 * L), dtype=np.uint64)
    pinf = np.zeros(n + 8, dtype=np.uint8)
    ys = np.zeros((n + 8, 4), dtype=np.uint64)
    pxy[:n], pinf[:n], ys[:n] = dxy.reshape(n, -1), dinf.reshape(n), dev.reshape(n, 4)
    for k in range(n, n + 8):
        xy, inf, ev = ctx.open(ck.srs, poly, [n], n, native.int_to_words(zs[k]), native.int_to_words(1))
        pxy[k], pinf[k], ys[k] = xy, inf[0], ev
    K = n + 8
    ci = np.zeros(K, dtype=np.uint32)
    zl = limbs(native, zs)
    rho = 0x27182818 ** 8 % r
    two_xy = np.concatenate([cxy, pxy[:1]])                                # a second, wrong commitment to point at
    two_inf = np.concatenate([cinf, pinf[:1]])

    def holds(cxy=cxy, cinf=cinf, ci=ci, zl=zl, ys=ys, pxy=pxy, pinf=pinf):
        xy, inf = ctx.verify_points(cxy, cinf, ci, zl, ys, pxy, pinf, rho)
        return trapdoor_holds(curve, cv, xy, inf)

    assert holds()
    assert holds(cxy=two_xy, cinf=two_inf)
    bad = ys.copy()
    bad[n + 3, 2] ^= np.uint64(1 << 20)                                    # one limb of one y (still reduced)
    assert not holds(ys=bad)
    bad = zl.copy()
    bad[n + 5] = native.int_to_words((zs[n + 5] + 1) % r)                  # one z
    assert not holds(zl=bad)
    bad = pxy.copy()
    bad[[5, n + 1]] = bad[[n + 1, 5]]                                      # two distinct proofs swapped
    assert (pxy[5] != pxy[n + 1]).any()
    assert not holds(pxy=bad)
    bad = ci.copy()
    bad[77] = 1                                                            # one wrong commitment index
    assert not holds(cxy=two_xy, cinf=two_inf, ci=bad)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def _raw(native, ctx, cxy, cinf, n_comm, ci, zl, ys, pxy, pinf, K, rho=7):
    """kzg_verify_points with every size given explicitly: -> return code"""
    vp = native._as_vp
    out_xy = np.zeros((2, 2 * ctx.fp_limbs), dtype=np.uint64)
    out_inf = np.zeros(2, dtype=np.uint8)
    return native.lib().kzg_verify_points(ctx._h, vp(cxy), vp(cinf), n_comm, vp(ci), vp(zl), vp(ys), vp(pxy), vp(pinf),
                                          K, vp(native.int_to_words(rho)), vp(out_xy), vp(out_inf))


@pytest.mark.parametrize("curve", CURVES)
def test_argument_errors_are_refused_and_leave_the_context_usable(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    L, r, p = ctx.fp_limbs, cv.r, cv.p
    _, kxy, kinf = mono_key(kzg, 512)
    K = 300
    rng = random.Random(9)
    cxy, cinf = kxy[1:3].copy(), kinf[1:3].copy()
    pxy, pinf = kxy[100:100 + K].copy(), kinf[100:100 + K].copy()
    ci = np.array([k % 2 for k in range(K)], dtype=np.uint32)
    zs = [rng.randrange(r) for _ in range(K)]
    ys = [rng.randrange(r) for _ in range(K)]
    zl, yl = limbs(native, zs), limbs(native, ys)
    good = dict(cxy=cxy, cinf=cinf, n_comm=2, ci=ci, zl=zl, ys=yl, pxy=pxy, pinf=pinf, K=K)

    def rc(**over):
        return _raw(native, ctx, **{**good, **over})

    def still_works():
        assert agrees_with_the_restatement(native, ctx, cv, cxy, cinf, list(ci[:3]), zs[:3], ys[:3], pxy[:3], pinf[:3], 99)

    bad_ci = ci.copy()
    bad_ci[K // 2] = 2
    off_curve = pxy.copy()
    off_curve[K // 2, 0] ^= np.uint64(1)                                   # x changed: not on the curve
    big = pxy.copy()
    big[7, :L] = native.ints_to_limbs([int.from_bytes(pxy[7, :L].tobytes(), "little") + p], L)[0]    # x + p
    big_y = cxy.copy()
    big_y[0, L:] = native.ints_to_limbs([int.from_bytes(cxy[0, L:].tobytes(), "little") + p], L)[0]  # commitment y + p
    off_comm = cxy.copy()
    off_comm[1, L] ^= np.uint64(1)
    cases = {
        "commitment index out of range": dict(ci=bad_ci),
        "no commitments": dict(n_comm=0),
        "too many commitments": dict(n_comm=(1 << 16) + 1),
        "K above 2^21": dict(K=(1 << 21) + 1),
        "a proof off the curve": dict(pxy=off_curve),
        "a proof coordinate >= p": dict(pxy=big),
        "a commitment coordinate >= p": dict(cxy=big_y),
        "a commitment off the curve": dict(cxy=off_comm),
    }
    assert rc() == 0
    for what, over in cases.items():
        assert rc(**over) == KZG_ERR_ARG, what
        assert native.lib().kzg_last_error(ctx._h), what
        still_works()
    # K = 0: both points at infinity
    xy, inf = ctx.verify_points(cxy, cinf, ci[:0], zl[:0], yl[:0], pxy[:0], pinf[:0], 5)
    assert list(inf) == [1, 1] and not xy.any()


# ---- 7. the commit pipeline is not touched ---------------------------------------------------------------------------------
def test_pending_commits_stay_pending_and_correct_across_a_verification(kzgs, native):
    import torch
    curve = "bls12_381"
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    L, r = ctx.fp_limbs, cv.r
    n = 1 << 12
    ck, kxy, kinf = mono_key(kzg, n)
    rng = np.random.default_rng(6)
    polys = rng.integers(0, 1 << 63, size=(2, n, 4), dtype=np.uint64)
    polys[..., 3] %= np.uint64(r >> 192)
    want_xy, want_inf = ctx.commit(ck.srs, polys, [n, n], n)
    K = 70
    zs, ys = [int(v) for v in rng.integers(1, 1 << 62, size=K)], [int(v) for v in rng.integers(1, 1 << 62, size=K)]
    d = torch.from_numpy(polys.view(np.int64)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize(ctx.device)
    out_xy = np.zeros((2, 2 * L), dtype=np.uint64)
    out_inf = np.full(2, 9, dtype=np.uint8)
    ctx.commit_device_async(ck.srs, d.data_ptr(), [n, n], n, out_xy, out_inf)
    ok = agrees_with_the_restatement(native, ctx, cv, kxy[1:2], kinf[1:2], [0] * K, zs, ys, kxy[10:10 + K], kinf[10:10 + K],
                                     31337)
    assert len(ctx._inflight) == 1 and (out_inf == 9).all()               # not retired: delivered at the flush
    ctx.commit_flush()
    assert ok
    assert (out_xy == want_xy).all() and (out_inf == want_inf).all()


# ---- 8. facade: real pairings ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_facade_accepts_honest_blobs_and_rejects_tampering(kzgs, curve):
    kzg = kzgs[curve]
    r = kzg.curve_order
    rng = random.Random(11)
    n = 64
    lk, rk = kzg.setup_lagrange(n, tau=TAU)
    w = lk.w
    blobs = [[rng.randrange(r) for _ in range(n)] for _ in range(3)] + [[rng.randrange(r) for _ in range(40)]]
    comms = kzg.commit_evaluations(lk, blobs)
    zs = [rng.randrange(r), pow(w, 5, r), rng.randrange(r), rng.randrange(r)]          # one challenge in the domain
    proofs = [kzg.open_evaluations(lk, [blob], z, 1) for blob, z in zip(blobs, zs)]
    rho = 424242
    assert kzg.verify_blobs(lk, rk, comms, blobs, zs, proofs, r=rho) is True
    assert kzg.verify_blobs(w, rk, comms, blobs, zs, proofs) is True                    # the root alone; rho sampled
    ys = kzg.evaluate_evaluations_each(lk, blobs, zs)
    assert [int(y) for y in ys] == [int(kzg.evaluate_evaluations(lk, blob, z)) for blob, z in zip(blobs, zs)]
    assert int(ys[1]) == blobs[1][5]
    idx = list(range(4))
    assert kzg.verify_points(rk, comms, idx, zs, ys, proofs, r=rho) is True

    bad_blobs = [list(b) for b in blobs]
    bad_blobs[2][17] = (bad_blobs[2][17] + 1) % r                                        # one changed value
    bad_proofs = [proofs[1], proofs[0]] + proofs[2:]                                     # one swapped pair of proofs
    bad_zs = zs[:3] + [(zs[3] + 1) % r]                                                  # one changed challenge
    assert kzg.verify_blobs(lk, rk, comms, bad_blobs, zs, proofs, r=rho) is False
    assert kzg.verify_blobs(lk, rk, comms, blobs, zs, bad_proofs, r=rho) is False
    assert kzg.verify_blobs(lk, rk, comms, blobs, bad_zs, proofs, r=rho) is False
    bad_ys = kzg.evaluate_evaluations_each(lk, bad_blobs, zs)
    assert kzg.verify_points(rk, comms, idx, zs, bad_ys, proofs, r=rho) is False
    assert kzg.verify_points(rk, comms, idx, zs, ys, bad_proofs, r=rho) is False
    assert kzg.verify_points(rk, comms, idx, bad_zs, ys, proofs, r=rho) is False
    off = list(proofs)
    off[0] = (off[0][0], (off[0][1] + 1) % kzg._cv.p, 1)
    assert kzg.verify_points(rk, comms, idx, zs, ys, off, r=rho) is False               # off the curve: False
    if curve == "bls12_381":
        from g1_bytes_cases import subgroup_matrix
        from kzg_snark_amd import curve as C
        cv = kzg._cv
        t = next(pt for pt, ok, what in subgroup_matrix() if what.startswith("T"))
        forged = list(proofs)
        forged[2] = C.g1_group(cv).add(forged[2], t)                                     # on the curve, outside G1
        assert C.on_curve_g1(forged[2], cv) and not C.in_subgroup_g1(forged[2], cv)
        assert kzg.verify_points(rk, comms, idx, zs, ys, forged, r=rho, check_subgroup=True) is False
        assert kzg.verify_points(rk, comms, idx, zs, ys, proofs, r=rho, check_subgroup=True) is True
        assert kzg.verify_blobs(lk, rk, comms, blobs, zs, forged, r=rho, check_subgroup=True) is False


# ---- 9. one profiling span per call -----------------------------------------------------------------------------------
def test_one_span_per_call(kzgs, native):
    curve = "bn254"
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    _, kxy, kinf = mono_key(kzg, 512)
    K = 300
    zl, yl = limbs(native, range(1, K + 1)), limbs(native, range(K, 2 * K))
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for _ in range(3):
            ctx.verify_points(kxy[:1], kinf[:1], [0] * K, zl, yl, kxy[5:5 + K], kinf[5:5 + K], 77)
        ms, count = ctx.prof_read("verify_points")
        assert count == 3 and ms > 0
        nbytes, have = ctx.prof_read("verify_points_device_bytes")
        assert have == 1 and nbytes >= K * (2 * 8 * ctx.fp_limbs + 4 * 32)
    finally:
        ctx.prof_enable(False)

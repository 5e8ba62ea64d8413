"""GPU tests of the pairing-product checks (csrc/pairing.hip through the C ABI and the facade): values
against kzg_snark_amd/pairing.py to the power c; bilinearity, infinity, malformed and out-of-subgroup points built with
the trapdoor (a G1, b G2 with known a, b -- no host pairing); batches at the edges of the launch layout; the commit
pipeline left alone; the facade's verifiers with the pairing on the device and on the host; then what separates the wave
from the host's lane loop and the inputs the header documents -- lanes past 64 (k = 11 .. 16) with values at every
equation index, skip patterns, NULL flag arrays, the context's buffer across layouts, a malformed finite point beside an
infinite partner, a twist point outside the subgroup, the verifiers with L or R at infinity.  Equality of integers and
of verdicts everywhere."""
import ctypes
import random

import numpy as np
import pytest

from g1_bytes_cases import golden_failures
from kzg_snark_amd import curve as C
from kzg_snark_amd import pairing as PR

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
KZG_ERR_ARG = -1
# The launch layout of csrc/pairing.hip: one wave of 64 lanes per workgroup, one equation per
# workgroup, a grid of m workgroups and no grid-stride loop; the MI355X has 256 compute units, so 257 equations put a
# second workgroup on one of them.
EQUATIONS_PER_WORKGROUP = 1
COMPUTE_UNITS = 256
MAX_PAIRS = 16
POOL = 8


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


class Pool:
    """POOL scalars per side with their points a_i G1 and b_j G2, and the G1 points that close an equation:
    closing(s) = -s G1, so [(a G1, b G2), (closing(a b), G2)] has the product one"""

    def __init__(self, kzg, native, seed):
        self.kzg, self.native, self.cv = kzg, native, kzg._cv
        self.L = (self.cv.p.bit_length() + 63) // 64
        rng = random.Random(seed)
        r = self.cv.r
        self.a = [rng.randrange(1, r) for _ in range(POOL)]
        self.b = [rng.randrange(1, r) for _ in range(POOL)]
        self.A = [kzg.multiply(kzg.G1, a) for a in self.a]
        self.B = [kzg.multiply(kzg.G2, b) for b in self.b]
        self._closing = {}

    def closing(self, s):
        s %= self.cv.r
        if s not in self._closing:
            self._closing[s] = self.kzg.neg(self.kzg.multiply(self.kzg.G1, s)) if s else self.kzg.Z1
        return self._closing[s]

    def equation(self, i, j, holds=True):
        """k = 2: e(a_i G1, b_j G2) e(-(a_i b_j [+ 1]) G1, G2)"""
        return [(self.A[i], self.B[j]), (self.closing(self.a[i] * self.b[j] + (0 if holds else 1)), self.kzg.G2)]

    def arrays(self, equations):
        g1 = self.native.points_to_limbs([pr[0] for e in equations for pr in e], self.L)
        g2 = self.native.g2_points_to_limbs([pr[1] for e in equations for pr in e], self.L)
        return g1[0], g1[1], g2[0], g2[1]


_POOLS = {}


@pytest.fixture
def pool(kzgs, native, curve):
    if curve not in _POOLS:
        _POOLS[curve] = Pool(kzgs[curve], native, seed=len(curve))
    return _POOLS[curve]


def statuses(pool, equations):
    ctx = pool.kzg._context()
    return list(ctx.pairing_check(*pool.arrays(equations), len(equations[0])))


# ---- 1. values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_values_equal_the_host_pairing_to_the_power_c(pool, native, curve):
    kzg, cv = pool.kzg, pool.cv
    K = PR._CURVES[curve].K
    c = native.PAIRING_GT_MULTIPLE[curve]
    assert c == (3 if curve == "bls12_381" else 1)
    host = [list(kzg.pairing(pool.B[i + 1], pool.A[i])) for i in range(2)]
    for i in range(2):
        assert kzg.pairing_product([(pool.A[i], pool.B[i + 1])]) == tuple(K.pow(host[i], c))
    both = [(pool.A[0], pool.B[1]), (pool.A[1], pool.B[2])]
    assert kzg.pairing_product(both) == tuple(K.pow(K.mul(host[0], host[1]), c))
    assert kzg.pairing_check(both) is False
    assert kzg.pairing_product([both, pool.equation(0, 0)])[1] == tuple(K.one)


# ---- 2. bilinearity by trapdoor ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_bilinearity_by_trapdoor(pool, native, curve):
    kzg, r = pool.kzg, pool.cv.r
    assert statuses(pool, [pool.equation(2, 3)]) == [0]
    assert statuses(pool, [pool.equation(2, 3, holds=False)]) == [1]
    for k in (3, 4, MAX_PAIRS):
        idx = [(t % POOL, (3 * t + 1) % POOL) for t in range(k - 1)]
        total = sum(pool.a[i] * pool.b[j] for i, j in idx)
        eq = [(pool.A[i], pool.B[j]) for i, j in idx]
        assert statuses(pool, [eq + [(pool.closing(total), kzg.G2)]]) == [0], k
        assert statuses(pool, [eq + [(pool.closing(total + 1), kzg.G2)]]) == [1], k
        assert kzg.pairing_check(eq + [(pool.closing(total), kzg.G2)]) is True
    # the range of k, refused before anything is queued
    ctx = kzg._context()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                       # noqa: E731
    eq = [(pool.A[0], pool.B[0])] * (MAX_PAIRS + 1)
    g1, _, g2, _ = pool.arrays([eq])
    st = np.full(1, 9, dtype=np.uint8)
    gt = np.zeros((1, 12, pool.L), dtype=np.uint64)
    lib = native.lib()
    for k in (MAX_PAIRS + 1, 0):
        assert lib.kzg_pairing_check(ctx._h, vp(g1), None, vp(g2), None, 1, k, vp(st)) == KZG_ERR_ARG, k
        assert lib.kzg_pairing_product(ctx._h, vp(g1), None, vp(g2), None, 1, k, vp(gt), vp(st)) == KZG_ERR_ARG, k
    assert lib.kzg_pairing_check(ctx._h, vp(g1), None, vp(g2), None, (1 << 20) + 1, 1, vp(st)) == KZG_ERR_ARG
    assert st[0] == 9
    assert lib.kzg_pairing_check(ctx._h, None, None, None, None, 0, 2, None) == 0          # m = 0: no work
    with pytest.raises(ValueError):
        kzg.pairing_check(eq)
    with pytest.raises(ValueError):
        kzg.pairing_check([[(pool.A[0], pool.B[0])], [(pool.A[0], pool.B[0])] * 2])
    assert statuses(pool, [pool.equation(1, 1)]) == [0]                                      # the context still works


# ---- 3. infinity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_infinity_skips_a_pair(pool, curve):
    kzg = pool.kzg
    P, Q, Q2 = pool.A[0], pool.B[0], pool.B[1]
    O1, O2 = kzg.Z1, kzg.Z2
    one = [[(O1, Q)], [(P, O2)], [(O1, O2)]]
    assert statuses(pool, one) == [0, 0, 0]
    three = [[(P, Q), (O1, Q2), (kzg.neg(P), Q)], [(O1, Q), (P, O2), (O1, O2)], [(P, Q), (kzg.neg(P), Q), (P, O2)]]
    assert statuses(pool, three) == [0, 0, 0]
    assert statuses(pool, [[(P, Q), (O1, Q2)], [(O1, Q2), (P, Q)], [(O1, Q), (O1, Q2)]]) == [1, 1, 0]


# ---- 4. malformed points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_malformed_points_give_status_2_for_their_equation_only(pool, native, curve):
    kzg, p, L = pool.kzg, pool.cv.p, pool.L
    ctx = kzg._context()
    eqs = [pool.equation(t % POOL, (t + 2) % POOL, holds=t not in (2, 5)) for t in range(8)]
    g1, g1_inf, g2, g2_inf = pool.arrays(eqs)
    assert list(ctx.pairing_check(g1, g1_inf, g2, g2_inf, 2)) == [0, 0, 1, 0, 0, 1, 0, 0]
    limbs = lambda v: native.ints_to_limbs([v], L)[0]                     # noqa: E731
    g1[2 * 1 + 1, L] ^= np.uint64(1)                                       # equation 1, second pair: G1 off the curve
    g2[2 * 3 + 0, 2 * L] ^= np.uint64(1)                                   # equation 3, first pair: G2 off the twist
    g1[2 * 4 + 0, :L] = limbs(p)                                           # equation 4: a G1 coordinate equal to p
    x_c1 = native.limbs_to_ints(g2[2 * 6 + 1, L:2 * L].reshape(1, L))[0]
    g2[2 * 6 + 1, L:2 * L] = limbs(x_c1 + p)                               # equation 6: x.c1 + p, c1 alone >= p
    want = [0, 2, 1, 2, 2, 1, 2, 0]
    assert list(ctx.pairing_check(g1, g1_inf, g2, g2_inf, 2)) == want
    gt, status = ctx.pairing_product(g1, g1_inf, g2, g2_inf, 2)
    assert list(status) == want
    one = native.gt_to_tuple(gt[0], curve)
    assert one == tuple(PR._CURVES[curve].K.one) == native.gt_to_tuple(gt[7], curve)
    for e, st in enumerate(want):
        assert gt[e].any() == (st != 2), e                                  # zeros where the status is 2
    # a malformed point beside an infinity flag: the flag wins over the coordinates
    g1_inf[2 * 1 + 1] = 1
    assert list(ctx.pairing_check(g1, g1_inf, g2, g2_inf, 2))[1] == 1
    assert kzg.pairing_check([(pool.A[0], ((1, 2), (3, 4), (1, 0)))]) is False
    with pytest.raises(ValueError):
        kzg.pairing_product([(pool.A[0], ((1, 2), (3, 4), (1, 0)))])


# ---- 5. input the call does not vet ---------------------------------------------------------------------------------------
def test_a_g1_point_outside_the_subgroup_neither_traps_nor_hangs(kzgs, native):
    curve = "bls12_381"
    if curve not in _POOLS:
        _POOLS[curve] = Pool(kzgs[curve], native, seed=len(curve))
    pool = _POOLS[curve]
    blob = next(b for b, st, _ in golden_failures(curve) if st == 3)
    T, st = C.decompress_g1_status(blob, pool.cv, check_subgroup=False)
    assert st == 0 and C.on_curve_g1(T, pool.cv) and not C.in_subgroup_g1(T, pool.cv)
    eqs = [pool.equation(0, 1), [(T, pool.B[0]), (pool.A[1], pool.B[1])], pool.equation(1, 0, holds=False)]
    got = statuses(pool, eqs)
    # pairing.py meets no vertical line on T, and the Miller function it evaluates is the device's whatever the order
    # of T: the value of [(T, B0)] is its value to the power c, and the status of the two pairs follows from its product
    kzg, K, c = pool.kzg, PR._CURVES[curve].K, native.PAIRING_GT_MULTIPLE[curve]
    host_t = list(kzg.pairing(pool.B[0], T))
    host = K.mul(host_t, list(kzg.pairing(pool.B[1], pool.A[1])))
    assert got == [0, 0 if host == K.one else 1, 1]
    assert kzg.pairing_product([(T, pool.B[0])]) == tuple(K.pow(host_t, c))
    assert kzg.pairing_product(eqs[1]) == tuple(K.pow(host, c))


# ---- 6. batches at the edges of the layout ----------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_batches_at_the_layout_edges(pool, curve):
    ctx = pool.kzg._context()
    rng = random.Random(7 + len(curve))
    for m in (EQUATIONS_PER_WORKGROUP, EQUATIONS_PER_WORKGROUP - 1, EQUATIONS_PER_WORKGROUP + 1, 2, COMPUTE_UNITS + 1):
        pattern = [rng.randrange(2) == 0 for _ in range(m)]
        picks = [(rng.randrange(POOL), rng.randrange(POOL)) for _ in range(m)]
        eqs = [pool.equation(i, j, holds=h) for (i, j), h in zip(picks, pattern)]
        if m == 0:
            empty = np.zeros((0, 2 * pool.L), dtype=np.uint64), None, np.zeros((0, 4 * pool.L), dtype=np.uint64), None
            assert list(ctx.pairing_check(*empty, 2)) == []
            continue
        assert statuses(pool, eqs) == [0 if h else 1 for h in pattern], m
    assert pool.kzg.pairing_check([]) == []


# ---- 7. the commit pipeline is not touched ------------------------------------------------------------------------------
def test_pending_commits_stay_pending_and_correct_across_a_pairing_check(kzgs, native):
    import torch
    curve = "bls12_381"
    kzg = kzgs[curve]
    if curve not in _POOLS:
        _POOLS[curve] = Pool(kzg, native, seed=len(curve))
    pool = _POOLS[curve]
    ctx = kzg._context()
    L, r = ctx.fp_limbs, pool.cv.r
    n = 1 << 8
    ck = kzg.setup(n - 1, tau=TAU)[0]
    rng = np.random.default_rng(6)
    polys = rng.integers(0, 1 << 63, size=(2, n, 4), dtype=np.uint64)
    polys[..., 3] %= np.uint64(r >> 192)
    want_xy, want_inf = ctx.commit(ck.srs, polys, [n, n], n)
    d = torch.from_numpy(polys.view(np.int64)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize(ctx.device)
    out_xy = np.zeros((2, 2 * L), dtype=np.uint64)
    out_inf = np.full(2, 9, dtype=np.uint8)
    ctx.commit_device_async(ck.srs, d.data_ptr(), [n, n], n, out_xy, out_inf)
    got = statuses(pool, [pool.equation(0, 0), pool.equation(1, 2, holds=False), pool.equation(3, 3)])
    assert len(ctx._inflight) == 1 and (out_inf == 9).all()               # not retired: delivered at the flush
    ctx.commit_flush()
    assert got == [0, 1, 0]
    assert (out_xy == want_xy).all() and (out_inf == want_inf).all()


# ---- 8. facade --------------------------------------------------------------------------------------------------------
def test_pairing_check_on_a_real_opening_agrees_with_check(kzgs):
    kzg = kzgs["bn254"]
    r = kzg.curve_order
    rng = random.Random(3)
    ck, rk = kzg.setup(7, tau=TAU)
    poly = kzg.R([rng.randrange(r) for _ in range(8)])
    z, xi = rng.randrange(r), rng.randrange(r)
    comms = kzg.commit(ck, [poly])
    evals = [poly(kzg.Fq(z))]
    proof = kzg.open(ck, [poly], z, xi)
    assert kzg.check(rk, comms, z, evals, proof, xi) is True

    def on_device(values):
        F = kzg._folded_claim(comms, values, kzg.Fq(xi))
        shifted = kzg.add(rk, kzg.neg(kzg.multiply(kzg.G2, z)))
        return kzg.pairing_check([(F, kzg.G2), (kzg.neg(proof), shifted)])

    assert on_device(evals) is True
    assert on_device([evals[0] + 1]) is False


def test_verify_points_agrees_between_host_and_device_pairings(kzgs):
    kzg = kzgs["bls12_381"]
    r = kzg.curve_order
    rng = random.Random(5)
    n = 8
    lk, rk = kzg.setup_lagrange(n, tau=TAU)
    values = [[rng.randrange(r) for _ in range(n)] for _ in range(n)]
    comms = kzg.commit_evaluations(lk, values)
    zs = [rng.randrange(r) for _ in range(n)]
    ys = [int(y) for y in kzg.evaluate_evaluations_each(lk, values, zs)]
    proofs = [kzg.open_evaluations(lk, [values[j]], zs[j], 1) for j in range(n)]
    idx = list(range(n))
    assert kzg.verify_points(rk, comms, idx, zs, ys, proofs, r=77) is True
    assert kzg.verify_points(rk, comms, idx, zs, ys, proofs, r=77, pairing="host") is True
    ys[5] = (ys[5] + 1) % r
    assert kzg.verify_points(rk, comms, idx, zs, ys, proofs, r=77) is False
    assert kzg.verify_points(rk, comms, idx, zs, ys, proofs, r=77, pairing="host") is False
    with pytest.raises(ValueError):
        kzg.verify_points(rk, comms, idx, zs, ys, proofs, pairing="gpu")


@pytest.mark.parametrize("curve", CURVES)
def test_blob_batch_agrees_between_host_and_device_pairings(kzgs, curve):
    kzg = kzgs[curve]
    r = kzg.curve_order
    rng = random.Random(9)
    n = b = 8
    lk, rk = kzg.setup_lagrange(n, tau=TAU)
    blobs = [b"".join(rng.randrange(r).to_bytes(32, "big") for _ in range(n)) for _ in range(b)]
    comms = kzg.blob_to_kzg_commitment(lk, blobs)
    proofs = kzg.compute_blob_kzg_proof(lk, blobs, comms)
    assert kzg.verify_blob_kzg_proof_batch(lk, rk, blobs, comms, proofs) is True
    assert kzg.verify_blob_kzg_proof_batch(lk, rk, blobs, comms, proofs, pairing="host") is True
    swapped = [proofs[1], proofs[0]] + proofs[2:]
    assert kzg.verify_blob_kzg_proof_batch(lk, rk, blobs, comms, swapped) is False
    assert kzg.verify_blob_kzg_proof_batch(lk, rk, blobs, comms, swapped, pairing="host") is False


# ---- 9 .. 15: what separates the device run from the host run ---------------------------------------------------------
# The host shim runs fp_tower.h's phases one lane after the other; the wave runs lane t, t + 64, ... and meets.  The
# per-pair product phases are k * jobs lanes wide with jobs up to 6: they pass the wave's 64 lanes from k = 11 (66 lanes,
# the 6-job phases) and, in the 5-job phase, from k = 13 (65).  Expected values come from the trapdoor: the product of
# (a_i G1, b_j G2) over the live pairs is E^(sum a_i b_j) with E = pairing.py's e(G1, G2), one host pairing per curve,
# and the device's value is that to the power c.
_GENERATOR_PAIRING = {}
_GT_POWERS = {}


def gt_power(pool, native, curve, delta):
    """E^(c delta) as kzg_pairing_product's tuple"""
    if curve not in _GENERATOR_PAIRING:
        _GENERATOR_PAIRING[curve] = list(pool.kzg.pairing(pool.kzg.G2, pool.kzg.G1))
    e = native.PAIRING_GT_MULTIPLE[curve] * delta % pool.cv.r
    if (curve, e) not in _GT_POWERS:
        _GT_POWERS[curve, e] = tuple(PR._CURVES[curve].K.pow(_GENERATOR_PAIRING[curve], e))
    return _GT_POWERS[curve, e]


def pair_indices(k):
    return [(t % POOL, (3 * t + 1) % POOL) for t in range(k)]


def chain(pool, k, delta=0, skip1=(), skip2=()):
    """k pairs whose product is E^delta: pair t is (a_i G1, b_j G2), its G1 point infinity for t in skip1 and its G2
    point for t in skip2; the last pair that is left closes the others: (-(sum a_i b_j - delta) G1, G2)"""
    kzg = pool.kzg
    live = [t for t in range(k) if t not in skip1 and t not in skip2]
    idx = pair_indices(k)
    total = sum(pool.a[idx[t][0]] * pool.b[idx[t][1]] for t in live[:-1])
    pairs = []
    for t, (i, j) in enumerate(idx):
        P, Q = (pool.closing(total - delta), kzg.G2) if t == live[-1] else (pool.A[i], pool.B[j])
        pairs.append((kzg.Z1 if t in skip1 else P, kzg.Z2 if t in skip2 else Q))
    return pairs


def gt_tuples(native, curve, gt):
    return [native.gt_to_tuple(row, curve) for row in gt]


def products(pool, native, curve, equations):
    """kzg_pairing_product on the pool's context -> (values as pairing.py's tuples, statuses)"""
    gt, status = pool.kzg._context().pairing_product(*pool.arrays(equations), len(equations[0]))
    return gt_tuples(native, curve, gt), [int(s) for s in status]


# ---- 9. lanes past the wave: statuses and values at every equation index ---------------------------------------------
@pytest.mark.parametrize("k", [10, 11, 13, 16])
@pytest.mark.parametrize("curve", CURVES)
def test_wrapped_lanes_give_the_trapdoor_values_at_every_equation_index(pool, native, curve, k):
    S = 0x1234_5678_9abc_def0_0fed_cba9 + k
    # (i) closes; (ii) the closing scalar of the LAST pair, the one whose lanes wrap, is off by one: E^-1; (iii) E^S
    eqs = [chain(pool, k), chain(pool, k, delta=-1), chain(pool, k, delta=S)]
    values, status = products(pool, native, curve, eqs)
    assert status == [0, 1, 1]
    one = tuple(PR._CURVES[curve].K.one)
    assert gt_power(pool, native, curve, 0) == one != gt_power(pool, native, curve, -1)
    assert values == [one, gt_power(pool, native, curve, -1), gt_power(pool, native, curve, S)]
    assert statuses(pool, eqs) == [0, 1, 1]


# ---- 10. skips ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_skip_patterns_give_the_product_of_the_live_pairs(pool, native, curve):
    kzg = pool.kzg
    one = tuple(PR._CURVES[curve].K.one)
    P, Q = pool.A[0], pool.B[0]
    # the first pair skipped and the product one: the search of OP_PAIRS_BEGIN starts past pair 0
    values, status = products(pool, native, curve, [[(kzg.Z1, pool.B[1]), (P, Q), (kzg.neg(P), Q)]])
    assert status == [0] and values == [one]
    k = MAX_PAIRS
    idx = pair_indices(k)
    eqs = [chain(pool, k, skip1=range(0, k, 2), skip2=(1, 15)),                        # live: 3, 5, ..., 13, closing to one
           chain(pool, k, delta=5, skip1=range(0, k, 2), skip2=(1, 15))]               # the same pattern, E^5
    want = [one, gt_power(pool, native, curve, 5)]
    for live in (0, k - 1):                    # one pair alone, the first and the last; the others lose G1 or G2 in turn
        eqs.append([(pool.A[i], pool.B[j]) if t == live else (kzg.Z1, pool.B[j]) if t % 2 == 0 else (pool.A[i], kzg.Z2)
                    for t, (i, j) in enumerate(idx)])
        want.append(gt_power(pool, native, curve, pool.a[idx[live][0]] * pool.b[idx[live][1]]))
    values, status = products(pool, native, curve, eqs)
    assert status == [0, 1, 1, 1]
    assert values == want
    assert statuses(pool, eqs) == [0, 1, 1, 1]


@pytest.mark.parametrize("curve", CURVES)
def test_a_g2_infinity_flag_wins_over_garbage_coordinates(pool, native, curve):
    kzg, L = pool.kzg, pool.L
    ctx = kzg._context()
    s0, s1 = pool.a[0] * pool.b[1], pool.a[1] * pool.b[2]
    eqs = [[(pool.A[0], pool.B[1]), (pool.A[2], kzg.Z2), (pool.closing(s0), kzg.G2)],
           [(pool.A[2], kzg.Z2), (pool.A[0], pool.B[1]), (pool.A[1], pool.B[2])]]
    g1, g1_inf, g2, g2_inf = pool.arrays(eqs)
    assert list(g2_inf) == [0, 1, 0, 1, 0, 0]
    g2 = g2.copy()
    g2[1, :] = np.uint64(0xffff_ffff_ffff_ffff)                              # every coordinate >= p, off the twist
    g2[3, :] = g2[0, :]
    g2[3, 2 * L] ^= np.uint64(1)                                             # below p, off the twist
    g2[3, :L] = native.ints_to_limbs([pool.cv.p], L)[0]                      # and x.c0 = p
    gt, status = ctx.pairing_product(g1, g1_inf, g2, g2_inf, 3)
    assert list(status) == [0, 1]
    assert gt_tuples(native, curve, gt) == [gt_power(pool, native, curve, 0), gt_power(pool, native, curve, s0 + s1)]
    assert list(ctx.pairing_check(g1, g1_inf, g2, None, 3)) == [2, 2]         # the same coordinates without the flags


# ---- 11. NULL flag arrays ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_null_flag_arrays_mean_no_point_is_infinity(pool, native, curve):
    ctx = pool.kzg._context()
    delta = pool.a[0] * pool.b[1] + pool.a[1] * pool.b[2]
    eqs = [pool.equation(0, 1), pool.equation(1, 2, holds=False), [(pool.A[0], pool.B[1]), (pool.A[1], pool.B[2])],
           pool.equation(3, 3)]
    g1, g1_inf, g2, g2_inf = pool.arrays(eqs)
    assert not g1_inf.any() and not g2_inf.any()
    # the call before leaves a set flag at every position of the context's buffer: all pairs skipped, every product one
    ones = np.ones(8, dtype=np.uint8)
    gt, status = ctx.pairing_product(g1, ones, g2, ones, 2)
    one = gt_power(pool, native, curve, 0)
    assert list(status) == [0, 0, 0, 0] and gt_tuples(native, curve, gt) == [one] * 4
    want = [one, gt_power(pool, native, curve, -1), gt_power(pool, native, curve, delta), one]
    for f1, f2 in ((g1_inf, g2_inf), (None, g2_inf), (g1_inf, None), (None, None)):
        gt, status = ctx.pairing_product(g1, f1, g2, f2, 2)
        which = (f1 is None, f2 is None)
        assert list(status) == [0, 1, 1, 0], which
        assert gt_tuples(native, curve, gt) == want, which
    ctx.pairing_check(g1, ones, g2, ones, 2)                                   # the layout without the values
    for f1, f2 in ((None, g2_inf), (g1_inf, None), (None, None)):
        assert list(ctx.pairing_check(g1, f1, g2, f2, 2)) == [0, 1, 1, 0], (f1 is None, f2 is None)


# ---- 12. one buffer, layouts that differ --------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_the_context_buffer_is_reused_across_layouts(pool, native, curve):
    """kzg_pairing_product puts the out_gt region between the flags and the statuses, so every call of this sequence
    finds the regions of the one before at other offsets"""
    kzg = pool.kzg
    rng = random.Random(13 + len(curve))
    m = COMPUTE_UNITS + 1
    pattern = [rng.randrange(2) == 0 for _ in range(m)]
    eqs = [pool.equation(rng.randrange(POOL), rng.randrange(POOL), holds=h) for h in pattern]
    assert statuses(pool, eqs) == [0 if h else 1 for h in pattern]
    S = 0xfeed_0000_0000_0001
    values, status = products(pool, native, curve, [chain(pool, MAX_PAIRS, delta=S)])
    assert status == [1] and values == [gt_power(pool, native, curve, S)]
    delta = pool.a[4] * pool.b[5] + pool.a[6] * pool.b[7]
    three = [pool.equation(2, 5), pool.equation(5, 2, holds=False), [(pool.A[4], pool.B[5]), (pool.A[6], pool.B[7])]]
    values, status = products(pool, native, curve, three)
    assert status == [0, 1, 1]
    assert values == [gt_power(pool, native, curve, d) for d in (0, -1, delta)]
    singles = [[(kzg.Z1 if e % 5 == 0 else pool.A[e % POOL], pool.B[(e // POOL) % POOL])] for e in range(64)]
    assert statuses(pool, singles) == [0 if e % 5 == 0 else 1 for e in range(64)]


# ---- 13. status 2 is about every FINITE point of the equation --------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_a_malformed_finite_point_beside_an_infinite_partner_gives_status_2(pool, native, curve):
    kzg, L = pool.kzg, pool.L
    ctx = kzg._context()
    delta = pool.a[0] * pool.b[1] + pool.a[1] * pool.b[2]
    eqs = [pool.equation(0, 1),
           [(kzg.Z1, pool.B[0]), (pool.A[1], pool.B[1])],                    # pair 0: G1 infinity beside a finite G2
           [(pool.A[0], pool.B[1]), (pool.A[1], pool.B[2])],
           [(kzg.Z1, pool.B[3]), (kzg.Z1, kzg.Z2)],                          # nothing live, one finite G2
           [(pool.A[2], kzg.Z2), (kzg.Z1, kzg.Z2)]]                          # nothing live, one finite G1
    g1, g1_inf, g2, g2_inf = pool.arrays(eqs)
    values = [gt_power(pool, native, curve, d) for d in (0, pool.a[1] * pool.b[1], delta, 0, 0)]
    gt, status = ctx.pairing_product(g1, g1_inf, g2, g2_inf, 2)
    assert list(status) == [0, 1, 1, 0, 0] and gt_tuples(native, curve, gt) == values
    g1, g2 = g1.copy(), g2.copy()
    g2[2 * 1 + 0, 2 * L] ^= np.uint64(1)                                     # that G2 off the twist
    g2[2 * 3 + 0, 2 * L] ^= np.uint64(1)
    g1[2 * 4 + 0, L] ^= np.uint64(1)                                         # that G1 off the curve
    want = [0, 2, 1, 2, 2]
    assert list(ctx.pairing_check(g1, g1_inf, g2, g2_inf, 2)) == want
    gt, status = ctx.pairing_product(g1, g1_inf, g2, g2_inf, 2)
    assert list(status) == want
    got = gt_tuples(native, curve, gt)
    assert got[0] == values[0] and got[2] == values[2]                        # the neighbours are untouched
    for e in (1, 3, 4):
        assert not gt[e].any(), e                                             # zeros where the status is 2


# ---- 14. a G2 point outside the subgroup --------------------------------------------------------------------------------
def sqrt_fp2(a, p):
    """a square root of a = a0 + a1 i in Fp[i]/(i^2 + 1), p = 3 (mod 4), or None when a is not a square: with n a root
    of the norm a0^2 + a1^2, x0^2 = (a0 + n) / 2 or (a0 - n) / 2 (their product -a1^2 / 4 is not a square, so it is one
    of the two when a1 != 0) and x1 = a1 / (2 x0)"""
    a0, a1 = a[0] % p, a[1] % p
    if a1 == 0:
        s = C.sqrt_fp(a0, p)
        return (s, 0) if s is not None else (0, C.sqrt_fp(-a0 % p, p))
    n = C.sqrt_fp((a0 * a0 + a1 * a1) % p, p)
    if n is None:
        return None
    for s in (n, p - n):
        x0 = C.sqrt_fp((a0 + s) * pow(2, -1, p) % p, p)
        if x0:
            return (x0, a1 * pow(2 * x0, -1, p) % p)
    return None


def first_twist_point(cv):
    """the first x = (3 + j) + i, j = 0, 1, ..., with x^3 + b' a square in Fp2, and a root y"""
    F2 = C._Fp2(cv.p)
    for j in range(64):
        x = (3 + j, 1)
        rhs = F2.add(F2.mul(F2.mul(x, x), x), cv.b2)
        y = sqrt_fp2(rhs, cv.p)
        if y is not None:
            assert F2.mul(y, y) == rhs
            return (x, y, (1, 0))
    raise AssertionError("no twist point among 64 abscissae")


@pytest.mark.parametrize("curve", CURVES)
def test_a_g2_point_outside_the_subgroup_gives_the_host_value(pool, native, curve):
    kzg, cv = pool.kzg, pool.cv
    K, c = PR._CURVES[curve].K, native.PAIRING_GT_MULTIPLE[curve]
    Q = first_twist_point(cv)
    assert C.on_curve_g2(Q, cv) and not kzg._g2.is_inf(kzg._g2.multiply(Q, cv.r))
    host = list(kzg.pairing(Q, pool.A[0]))
    eqs = [pool.equation(0, 1), [(pool.A[0], Q), (kzg.Z1, kzg.G2)], pool.equation(1, 0, holds=False)]
    values, status = products(pool, native, curve, eqs)
    assert status == [0, 0 if host == K.one else 1, 1]
    assert values == [gt_power(pool, native, curve, 0), tuple(K.pow(host, c)), gt_power(pool, native, curve, -1)]
    assert kzg.pairing_product([(pool.A[0], Q)]) == tuple(K.pow(host, c))


# ---- 15. the verifiers where L or R is the point at infinity ------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_verify_points_at_infinity_agrees_between_host_and_device_pairings(kzgs, curve):
    kzg = kzgs[curve]
    r = kzg.curve_order
    rng = random.Random(15)
    n = 8
    lk, rk = kzg.setup_lagrange(n, tau=TAU)
    idx = list(range(n))
    zs = [rng.randrange(r) for _ in range(n)]

    def claims(values):
        comms = kzg.commit_evaluations(lk, values)
        ys = [int(y) for y in kzg.evaluate_evaluations_each(lk, values, zs)]
        proofs = [kzg.open_evaluations(lk, [values[j]], zs[j], 1) for j in range(n)]
        return comms, ys, proofs

    def verdicts(comms, ys, proofs):
        return [kzg.verify_points(rk, comms, idx, zs, ys, proofs, r=77, pairing=where) for where in ("device", "host")]

    # every polynomial zero: commitments, values and proofs are O, 0, O -- L = R = O, both pairs skipped
    comms, ys, proofs = claims([[0] * n for _ in range(n)])
    assert all(kzg._g1.is_inf(pt) for pt in list(comms) + list(proofs)) and ys == [0] * n
    assert verdicts(comms, ys, proofs) == [True, True]
    ys[0] = 1                                                                   # L != O, R = O: one live pair
    assert verdicts(comms, ys, proofs) == [False, False]
    # one polynomial among zero ones: L != O and R != O from a single claim
    values = [[0] * n for _ in range(n)]
    values[3] = [rng.randrange(r) for _ in range(n)]
    comms, ys, proofs = claims(values)
    assert [kzg._g1.is_inf(pt) for pt in comms] == [j != 3 for j in range(n)]
    assert verdicts(comms, ys, proofs) == [True, True]
    ys[3] = (ys[3] + 1) % r
    assert verdicts(comms, ys, proofs) == [False, False]

"""The two folded points of bulk verification as multiples of the generator (a plain module, no fixtures).

The fold of kzg_verify_cosets / kzg_verify_points is linear in its points.  With proofs and commitments taken from a
generated key -- point e is [tau^e] G -- L and R are known multiples of G, for ANY values, indices and weights: the
claims need not be honest.  The scalars are computed here in Python integers; a case costs two scalar multiplications
of the C oracle, whatever its size.  That pins the weights themselves, which the relation L == tau^l R cannot: every
honest claim satisfies it on its own, so it holds for any weights the kernels agree on.

    r_k = rho^(k+1),  h_k = w^(i_k),  zeta = w^(N/l)
    Rs = sum_k r_k tau^(e_k)
    Ls = sum_j W_j tau^(f_j)  -  sum_j T_j tau^j  +  sum_k r_k w^(i_k l) tau^(e_k)        (cosets)
    Ls = sum_j W_j tau^(f_j)  -  sum_k r_k y_k    +  sum_k r_k z_k tau^(e_k)              (points)
    W_j = the sum of r_k over the claims of commitment j,  T_j = sum_k r_k h_k^-j l^-1 sum_t y_k[t] zeta^(-jt)

An exponent None stands for the point at infinity and contributes 0.  tests/test_verify_scalars_host.py pins these
formulas to the restatements over the group law (verify_restated.restated_LR, points_restated.restated_LR_points), and
the shapes below to the launch plan of csrc/ver_layout.h; tests/test_verify_exact_gpu.py compares the library with them
limb for limb.  Nothing here calls the library."""
import os
import random
import re
from collections import namedtuple

import numpy as np

from oracle import c_oracle
from oracle import py_oracle as O

CURVES = ["bls12_381", "bn254"]
_CURVE_OF_R = {O.curve(c).r: c for c in CURVES}


# ---- values: uint64[..., 4] little-endian limbs <-> Python integers --------------------------------------------------
def limbs_to_ints(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[o:o + 32], "little") for o in range(0, len(raw), 32)]


def ints_to_limbs(values):
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).copy()


def random_reduced(rng, shape, r):
    """uniform below 2^254-ish and reduced: random limbs, the top one below the modulus' top limb (rng: numpy)"""
    raw = rng.integers(0, 1 << 63, size=(*shape, 4), dtype=np.uint64)
    raw[..., 3] %= np.uint64(r >> 192)
    return raw


# ---- the scalars -------------------------------------------------------------------------------------------------
def cell_interpolate(cell, h, zeta, r):
    """verify_restated.coset_interpolate through the C oracle's inverse transform: rho_j = h^-j (l^-1 sum_t y_t
    zeta^(-jt)).  cell: uint64[l, 4] (left unchanged) -> l integers"""
    l = cell.shape[0]
    c = limbs_to_ints(c_oracle.fft(_CURVE_OF_R[r], np.array(cell, dtype=np.uint64), zeta, inverse=True)) if l > 1 \
        else limbs_to_ints(cell)
    hi, f, out = pow(h, -1, r), 1, []
    for j in range(l):
        out.append(c[j] * f % r)
        f = f * hi % r
    return out


def _tau_pow(e, tau, r):
    return 0 if e is None else pow(tau, e, r)


def _weights(K, rho, r):
    out, rk = [], 1
    for _ in range(K):
        rk = rk * rho % r
        out.append(rk)
    return out


def coset_fold_scalars(e_comm, comm_idx, coset_idx, values, e_proof, l, N, w, rho, tau, r):
    """(Ls, Rs) of K coset claims: commitment j is [tau^(e_comm[j])] G, proof k is [tau^(e_proof[k])] G (None:
    infinity), values uint64[K, l, 4] in natural order"""
    K = len(e_proof)
    values = np.ascontiguousarray(values, dtype=np.uint64).reshape(K, l, 4)
    zeta = pow(w, N // l, r)
    tp = {e: _tau_pow(e, tau, r) for e in set(e_proof) | set(e_comm)}
    W, T = [0] * len(e_comm), [0] * l
    Rs = Ss = 0
    flat = limbs_to_ints(values) if l == 1 else None
    a_of = {}                                              # a_k = w^(i_k l) by coset index
    for k, rk in enumerate(_weights(K, rho, r)):
        c, i = int(comm_idx[k]), int(coset_idx[k])
        W[c] += rk
        if l == 1:
            T[0] += rk * flat[k]
        else:
            for j, coef in enumerate(cell_interpolate(values[k], pow(w, i, r), zeta, r)):
                T[j] += rk * coef % r
        if i not in a_of:
            a_of[i] = pow(w, i * l, r)
        t = rk * tp[e_proof[k]] % r
        Rs += t
        Ss += t * a_of[i]
    Ls = sum(Wj % r * tp[f] for Wj, f in zip(W, e_comm)) - sum(Tj % r * pow(tau, j, r) for j, Tj in enumerate(T)) + Ss
    return Ls % r, Rs % r


def point_fold_scalars(e_comm, comm_idx, zs, ys, e_proof, rho, tau, r):
    """(Ls, Rs) of K claims at arbitrary points: zs, ys uint64[K, 4] or lists of integers"""
    K = len(e_proof)
    zs = limbs_to_ints(zs) if isinstance(zs, np.ndarray) else [int(z) % r for z in zs]
    ys = limbs_to_ints(ys) if isinstance(ys, np.ndarray) else [int(y) % r for y in ys]
    tp = {e: _tau_pow(e, tau, r) for e in set(e_proof) | set(e_comm)}
    W = [0] * len(e_comm)
    Rs = Ss = Ys = 0
    for k, rk in enumerate(_weights(K, rho, r)):
        W[int(comm_idx[k])] += rk
        Ys += rk * ys[k]
        t = rk * tp[e_proof[k]] % r
        Rs += t
        Ss += t * zs[k]
    return (sum(Wj % r * tp[f] for Wj, f in zip(W, e_comm)) - Ys + Ss) % r, Rs % r


def expected(curve, G_xy, scalar):
    """[scalar] G in the C layout: (xy uint64[2 * fp_limbs], inf); scalar 0: the point at infinity, coordinates zero"""
    if scalar == 0:
        return np.zeros_like(np.asarray(G_xy, dtype=np.uint64)), 1
    xy, inf = c_oracle.g1_mul(curve, np.ascontiguousarray(G_xy, dtype=np.uint64), scalar)
    assert not inf                                         # the group has prime order r and 0 < scalar < r
    return xy, 0


def key_points(kxy, exps):
    """the points [tau^e] G of a key exported as kxy, in the C layout: (xy, inf); None: infinity, coordinates zero"""
    xy = np.zeros((len(exps), kxy.shape[1]), dtype=np.uint64)
    inf = np.zeros(len(exps), dtype=np.uint8)
    for k, e in enumerate(exps):
        if e is None:
            inf[k] = 1
        else:
            xy[k] = kxy[e]
    return xy, inf


def draw_proofs(rng, K, key_n):
    """K exponents with repetition (rng: random.Random): two proofs at infinity and one proof repeated far apart when
    K >= 4; below that what fits -- K = 3: [e, None, None] shuffled, K = 2: one infinity, K = 1: a finite proof"""
    e = [rng.randrange(key_n) for _ in range(K)]
    slots = rng.sample(range(K), min(K, 4))
    for s in slots[:min(2, K - 1)]:
        e[s] = None
    if K >= 4:
        e[slots[3]] = e[slots[2]]
    return e


# ---- the shapes of tests/test_verify_exact_gpu.py --------------------------------------------------------------------
# The smallest shapes at which each launch regime of kzg_verify_cosets / kzg_verify_points exists.  `reach` names the
# fields of the launch plan (VerPlan, csrc/ver_layout.h) or of the power table that the row is there for; the host
# test checks them against the plan the shim prints, so a changed constant fails the table instead of silently losing
# the regime.  Keys of reach: ntiles, tail (the last tile is short), strided (more tiles than workgroups), lds_bytes,
# m_vs_sum (-1, 0, 1: M below, at, above sum_threads), shares, slice_bits, slices, rho_hi / w_hi (the second level of
# the rho / w table is read: an exponent >= 2048).
KEY_N = 4096                                             # the generated key proofs and commitments are drawn from
W_LO = 2048                                              # case A (l = 1) keeps its coset indices, the exponents of w, below
Case = namedtuple("Case", "group log_l log_N K n_comm reach curves")


def case_id(c):
    return f"{c.group}-l{1 << c.log_l}-N2^{c.log_N}-K{c.K}-c{c.n_comm}"


def _tile_cases():
    out = []
    for log_l in range(1, 9):
        l = 1 << log_l
        ks = [1, 256 // l, 256 // l + 1] + [k for k in (384 // l + 1, 384 // l) if 256 < k * l < 512][:1]
        for K in sorted(set(ks)):
            M = K * l
            out.append(Case("C", log_l, 13, K, 3, dict(ntiles=-(-M // 256), tail=M % 256 != 0, strided=False,
                                                       lds_bytes=8192), CURVES))
    for log_l in (9, 10, 11, 12):
        for K in (1, 3):
            out.append(Case("C", log_l, 13, K, 3, dict(ntiles=K, tail=False, strided=False, lds_bytes=32 << log_l),
                            CURVES))
    for K, side in ((511, -1), (512, 0), (513, 1)):
        out.append(Case("C", 6, 13, K, 3, dict(m_vs_sum=side, ntiles=-(-K // 4), tail=K % 4 != 0), CURVES))
    return out


A_CASES = [Case("A", 0, 13, K, 3, dict(rho_hi=K >= 2048, w_hi=False, ntiles=-(-K // 256)), CURVES)
           for K in (1, 2047, 2048, 2049, 4095, 4096, 4097)]
A_RHO_K = 2049                                           # and rho = 0, 1, r - 1 at this K
B_CASES = [Case("B", log_l, log_N, 8, 3, dict(w_hi=True, ntiles=-(-(8 << log_l) // max(256, 1 << log_l))), CURVES)
           for log_l, log_N in ((1, 12), (0, 21), (4, 21), (12, 21))]
C_CASES = _tile_cases()
D_CASES = [Case("D", 8, 13, 4097, 3, dict(ntiles=4097, strided=True, tail=False), ["bls12_381"])]
E_CASES = [Case("E", 0, 13, 20000, n_comm, dict(shares=64 if n_comm < 64 else 1), CURVES)
           for n_comm in (1, 2, 63, 64, 65, 300)]
F_CASES = [Case("F", 0, 18, (1 << 18) - 1, 3, dict(slice_bits=15, slices=17, rho_hi=True), CURVES),
           Case("F", 0, 18, 1 << 18, 3, dict(slice_bits=19, slices=14, rho_hi=True), CURVES)]
G_KS = [2047, 2048, 2049, 16384, 16385, 65792]           # kzg_verify_points, n_comm = 3
H_CASES = [c for c in C_CASES if c.log_l == 6 and c.K in (5, 7)] + B_CASES[:1] + B_CASES[2:3]
COSET_CASES = A_CASES + B_CASES + C_CASES + D_CASES + E_CASES + F_CASES

# kzg_verify_points (verify_points.hip): lanes per workgroup, workgroups per ladder launch, threads of the weights kernel
VPT_TB, VPT_LAUNCH_BLOCKS, VPT_WEIGHT_THREADS = 256, 512, 1 << 14


def w_table_indices(c, rng):
    """case B: coset indices 0, 1, C/2, C - 1, the index with i l = 2048 and its neighbours (where l divides 2048 and
    they exist; random ones otherwise), one random index"""
    C, l = 1 << (c.log_N - c.log_l), 1 << c.log_l
    idx = [0, 1, C // 2, C - 1]
    i0 = 2048 // l
    idx += [i0 - 1, i0, i0 + 1] if 2048 % l == 0 and i0 + 1 < C else [rng.randrange(C) for _ in range(3)]
    return idx + [rng.randrange(C)]


def commitment_cells(c, rng):
    """case E: the commitment index of every cell, shuffled.  n_comm = 1: all 20,000 (not a multiple of 64, above
    16,384) on the one commitment; n_comm = 2: 19,999 and exactly one; otherwise commitment 0 has no cell, 1 exactly
    one, 2 has 16,421 (16,384 + 37) and the rest fall at random on commitments 3 and up"""
    K, n = c.K, c.n_comm
    if n == 1:
        return [0] * K
    if n == 2:
        ci = [0] * (K - 1) + [1]
    else:
        ci = [1] + [2] * 16421
        ci += [rng.randrange(3, n) for _ in range(K - len(ci))]
    rng.shuffle(ci)
    return ci


def infinite_commitments(c):
    """case E: two commitments at infinity where there are more than two -- one that has cells, and the last"""
    return {3, c.n_comm - 1} if c.n_comm > 4 else set()


def draw_case(c, cv, seed):
    """The inputs of one coset case in Python terms: (e_comm, comm_idx, coset_idx, values, e_proof, rho).  Proofs and
    commitments by their exponents in the key; values uint64[K, l, 4], random and reduced"""
    r = cv.r
    rng = random.Random(f"{seed}-{case_id(c)}")
    K, l, C = c.K, 1 << c.log_l, 1 << (c.log_N - c.log_l)
    e_proof = draw_proofs(rng, K, KEY_N)
    e_comm = [rng.randrange(KEY_N) for _ in range(c.n_comm)]
    if c.group == "E":
        comm_idx = commitment_cells(c, rng)
        for j in infinite_commitments(c):
            e_comm[j] = None
    else:
        comm_idx = [rng.randrange(c.n_comm) for _ in range(K)]
    if c.group == "B":
        coset_idx = w_table_indices(c, rng)
    else:                                                # A: the w table's first level alone, so that A is the rho table's
        coset_idx = [rng.randrange(min(C, W_LO) if c.group == "A" else C) for _ in range(K)]
    values = random_reduced(np.random.default_rng(rng.randrange(1 << 32)), (K, l), r)
    rho = r - 1 - rng.randrange(1 << 64) if c.group == "F" else rng.randrange(2, r)       # F: the top bits are set
    return e_comm, comm_idx, coset_idx, values, e_proof, rho


# ---- constants of the library the table depends on, read from its sources -----------------------------------------
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kzg_snark_amd", "csrc")


def source_constant(filename, pattern):
    m = re.search(pattern, open(os.path.join(_CSRC, filename)).read())
    assert m, f"{filename}: {pattern} not found"
    return int(m.group(1))

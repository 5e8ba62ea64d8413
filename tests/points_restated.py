"""Bulk verification at arbitrary points restated in plain Python over the oracle's group law (a plain module, no
fixtures): the two G1 points (L, R) that kzg_verify_points returns.  The CPU tests pin this restatement to the pairing
equation through the trapdoor (L == tau R); the GPU tests compare the library's points with it coordinate for
coordinate."""
from oracle import py_oracle as O
from restated import g1_mul


def restated_LR_points(commitments, comm_idx, zs, ys, proofs, rho, cv):
    """L = sum_j (sum_(k: c_k = j) r_k) C[j] - (sum_k r_k y_k) G1 + sum_k (r_k z_k) pi_k,  R = sum_k r_k pi_k,
    r_k = rho^(k+1)"""
    r = cv.r
    weights, ysum = [0] * len(commitments), 0
    L, R = O.Z1(), O.Z1()
    rk = 1
    for c, z, y, pi in zip(comm_idx, zs, ys, proofs):
        rk = rk * rho % r
        weights[c] = (weights[c] + rk) % r
        ysum = (ysum + rk * (int(y) % r)) % r
        L = O.add(L, g1_mul(pi, rk * (int(z) % r) % r, cv), cv)
        R = O.add(R, g1_mul(pi, rk, cv), cv)
    for C, wt in zip(commitments, weights):
        L = O.add(L, g1_mul(C, wt, cv), cv)
    L = O.add(L, O.neg(g1_mul(O.from_affine(cv.g1), ysum, cv), cv), cv)
    return L, R

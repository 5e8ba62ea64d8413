"""Bulk verification restated in plain Python over the oracle's group law (a plain module, no fixtures): the two G1
points (L, R) that kzg_verify_cosets returns, the claims an honest prover makes, and the slice identity its MSM route
rests on.  The CPU tests pin this restatement to the pairing equation through the trapdoor (L == tau^l R); the GPU
tests compare the library's points with it coordinate for coordinate."""
from oracle import py_oracle as O
from restated import g1_mul


def coset_divide(coeffs, l, a, r):
    """(quotient, remainder) of p by X^l - a: S_t = c_t + a S_(t+l), q_t = S_(t+l), rho_j = S_j"""
    c = [int(x) % r for x in coeffs]
    S = c + [0] * l
    for t in range(len(c) - 1, -1, -1):
        S[t] = (c[t] + a * S[t + l]) % r
    return [S[t + l] for t in range(max(len(c) - l, 0))], [S[j] for j in range(l)]


def coset_interpolate(values, h, zeta, r):
    """rho_j = h^-j l^-1 sum_t y_t zeta^(-jt)"""
    l = len(values)
    zi, hi, li = pow(zeta, -1, r), pow(h, -1, r), pow(l, -1, r)
    return [sum(y * pow(zi, j * t, r) for t, y in enumerate(values)) * li * pow(hi, j, r) % r for j in range(l)]


def honest_cell(ck, coeffs, i, l, N, w, cv):
    """(values, proof) of coset i of {w^t, t < N} for the polynomial `coeffs`: y[t] = p(w^(i + t N/l)), the proof the
    oracle's commitment of (p - rho) / (X^l - w^(i l))"""
    r = cv.r
    values = [O.poly_eval(coeffs, pow(w, i + t * (N // l), r), r) for t in range(l)]
    q, _ = coset_divide(coeffs, l, pow(w, i * l, r), r)
    return values, O.commit(ck, [q], cv)[0]


def restated_LR(ck, commitments, comm_idx, coset_idx, values, proofs, l, N, w, rho, cv):
    """L = sum_j (sum_(k: c_k = j) r_k) C[j] - [(sum_k r_k I_k)(tau)] G1 + sum_k (r_k a_k) pi_k,  R = sum_k r_k pi_k,
    r_k = rho^(k+1), a_k = w^(i_k l), I_k interpolated from the values of cell k"""
    r = cv.r
    zeta = pow(w, N // l, r)
    weights, T = [0] * len(commitments), [0] * l
    L, R = O.Z1(), O.Z1()
    rk = 1
    for k, (c, i, ys, pi) in enumerate(zip(comm_idx, coset_idx, values, proofs)):
        rk = rk * rho % r
        weights[c] = (weights[c] + rk) % r
        for j, coef in enumerate(coset_interpolate([int(y) % r for y in ys], pow(w, i, r), zeta, r)):
            T[j] = (T[j] + rk * coef) % r
        L = O.add(L, g1_mul(pi, rk * pow(w, i * l, r), cv), cv)
        R = O.add(R, g1_mul(pi, rk, cv), cv)
    for C, wt in zip(commitments, weights):
        L = O.add(L, g1_mul(C, wt, cv), cv)
    for j, coef in enumerate(T):
        L = O.add(L, O.neg(g1_mul(ck[j], coef, cv), cv), cv)
    return L, R


def slices(scalar, win_bits, total_bits=255):
    """the scalar cut into pieces of win_bits - 1 bits, lowest first: what each proof MSM's slice vectors hold"""
    sb = win_bits - 1
    return [(scalar >> (s * sb)) & ((1 << sb) - 1) for s in range((total_bits + sb - 1) // sb)]

"""The Shplonk opening (Boneh-Drake-Fisch-Gabizon 2020, second scheme) restated in plain Python (a
plain module, no fixtures): integers mod r for the polynomials, the oracle's group law for the points.  The library
computes the first proof point as a weighted sum of single-point quotients; this restatement does NOT: it divides
every f_i - r_i by Z_(S_i) by long division, and L by (X - zeta).  Commitments come from a known tau as [p(tau)] G1.
The CPU tests pin the restatement to the check equation through the trapdoor; the GPU tests compare the library's
quotients and points with it, value for value."""
from collections import namedtuple

from oracle import py_oracle as O
from restated import g1_mul


def poly_add_scaled(a, b, s, r):
    """a + s b"""
    out = [0] * max(len(a), len(b))
    for i, c in enumerate(a):
        out[i] = c % r
    for i, c in enumerate(b):
        out[i] = (out[i] + s * c) % r
    return out


def vanishing(points, r):
    """the coefficients of Z_S = prod_(z in S) (X - z)"""
    c = [1]
    for z in points:
        c = [((c[i - 1] if i else 0) - z * (c[i] if i < len(c) else 0)) % r for i in range(len(c) + 1)]
    return c


def vanishing_at(points, x, r):
    acc = 1
    for z in points:
        acc = acc * (x - z) % r
    return acc


def poly_divmod(a, d, r):
    """long division by a monic d: (quotient, remainder)"""
    assert d[-1] == 1
    rem = [c % r for c in a]
    q = [0] * max(len(a) - len(d) + 1, 0)
    for i in range(len(q) - 1, -1, -1):
        c = rem[i + len(d) - 1]
        q[i] = c
        for j, dj in enumerate(d):
            rem[i + j] = (rem[i + j] - c * dj) % r
    return q, rem[:len(d) - 1]


def interpolate(points, values, r):
    """the coefficients of the polynomial of degree < len(points) through (points[j], values[j]): Lagrange's formula"""
    out = [0] * len(points)
    for z, v in zip(points, values):
        others = [m for m in points if m != z]
        scale = v * pow(vanishing_at(others, z, r), -1, r) % r
        out = poly_add_scaled(out, vanishing(others, r), scale, r)
    return out


def union(sets):
    """the distinct points in order of first appearance"""
    return list(dict.fromkeys(z for S in sets for z in S))


def quotient_points(polys, points, weights, r):
    """what kzg_open_points commits: sum_j (c_j - c_j(z_j)) / (X - z_j), c_j = sum_i weights[i][j] polys[i] -- every
    combination divided on its own (points may repeat, z = 0 included).  n - 1 coefficients, n = the longest length."""
    n = max((len(p) for p in polys), default=0)
    out = [0] * max(n - 1, 0)
    for j, z in enumerate(points):
        comb = []
        for p, row in zip(polys, weights):
            comb = poly_add_scaled(comb, p, row[j] % r, r)
        q, _ = O.poly_divide_linear(comb, z % r, r)
        out = poly_add_scaled(out, q, 1, r)
    return out


Multi = namedtuple("Multi", "T evaluations q W L q2 W2")


def restate_open_multi(polys, sets, gamma, zeta, tau, cv):
    """the prover.  q = sum_i gamma^(i+1) (f_i - r_i) / Z_(S_i) and
    L = sum_i gamma^(i+1) Z_(T\\S_i)(zeta) (f_i - r_i(zeta)) - Z_T(zeta) q, q2 = L / (X - zeta): both divisions exact."""
    r = cv.r
    T = union(sets)
    evaluations = [[O.poly_eval(f, z, r) for z in S] for f, S in zip(polys, sets)]
    n = max((len(f) for f in polys), default=0)
    q, L, g = [0] * max(n - 1, 0), [0] * n, 1
    for f, S, vals in zip(polys, sets, evaluations):
        g = g * gamma % r
        r_i = interpolate(S, vals, r)
        quot, rem = poly_divmod(poly_add_scaled(f, r_i, -1, r), vanishing(S, r), r)
        assert not any(rem)
        q = poly_add_scaled(q, quot, g, r)
        scale = g * vanishing_at([z for z in T if z not in S], zeta, r) % r
        L = poly_add_scaled(L, poly_add_scaled(f, [O.poly_eval(r_i, zeta, r)], -1, r), scale, r)
    L = poly_add_scaled(L, q, -vanishing_at(T, zeta, r), r)
    q2, rem = poly_divmod(L, [-zeta % r, 1], r)
    assert not any(rem)
    return Multi(T, evaluations, q, O.commit_trapdoor(q, tau, cv), L, q2, O.commit_trapdoor(q2, tau, cv))


def multi_F(commitments, sets, evaluations, W, gamma, zeta, cv):
    """the verifier's F = sum_i gamma^(i+1) Z_(T\\S_i)(zeta) (C_i - [r_i(zeta)] G1) - Z_T(zeta) W"""
    r = cv.r
    T = union(sets)
    F, g = O.Z1(), 1
    G1 = O.from_affine(cv.g1)
    for C, S, vals in zip(commitments, sets, evaluations):
        g = g * gamma % r
        scale = g * vanishing_at([z for z in T if z not in S], zeta, r) % r
        r_zeta = O.poly_eval(interpolate(S, [v % r for v in vals], r), zeta, r)
        F = O.add(F, g1_mul(O.add(C, O.neg(g1_mul(G1, r_zeta, cv), cv), cv), scale, cv), cv)
    return O.add(F, O.neg(g1_mul(W, vanishing_at(T, zeta, r), cv), cv), cv)


def check_in_the_exponent(commitments, sets, evaluations, W, W2, gamma, zeta, tau, cv):
    """e(F + zeta W', G2) = e(W', tau G2) with tau known: F + zeta W' == tau W'"""
    F = multi_F(commitments, sets, evaluations, W, gamma, zeta, cv)
    return O.eq(O.add(F, g1_mul(W2, zeta, cv), cv), g1_mul(W2, tau, cv), cv)

"""Coset recovery restated in plain Python integers (a plain module, no fixtures): the five steps of DESIGN.md 4.8 over
the oracle's transforms, the product tree with its wrap repair, direct Lagrange interpolation as the independent
statement, and the helpers the CPU and GPU test files share."""
import random

from oracle import py_oracle as O

GENERATOR = {"bn254": 5, "bls12_381": 7}          # the shift s of step 3: a generator of Fr*, so s^N != 1


def poly_mul(a, b, r):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % r
    return out


def cyclic_mul(a, b, T, r):
    """a b mod (X^T - 1): what a size-T transform, a pointwise product and the inverse transform give"""
    out = [0] * T
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[(i + j) % T] = (out[(i + j) % T] + x * y) % r
    return out


def pair_product(a, b, d, r):
    """The product of two monic-or-one nodes of capacity d (degree <= d, coefficient lists without trailing zeros) at
    transform size T = 2d.  Only two FULL nodes reach degree T: the leading 1 wraps onto position 0 and is moved back."""
    T = 2 * d
    assert len(a) - 1 <= d and len(b) - 1 <= d
    c = cyclic_mul(a, b, T, r)
    if len(a) - 1 == d and len(b) - 1 == d:
        c[0] = (c[0] - 1) % r
        c.append(1)
    else:
        c = c[:len(a) + len(b) - 1]
    return c


def vanishing_tree(roots, leaf, r):
    """prod (Y - root) by the tree of the device: leaves of `leaf` linear factors (the last ones padded with the
    constant 1, never with roots), then pairs at transform size twice the capacity"""
    count = max(1, -(-len(roots) // leaf))
    nodes = []
    for q in range(count):
        c = [1]
        for x in roots[q * leaf:(q + 1) * leaf]:
            c = poly_mul(c, [(-x) % r, 1], r)
        nodes.append(c)
    d = leaf
    while len(nodes) > 1:
        if len(nodes) & 1:
            nodes.append([1])
        nodes = [pair_product(nodes[2 * j], nodes[2 * j + 1], d, r) for j in range(len(nodes) // 2)]
        d *= 2
    return nodes[0]


def recover(idx, cells, l, n, N, w, s, r, leaf=64):
    """cells[k] = the l values on coset idx[k]  ->  (all N coefficients of the interpolant through the given values,
    tail included; whether the tail n .. N-1 is zero)"""
    C = N // l
    u = pow(w, l, r)
    given = {i: k for k, i in enumerate(idx)}
    missing = [i for i in range(C) if i not in given]
    V = vanishing_tree([pow(u, i, r) for i in missing], leaf, r)                     # 1
    V = V + [0] * (C - len(V))
    Zw = O.fft_ff(V, u, r)
    EZ = [cells[given[t % C]][t // C] * Zw[t % C] % r if t % C in given else 0 for t in range(N)]   # 2
    pz = O.ifft_ff(EZ, w, r)
    pzs = O.fft_ff([c * pow(s, t, r) % r for t, c in enumerate(pz)], w, r)          # 3
    Zs = O.fft_ff([c * pow(s, l * j, r) % r for j, c in enumerate(V)], u, r)
    assert all(Zs)
    ps = [v * pow(Zs[t % C], -1, r) % r for t, v in enumerate(pzs)]                  # 4
    p = [c * pow(s, -t, r) % r for t, c in enumerate(O.ifft_ff(ps, w, r))]
    return p, not any(p[n:])                                                         # 5


def lagrange(xs, ys, r):
    """coefficients (len(xs) of them) of the interpolant through (xs, ys), by the definition"""
    out = [0] * len(xs)
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        num, den = [1], 1
        for j, xj in enumerate(xs):
            if j != i:
                num = poly_mul(num, [(-xj) % r, 1], r)
                den = den * (xi - xj) % r
        f = yi * pow(den, -1, r) % r
        for t, c in enumerate(num):
            out[t] = (out[t] + c * f) % r
    return out


def coset_points(i, l, N, w, r):
    return [pow(w, i + k * (N // l), r) for k in range(l)]


def cells_of(evals, idx, l, N):
    """the cells of one polynomial from its N evaluations (natural order): cell k = values on coset idx[k]"""
    C = N // l
    return [[evals[i + k * C] for k in range(l)] for i in idx]


def index_set(rng, C, K):
    idx = rng.sample(range(C), K)
    rng.shuffle(idx)
    return idx


def rng_for(*key):
    return random.Random(repr(key))

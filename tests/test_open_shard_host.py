"""The plain-Python restatement of the sharded opening (tests/open_shard_restated.py) against the oracle's unsharded
opening, on the host: what the GPU tests of kzg_open_shard_begin / _finish compare the device with must itself be the
opening of kzg.py:122-159, rank by rank.  Exact integer work."""
import random

import pytest

from oracle import py_oracle as O
from open_shard_restated import derivative_at, restate_sharded_open

CURVES = ["bls12_381", "bn254"]
LENS = [61, 40, 0, 23, 61, 1]                     # ragged, one empty, two of the full length
# boundaries inside, exactly at and beyond polynomials' ends (23 | 40 | 61), one-coefficient ranks, an empty top rank
BOUNDS = [(0, 61), (0, 1, 61), (0, 23, 40, 61), (0, 7, 22, 24, 39, 41, 60, 62), (0, 30, 64, 70), (0, 60, 61, 62, 90),
          (0, 1, 2, 3, 100)]


def make_polys(rng, r, lens=LENS):
    polys = [[rng.randrange(r) for _ in range(m)] for m in lens]
    polys[0][-1] = r - 1                            # the longest ends in a non-zero coefficient
    if len(polys) > 4:
        polys[4][5:9] = [0, 0, r - 1, 0]
    return polys


def z_cases(rng, r):
    return [("random", rng.randrange(2, r - 1)), ("zero", 0), ("one", 1), ("minus_one", r - 1)]


@pytest.mark.parametrize("bounds", BOUNDS, ids=lambda b: "-".join(map(str, b)))
@pytest.mark.parametrize("curve", CURVES)
def test_restated_ranks_add_up_to_the_oracle_opening(curve, bounds):
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(1000 * len(bounds) + sum(bounds) + len(curve))
    polys = make_polys(rng, r)
    xi, tau = rng.randrange(1, r), rng.randrange(2, r - 1)
    G1 = O.from_affine(cv.g1)
    for name, z in z_cases(rng, r):
        assert z != tau
        w = restate_sharded_open(polys, xi, z, bounds, tau, r)
        comb = O.combine(polys, xi, r)
        assert w.c[:len(comb)] == comb and not any(w.c[len(comb):]), name
        assert w.S[0] == O.poly_eval(comb, z, r), name
        assert w.ev[0] == w.S[0], name
        # the quotient of kzg.py:154 is S_1, S_2, ...
        quot, pz = O.poly_divide_linear(comb, z, r)
        assert pz == w.S[0] and O.poly_normalize(w.S[1:]) == quot, name
        for g in range(len(bounds) - 1):
            lo, hi = bounds[g], bounds[g + 1]
            assert w.carry[g] == w.S[hi], (name, g)                       # what the exchange hands down is S_hi
            assert w.H[g] == O.poly_eval(w.c[lo:hi], z, r), (name, g)
            assert w.H[g] == (w.S[lo] - pow(z, hi - lo, r) * w.S[hi]) % r, (name, g)
            if g:
                assert w.ev[g] == w.S[lo], (name, g)
        total = sum(w.scalar) % r
        assert O.normalize(O.multiply(G1, total, cv), cv) == O.normalize(O.open_trapdoor(polys, z, xi, tau, cv), cv), name


@pytest.mark.parametrize("curve", CURVES)
def test_restated_ranks_at_the_trapdoor_itself(curve):
    """z = tau: (c(tau) - c(z)) / (tau - z) has no value, the sum over the suffix values has -- the derivative c'(tau)."""
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(77)
    polys = make_polys(rng, r)
    xi, tau = rng.randrange(1, r), rng.randrange(2, r - 1)
    for bounds in BOUNDS:
        w = restate_sharded_open(polys, xi, tau, bounds, tau, r)
        assert sum(w.scalar) % r == derivative_at(O.combine(polys, xi, r), tau, r), bounds
        for g in range(len(bounds) - 1):
            assert w.carry[g] == w.S[bounds[g + 1]], (bounds, g)


@pytest.mark.parametrize("curve", CURVES)
def test_restated_per_rank_scalars_are_the_quotient_slices(curve):
    """Rank by rank, not only in total: scalar_g is the value at tau of the quotient's coefficients this rank commits
    (S_1 .. S_(hi-1) against key points 0 .. on the first rank, S_lo .. S_(hi-1) against lo-1 .. on the others)."""
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(5)
    polys = make_polys(rng, r)
    xi, tau, z = rng.randrange(1, r), rng.randrange(2, r - 1), rng.randrange(r)
    for bounds in BOUNDS:
        w = restate_sharded_open(polys, xi, z, bounds, tau, r)
        quot, _ = O.poly_divide_linear(O.combine(polys, xi, r), z, r)
        quot = quot + [0] * (bounds[-1] - len(quot))
        for g in range(len(bounds) - 1):
            lo, hi = max(bounds[g], 1), bounds[g + 1]
            want = sum(quot[j - 1] * pow(tau, j - 1, r) for j in range(lo, hi)) % r
            assert w.scalar[g] == want, (bounds, g)


def test_restated_empty_and_all_zero_input():
    r = O.curve("bn254").r
    w = restate_sharded_open([[], [0, 0, 0]], 5, 7, (0, 2, 4), 11, r)
    assert w.H == [0, 0] and w.carry == [0, 0] and w.ev == [0, 0] and w.scalar == [0, 0] and w.S == [0] * 5

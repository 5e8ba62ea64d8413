"""kzg_snark_amd/plonk_rounds.py -- the round algebra the device and the vector-sharded prover share -- against the host
prover (plonk.Prover on dense polynomials, the oracle standing in for the engine), without a GPU.

The algebra object is tests/oracle_backends.OracleShardBackend (Python ints behind the [m, 4] tensors).  Ground truth is
the trace of plonk.Prover.prove with fixed blinders: its polynomials evaluated at the points in question with the
formulas of plonk/prover.py:243-316 written out on scalars here.  Sizes are the smallest at which every term is live:
the reference's 16-gate instance on BN254 with the blinders of tests/golden/plonk_proof_n16.json (4n = 64 coset
points) and an 8-gate synthetic circuit on BLS12-381 (32)."""
import json
import os
import random

import numpy as np
import pytest

import oracle_backends as OB
from oracle import plonk_oracle as P
from oracle import py_oracle as O
from test_plonk import fixture_instance, oracle_backed

CURVES = ("bn254", "bls12_381")
WIRES, SIGMAS = ("a", "b", "c"), ("S_sigma1", "S_sigma2", "S_sigma3")


class Case:
    """one circuit proved by the host prover: proving key, trace, and its polynomials as coefficient lists"""

    def __init__(self, curve):
        from kzg_snark_amd import plonk
        from kzg_snark_amd.field import GF, PolynomialRing
        self.curve, self.r = curve, O.curve(curve).r
        r = self.r
        if curve == "bn254":
            gp = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plonk_proof_n16.json")))
            circuit, tau, blinders = fixture_instance(), int(gp["tau"], 16), [int(v, 16) for v in gp["blinders"]]
        else:
            circuit, tau, blinders = plonk.synthetic_circuit(8, GF(r), seed=3), 0x7a75, list(range(101, 112))
        idx, prv = plonk.Indexer(curve), plonk.Prover(curve)
        idx.kzg = prv.kzg = oracle_backed(curve)
        with pytest.MonkeyPatch.context() as mp:         # the host prover's interpolation on the oracle (no GPU)
            mp.setattr(plonk, "fft_ff_interpolation", lambda values, g, F: PolynomialRing(F, "X")(
                O.fft_ff_interpolation([int(v) for v in values], int(g), F.p)))
            self.ipk, _ = idx.preprocess(*circuit[:6], tau=tau)
            self.trace = {}
            prv.prove(self.ipk, circuit[6], circuit[7], blinders=blinders, trace=self.trace)
        self.x, self.w = list(circuit[6]), list(circuit[7])
        sub = self.ipk["subgroups"]
        self.n, self.g, self.k1, self.k2 = sub["n"], int(sub["g"]), int(sub["k1"]), int(sub["k2"])
        self.Fq = idx.kzg.Fq
        self.alg = OB.OracleShardBackend(curve)
        self.ch = {k: int(self.trace[k]) for k in ("beta", "gamma", "alpha", "zeta")}
        polys = dict(self.ipk["polynomials"], **{k: self.trace[k] for k in ("a", "b", "c", "z", "PI", "t", "t_lo", "t_mid",
                                                                               "t_hi", "r")})
        self.polys = {k: [int(c) % r for c in p.list()] for k, p in polys.items()}
        # the coset K * <w4> of the size-4n subgroup, natural order, and every polynomial on it
        n4 = 4 * self.n
        w4, K = int(self.Fq.root_of_unity(n4)), int(self.Fq.multiplicative_generator())
        self.pts = [K * pow(w4, i, r) % r for i in range(n4)]
        self.on_coset = {k: self.at(k, self.pts) for k in self.polys}
        self.z_shifted = self.at("z", [self.g * x % r for x in self.pts])

    def at(self, name, points):
        return [O.poly_eval(self.polys[name], x, self.r) for x in points]


@pytest.fixture(scope="module", params=CURVES)
def case(request):
    return Case(request.param)


def coset_expectations(c):
    """gate, permutation, L1 term and quotient at every coset point, on scalars (plonk/prover.py:297-316)"""
    r, n = c.r, c.n
    beta, gamma, alpha = c.ch["beta"], c.ch["gamma"], c.ch["alpha"]
    V = c.on_coset
    gate, perm, l1t = [], [], []
    for i, x in enumerate(c.pts):
        a, b, cc, z = V["a"][i], V["b"][i], V["c"][i], V["z"][i]
        gate.append((a * b * V["qM"][i] + a * V["qL"][i] + b * V["qR"][i] + cc * V["qO"][i] + V["PI"][i] + V["qC"][i]) % r)
        p1 = (a + beta * x + gamma) * (b + beta * c.k1 * x + gamma) * (cc + beta * c.k2 * x + gamma) * z
        p2 = ((a + beta * V["S_sigma1"][i] + gamma) * (b + beta * V["S_sigma2"][i] + gamma)
              * (cc + beta * V["S_sigma3"][i] + gamma) * c.z_shifted[i])
        perm.append((p1 - p2) % r)
        L1 = (pow(x, n, r) - 1) * pow(n * (x - 1), -1, r)
        l1t.append((z - 1) * L1 % r)
    return gate, perm, l1t, V["t"]


def run_coset_algebra(c, order):
    """the shared functions on vectors laid out as order[j] = natural index of element j; results back in natural order"""
    from kzg_snark_amd import plonk_rounds as R
    alg, r, n = c.alg, c.r, c.n
    n4 = 4 * n
    beta, gamma, alpha = c.ch["beta"], c.ch["gamma"], c.ch["alpha"]

    def vec(values):
        return OB.tensor_of([values[i] for i in order])

    def natural(t):
        out = [None] * n4
        for j, v in enumerate(OB.ints_of(t)):
            out[order[j]] = v
        return out

    E = {k: vec(c.on_coset[k]) for k in WIRES + SIGMAS + ("PI", "z", "qM", "qL", "qR", "qO", "qC")}
    xs, ones = vec(c.pts), alg.const(n4, 1)
    D = R.coset_constants(alg, n4, n, xs, vec([pow(x, n, r) for x in c.pts]), ones)
    gate = R.gate_constraint(alg, E)
    perm = R.permutation_constraint(alg, n4, E, vec(c.z_shifted), xs, ones, beta, gamma, c.k1, c.k2)
    l1t = R.l1_term(alg, E, ones, D["l1"])
    t_ev = R.quotient_evaluations(alg, n4, gate, perm, l1t, alpha, D["zh_inv"])
    return tuple(natural(t) for t in (gate, perm, l1t, t_ev))


def test_coset_evaluations_match_the_host_polynomials(case):
    """gate_constraint, permutation_constraint, l1_term and quotient_evaluations (with coset_constants' 1/Z_H and L1)
    on K w4^i, challenges from the host trace, against the host prover's polynomials at those points -- the quotient
    against trace["t"] itself; then the same with every input vector permuted by i -> 5 i + 3 mod 4n and the outputs
    un-permuted: the functions are element-wise, which is what lets the transposed layout share them."""
    c = case
    n4 = 4 * c.n
    want = coset_expectations(c)
    assert any(want[0]) and any(want[1]) and any(want[2]) and any(want[3])      # every term is live
    permuted = [(5 * i + 3) % n4 for i in range(n4)]
    assert sorted(permuted) == list(range(n4)) and permuted != list(range(n4))
    for order in (list(range(n4)), permuted):
        got = run_coset_algebra(c, order)
        for name, g_, w_ in zip(("gate", "permutation", "L1 term", "quotient"), got, want):
            assert g_ == w_, (name, "natural" if order[0] == 0 else "permuted")


def test_accumulator_ratios_give_the_host_accumulator(case):
    """exclusive prefix product of accumulator_ratios over H == acc of plonk.Prover (z(g^i): the blinding term
    vanishes on H)"""
    from kzg_snark_amd import plonk_rounds as R
    c, alg = case, case.alg
    r, n = c.r, c.n
    full = [int(v) % r for v in c.x + c.w]
    m = len(full) // 3
    vals = [OB.tensor_of(full[i * m:(i + 1) * m] + [0] * (n - m)) for i in range(3)]
    ss = c.ipk["sigma_star"]
    S = {k: OB.tensor_of([int(v) for v in ss[j * n:(j + 1) * n]]) for j, k in enumerate(SIGMAS)}
    H = [pow(c.g, i, r) for i in range(n)]
    ratios = R.accumulator_ratios(alg, n, vals, S, OB.tensor_of(H), alg.const(n, 1), c.ch["beta"], c.ch["gamma"],
                                  c.k1, c.k2)
    acc = c.at("z", H)
    assert acc[0] == 1 and len(set(acc)) > 2
    assert OB.ints_of(alg.prefix_product(ratios)) == acc


def padded(coeffs, length):
    assert len(coeffs) <= length
    return coeffs + [0] * (length - len(coeffs))


def test_linearisation_scalars_rebuild_r(case):
    """sum_k s_k * polynomial_k + constant == trace["r"], coefficient for coefficient; and the vector-sharded prover's
    split for G = 2 -- rank g combines coefficients [g m, (g+1) m), rank 0 adds the constant, the coefficients from
    X^n on are combined as a tail -- reassembles to the same list"""
    from kzg_snark_amd import plonk_rounds as R
    c, alg = case, case.alg
    r, n, zeta = c.r, c.n, c.ch["zeta"]
    ev = {k: int(v) for k, v in c.trace["evaluations"].items()}
    L1z = int(R.lagrange_1_at(c.Fq, n, c.Fq(zeta)))
    PIz = O.poly_eval(c.polys["PI"], zeta, r)
    s, const = R.linearisation(ev, c.ch["beta"], c.ch["gamma"], c.ch["alpha"], zeta, n, c.k1, c.k2, L1z, PIz, r)
    assert tuple(s) == R.LINEARISED and all(int(v) % r for v in s.values()) and const
    want = padded(c.polys["r"], n + 6)
    full = {k: padded(c.polys[k], n + 6) for k in R.LINEARISED}
    whole = [sum(s[k] * full[k][i] for k in R.LINEARISED) % r for i in range(n + 6)]
    whole[0] = (whole[0] + const) % r
    assert whole == want
    m = n // 2
    pieces = []
    for rank in range(2):
        local = alg.lincomb(m, [(s[k], OB.tensor_of(full[k][rank * m:(rank + 1) * m])) for k in R.LINEARISED])
        if rank == 0:
            alg.set_entries(local, [(0, const)])
        pieces += OB.ints_of(local)
    tail = [sum(s[k] * full[k][n + j] for k in R.LINEARISED) % r for j in range(6)]
    assert pieces + tail == want


@pytest.mark.parametrize("as_limbs", [False, True], ids=["ints", "limbs"])
@pytest.mark.parametrize("nx", [0, 1, 4])
def test_witness_intake(nx, as_limbs):
    """Witness: the column parts of every (G, rank) concatenate to the slice of x ++ w, the PI values are -x_i on the
    range and zero elsewhere -- with x empty, ending inside a range (nx = 1; nx = 4 of one rank's 8 rows) and ending
    on the boundary between two ranks (nx = 4, G = 2)"""
    from kzg_snark_amd import _native
    from kzg_snark_amd import plonk_rounds as R
    r, n = O.BLS12_381.r, 8
    rng = random.Random(nx)
    x = [rng.randrange(r) for _ in range(nx)]
    w = [rng.randrange(r) for _ in range(3 * n - nx)]
    full = _native.ints_to_limbs(x + w)
    wit = R.Witness(x, _native.ints_to_limbs(w) if as_limbs else w, n, r)
    assert wit.nx == nx
    for G, rank in ((1, 0), (2, 0), (2, 1)):
        m = n // G
        lo = rank * m
        for i in range(3):
            parts = wit.column_parts(i, lo, m)
            assert np.array_equal(np.concatenate(parts), full[i * n + lo:i * n + lo + m]), (G, rank, i)
        neg = wit.public_inputs(lo, m)
        assert padded(neg, m) == [(-x[j]) % r if j < nx else 0 for j in range(lo, lo + m)], (G, rank)
    assert all(np.array_equal(np.concatenate(wit.column_parts(i)), full[i * n:(i + 1) * n]) for i in range(3))
    assert wit.public_inputs() == wit.public_inputs(0, n)
    with pytest.raises(AssertionError):
        R.Witness(x, w[:-1], n, r)                       # x ++ w must fill the three columns


def test_blinders_are_eleven():
    from kzg_snark_amd import plonk_rounds as R
    from kzg_snark_amd.field import GF
    Fq = GF(O.BN254.r)
    drawn = R.draw_blinders(Fq)
    assert len(drawn) == 11 and all(isinstance(v, int) and 0 <= v < Fq.p for v in drawn)
    assert R.draw_blinders(Fq, [Fq.p + i for i in range(11)]) == list(range(11))
    with pytest.raises(AssertionError):
        R.draw_blinders(Fq, range(10))


@pytest.mark.parametrize("curve", CURVES)
def test_lagrange_1_at(curve):
    from kzg_snark_amd import plonk_rounds as R
    from kzg_snark_amd.field import GF
    from kzg_snark_amd.plonk import Domain
    r = O.curve(curve).r
    Fq = GF(r)
    rng = random.Random(7)
    for n in (8, 16):
        for x in (rng.randrange(2, r), rng.randrange(2, r)):
            got = R.lagrange_1_at(Fq, n, Fq(x))
            assert got == Domain(Fq, n).lagrange_1_at(Fq(x))
            assert int(got) == P.p_eval(P.first_lagrange(n, r), x, r)

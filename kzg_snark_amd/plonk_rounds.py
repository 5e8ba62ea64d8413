"""The algebra of the five PLONK rounds (plonk/prover.py:24-212) that does not depend on where a vector lives or how it
is laid out: stated once for plonk_device.DeviceProver (whole vectors, natural order) and plonk_sharded.ShardedProver
(a range of n/G values on H, a transposed-layout shard of 4n/G coset evaluations).

`alg` is anything with mul / add / sub / lincomb / inverse over [m, 4] vectors of canonical Fr elements
(plonk_device.DeviceAlgebra; tests use the oracle's CPU backend); `m` is the length of the vectors at hand.  Everything
here is element-wise, so any layout serves as long as all vectors of a call share it.  Layout, transforms, where a
round's commitments begin and end, exchanges and openings stay with each prover; plonk.Prover / plonk.Verifier (dense
host polynomials) state the protocol on their own: they are what these provers are tested against."""
import numpy as np

from . import _native

EVALUATIONS = ("a", "b", "c", "s_sigma1", "s_sigma2", "z_omega")       # plonk/prover.py:140-150, transcript order
LINEARISED = ("qM", "qL", "qR", "qO", "qC", "z", "S_sigma3", "t_lo", "t_mid", "t_hi")


def lagrange_1_at(Fq, n, x):
    """L1(x) = (x^n - 1) / (n (x - 1)), the first Lagrange polynomial of the order-n subgroup"""
    return (x ** n - 1) / (Fq(n) * (x - 1))


class Witness:
    """x ++ w (3n values: wire column i is rows [i n, (i+1) n)) as canonical limb arrays.  `w` may already be a
    uint64[., 4] array (what a witness generator emits): no per-element Python work then."""

    def __init__(self, x, w, n, r):
        self.n, self.r = n, r
        self.x = [int(v) % r for v in x]
        self.x_limbs = _native.ints_to_limbs(self.x).reshape(-1, 4)
        if isinstance(w, np.ndarray):
            self.w_limbs = np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, 4)
        else:
            self.w_limbs = _native.ints_to_limbs([int(v) % r for v in w]).reshape(-1, 4)
        self.nx = len(self.x)
        assert self.nx + self.w_limbs.shape[0] == 3 * n

    def column_parts(self, i, lo=0, m=None):
        """limb arrays whose concatenation is rows [i n + lo, i n + lo + m) of x ++ w (m = n: the whole column) --
        slices, so the 96 n bytes are never copied on the host"""
        a = i * self.n + lo
        b = a + (self.n if m is None else m)
        parts = []
        if a < self.nx:
            parts.append(self.x_limbs[a:min(b, self.nx)])
        if b > self.nx:
            parts.append(self.w_limbs[max(a, self.nx) - self.nx:b - self.nx])
        return parts

    def public_inputs(self, lo=0, m=None):
        """PI values -x_i of rows [lo, lo + m) that carry a public input (the leading ones; every later row is zero)"""
        return [(-v) % self.r for v in self.x[lo:lo + (self.n if m is None else m)]]


def draw_blinders(Fq, given=None):
    """b1..b11 of plonk/prover.py:72-75 and :346 in the reference's order; `given` (tests only) fixes them"""
    b = [int(Fq.random_element()) for _ in range(11)] if given is None else [int(v) % Fq.p for v in given]
    assert len(b) == 11
    return b


def gate_constraint(alg, E):
    """a b qM + a qL + b qR + c qO + PI + qC on evaluations E (plonk/prover.py:297)"""
    gate = alg.add(alg.add(alg.mul(alg.mul(E["a"], E["b"]), E["qM"]), alg.mul(E["a"], E["qL"])),
                   alg.add(alg.mul(E["b"], E["qR"]), alg.mul(E["c"], E["qO"])))
    return alg.add(gate, alg.add(E["PI"], E["qC"]))


def _copy_products(alg, m, wires, sigmas, ident, ones, beta, gamma, k1, k2):
    """prod_j (w_j + beta k_j id + gamma) and prod_j (w_j + beta sigma_j + gamma) over the three wires, k = 1, k1, k2"""
    num = den = None
    for v, shift, sig in zip(wires, (1, int(k1), int(k2)), sigmas):
        fn = alg.lincomb(m, [(1, v), (beta * shift, ident), (gamma, ones)])
        fd = alg.lincomb(m, [(1, v), (beta, sig), (gamma, ones)])
        num = fn if num is None else alg.mul(num, fn)
        den = fd if den is None else alg.mul(den, fd)
    return num, den


def accumulator_ratios(alg, m, vals, sigma_values, idH, ones, beta, gamma, k1, k2):
    """num_i / den_i on H (plonk/prover.py:243-264); z_i is their exclusive prefix product.  One batch inversion
    instead of the reference's n - 1 sequential divisions."""
    sigmas = [sigma_values[k] for k in ("S_sigma1", "S_sigma2", "S_sigma3")]
    num, den = _copy_products(alg, m, vals, sigmas, idH, ones, beta, gamma, k1, k2)
    return alg.mul(num, alg.inverse(den))


def permutation_constraint(alg, m, E, zw, xs, ones, beta, gamma, k1, k2):
    """prod (w_j + beta k_j X + gamma) z - prod (w_j + beta S_sigma_j + gamma) z(g X) at the points xs
    (plonk/prover.py:299-309); zw holds z(g x)"""
    p1, p2 = _copy_products(alg, m, [E[k] for k in ("a", "b", "c")], [E[k] for k in ("S_sigma1", "S_sigma2", "S_sigma3")],
                            xs, ones, beta, gamma, k1, k2)
    return alg.sub(alg.mul(p1, E["z"]), alg.mul(p2, zw))


def l1_term(alg, E, ones, l1):
    """(z - 1) L1 (plonk/prover.py:311-313)"""
    return alg.mul(alg.sub(E["z"], ones), l1)


def quotient_evaluations(alg, m, gate, perm, l1t, alpha, zh_inv):
    """t = (gate + alpha perm + alpha^2 (z - 1) L1) / Z_H point by point (plonk/prover.py:297-316)"""
    return alg.mul(alg.lincomb(m, [(1, gate), (alpha, perm), (alpha * alpha, l1t)]), zh_inv)


def coset_constants(alg, m, n, xs, xn, ones):
    """from coset points xs, their n-th powers and ones: 1 / Z_H(x), Z_H = X^n - 1 (four values on a coset of the
    size-4n subgroup), and L1(x) = Z_H(x) / (n (x - 1))"""
    zh = alg.sub(xn, ones)
    return {"zh_inv": alg.inverse(zh), "l1": alg.mul(zh, alg.inverse(alg.lincomb(m, [(n, xs), (-n, ones)])))}


def linearisation(ev, beta, gamma, alpha, zeta, n, k1, k2, L1z, PIz, r):
    """r(X) (plonk/prover.py:358-414) as scalars: ({name: s} over LINEARISED, constant term) with
    r = sum_name s_name * name(X) + constant; the scalars are unreduced integers"""
    za, zb, zc, s1, s2, zo = (ev[k] for k in EVALUATIONS)
    k1, k2 = int(k1), int(k2)
    zn = pow(zeta, n, r)
    f1 = (za + beta * zeta + gamma) * (zb + beta * k1 * zeta + gamma) * (zc + beta * k2 * zeta + gamma) % r
    f2 = (za + beta * s1 + gamma) * (zb + beta * s2 + gamma) * zo % r
    scalars = (za * zb, za, zb, zc, 1, alpha * f1 + alpha * alpha * L1z, -alpha * f2 * beta,
               -(zn - 1), -(zn - 1) * zn, -(zn - 1) * zn * zn)
    return dict(zip(LINEARISED, scalars)), (PIz - alpha * f2 * (zc + gamma) - alpha * alpha * L1z) % r


def proof_dict(wire_comms, z_comm, t_comms, evaluations, W_z, W_zw):
    """plonk/prover.py:188-210"""
    return {"commitments": dict(zip(("a", "b", "c"), wire_comms), z=z_comm,
                                t_lo=t_comms[0], t_mid=t_comms[1], t_hi=t_comms[2]),
            "evaluations": evaluations,
            "kzg_proofs": {"W_z": W_z, "W_zw": W_zw}}


def prove_flushing(flush, prove, *args):
    """prove(*args); a proof that fails half way (an assert of the protocol, an allocation) must not leave commitments
    of its rounds queued in the library's pipeline: `flush` (None: nothing to drain) runs before the error travels on"""
    try:
        return prove(*args)
    except BaseException:
        if flush is not None:
            try:
                flush()
            except Exception:   # noqa: BLE001
                pass
        raise

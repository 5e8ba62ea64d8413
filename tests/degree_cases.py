"""The degree rule of commit and of every opening as a table of cases with their expectations in plain integers (a plain
helper module, no fixtures).  The reference refuses a polynomial whose DEGREE exceeds len(ck) - 1 (kzg.py:103-106), an
opening inherits that through the commit of its witness (kzg.py:157), and trailing zeros are not degree.

A case is (label, m, polys, z, xi): m key points, the coefficient lists as the C ABI gets them (trailing zeros kept,
lens[i] = len(polys[i])), n = the longest length.  R = n - 1 - m is the number of quotient coefficients beyond the key:
the range any_nonzero_kernel looks at.  The expectation: O.combine -> O.poly_divide_linear -> O.poly_normalize; `refuse`
iff the normalised witness has more than m coefficients (the reference's own `if`); the evaluation P(z); the point by
the trapdoor identity O.open_trapdoor with the key's known tau.  The label's first letter is the family:

  A  the length boundary: k = 1, n = m, m + 1 (the witness fills the key: the check does not run), m + 2
  B  trailing zeros through the ABI: effective length m + 1 (accept) or m + 2 (the first element of the range is the
     lone dirty one), padded with literal zeros to a range of R
  C  z = 0, xi = 1, k = 1, so that q_j = c_(j+1): one dirty coefficient anywhere in the range, of every single word;
     and the mirror, q_(m-1) = r - 1 below a clean range
  D  B again, to be opened right after a longer opening on the same context (stale_poly): non-zero words beyond the range
  E  cancellation: k = 2 and 17, p_0 chosen so that sum xi^(i+1) p_i vanishes above the key; or at all but one index
  F  kzg_open_points (PointsCase: label, m, polys, points, weights), expectation by multi_restated.quotient_points

table(curve) holds the shapes the GPU tests run, table(curve, small=True) the same families at m <= 8 for the oracle."""
import random
from collections import namedtuple
from functools import lru_cache

from multi_restated import quotient_points
from oracle import py_oracle as O

CURVES = ["bls12_381", "bn254"]
TAU = 0x1d0c5eed0badc0ffee1234567
FAMILIES = "ABCDE"
STALE_EXTRA = 700                    # how much longer the opening before a case of family D is
MAX_N = 2 * 2048 + 2 * 2049          # no case is longer (keeps the uploads small)

Case = namedtuple("Case", "label m polys z xi")
PointsCase = namedtuple("PointsCase", "label m polys points weights")
Expect = namedtuple("Expect", "verdict value point")      # point: affine (x, y) or None for infinity; accept only
ExpectPoints = namedtuple("ExpectPoints", "verdict quotient point")   # quotient: all n - 1 coefficients

FULL = dict(A_m=(1, 2, 255, 256, 2048), B_m=(255, 300, 2048), B_R=(1, 255, 256, 257, 513, 2049),
            C_m=300, C_R=(257, 513), C_d=(0, 255, 256), D_m=(300, 2048), D_R=(1, 257), E_m=(300, 2048), E_R=(1, 300),
            F=((300, 300), (2048, 257)))
SMALL = dict(A_m=(1, 2, 3, 4), B_m=(2, 5), B_R=(1, 2, 3), C_m=3, C_R=(3, 5), C_d=(0, 1, 2), D_m=(2, 5), D_R=(1, 3),
             E_m=(2, 5), E_R=(1, 3), F=((3, 3), (5, 2)))


def family(case):
    return case.label[0]


def length(case):
    return max((len(p) for p in case.polys), default=0)


def beyond(case):
    """R: how many quotient coefficients lie beyond the key (<= 0: the library's check does not run)"""
    return length(case) - 1 - case.m


def tau_of(curve):
    return TAU % O.curve(curve).r


def _rng(curve, label):
    return random.Random(f"{curve}/{label}")


def rand_poly(rng, n, r):
    """n random coefficients, the top one non-zero"""
    return [rng.randrange(r) for _ in range(n - 1)] + [rng.randrange(1, r)] if n else []


def _padded(rng, r, m, R, kind):
    """effective length m + 1 (`fits`) or m + 2 (`over`), zeros up to n = m + 1 + R"""
    return rand_poly(rng, m + 1, r) + [0] * R if kind == "fits" else rand_poly(rng, m + 2, r) + [0] * (R - 1)


def cancelling(rng, r, k, m, R, kind, xi):
    """k random polynomials of n = m + 1 + R coefficients; p_0[i] = -sum_(j>=1) xi^j p_j[i] for i > m, so that the
    combination sum_i xi^(i+1) p_i = xi (p_0 + sum_(j>=1) xi^j p_j) vanishes there -- but for one index, if `kind` says"""
    n = m + 1 + R
    polys = [rand_poly(rng, n, r) for _ in range(k)]
    for i in range(m + 1, n):
        polys[0][i] = -sum(pow(xi, j, r) * polys[j][i] for j in range(1, k)) % r
    if kind != "cancel":
        i = m + 1 if kind == "low" else n - 1
        polys[0][i] = (polys[0][i] + 1) % r
    return polys


@lru_cache(maxsize=None)
def table(curve, small=False):
    P = SMALL if small else FULL
    r = O.curve(curve).r
    out = []

    def points_of(rng, extreme=False):
        return [("z0", 0), ("zr", rng.randrange(1, r))] + ([("zmax", r - 1)] if extreme else [])

    for m in P["A_m"]:
        for extra in (0, 1, 2):
            rng = _rng(curve, f"A:{m}:{extra}")
            for zname, z in points_of(rng):
                out.append(Case(f"A:m{m}:n=m+{extra}:{zname}", m, [rand_poly(rng, m + extra, r)], z, rng.randrange(1, r)))
    for fam, ms, Rs in (("B", P["B_m"], P["B_R"]), ("D", P["D_m"], P["D_R"])):
        for m in ms:
            for R in Rs:
                for kind in ("fits", "over"):
                    rng = _rng(curve, f"{fam}:{m}:{R}:{kind}")
                    for zname, z in points_of(rng):
                        out.append(Case(f"{fam}:m{m}:R{R}:{kind}:{zname}", m, [_padded(rng, r, m, R, kind)], z,
                                        rng.randrange(1, r)))
    m = P["C_m"]
    for R in P["C_R"]:
        rng = _rng(curve, f"C:{R}")
        low = rand_poly(rng, m + 1, r)
        dirty = [(f"d{d}", d, rng.randrange(1, r)) for d in sorted({*P["C_d"], R - 1})]
        dirty += [(f"word{w}", R - 1, 1 << (32 * w)) for w in range(8)]       # one non-zero word each, all below r
        for name, d, v in dirty:
            poly = low + [0] * R
            poly[m + 1 + d] = v                                              # q_(m+d): offset d of the range
            out.append(Case(f"C:R{R}:{name}", m, [poly], 0, 1))
        out.append(Case(f"C:R{R}:mirror", m, [low[:m] + [r - 1] + [0] * R], 0, 1))   # q_(m-1) = r - 1 still fits
    for k in (2, 17):
        for m in P["E_m"]:
            for R in P["E_R"]:
                for kind in ("cancel", "low", "high")[:2 if R == 1 else 3]:
                    rng = _rng(curve, f"E:{k}:{m}:{R}:{kind}")
                    for zname, z in points_of(rng, extreme=True):
                        xi = rng.randrange(2, r)
                        out.append(Case(f"E:k{k}:m{m}:R{R}:{kind}:{zname}", m, cancelling(rng, r, k, m, R, kind, xi), z, xi))
    assert len({c.label for c in out}) == len(out)
    assert all(c.z != tau_of(curve) for c in out)                            # the trapdoor identity divides by tau - z
    return out


def stale_poly(curve, case):
    """what family D opens first on the same context: STALE_EXTRA coefficients more, all random"""
    return rand_poly(_rng(curve, "stale:" + case.label), length(case) + STALE_EXTRA, O.curve(curve).r)


def witness(case, r):
    """-> (the normalised witness of the reference, P(z))"""
    q, value = O.poly_divide_linear(O.combine(case.polys, case.xi, r), case.z, r)
    return O.poly_normalize(q), value


def verdict(case, r):
    return "refuse" if len(witness(case, r)[0]) > case.m else "accept"


_EXPECT = {}


def expect(curve, case):
    """Expect(verdict, P(z), point); computed once per case (one scalar multiplication when accepted)"""
    key = (curve, case.label)
    if key not in _EXPECT:
        cv = O.curve(curve)
        q, value = witness(case, cv.r)
        if len(q) > case.m:
            _EXPECT[key] = Expect("refuse", value, None)
        else:
            point = O.open_trapdoor(case.polys, case.z, case.xi, tau_of(curve), cv)
            _EXPECT[key] = Expect("accept", value, O.normalize(point, cv))
    return _EXPECT[key]


# ---- family F -----------------------------------------------------------------------------------------------------

def as_points(case, r):
    """a case of the table as kzg_open_points sees it: t = 1, the weights xi^(i+1)"""
    return PointsCase("F:" + case.label, case.m, case.polys, [case.z],
                      [[pow(case.xi, i + 1, r)] for i in range(len(case.polys))])


def _cancel_over_points(polys, points, weights, m, r):
    """sets the coefficients of polys[0] above index m so that the quotient sum_j Q_(z_j)[c_j] vanishes from index m
    on although no single combination c_j = sum_i w_ij p_i does.  With S_j(i) = c_j[i+1] + z_j S_j(i+1) the quotient's
    coefficient i is sum_j S_j(i), linear in polys[0][i+1] with the slope sum_j w_0j."""
    n = len(polys[0])
    slope = sum(row for row in weights[0]) % r
    assert slope and all(len(p) <= n for p in polys)
    inv = pow(slope, -1, r)
    S = [0] * len(points)
    for i in range(n - 2, m - 1, -1):
        rest = [(sum(w[j] * (p[i + 1] if i + 1 < len(p) else 0) for p, w in zip(polys[1:], weights[1:])) + z * S[j]) % r
                for j, z in enumerate(points)]
        x = -sum(rest) * inv % r
        polys[0][i + 1] = x
        S = [(weights[0][j] * x + rest[j]) % r for j in range(len(points))]


@lru_cache(maxsize=None)
def points_table(curve, small=False):
    """the cases of family F that are not as_points of B and E: t = 4 (two launches of three points), a cancelling
    combination and the same with the top coefficient off by one; nothing but zero weights; one polynomial longer than
    the key that carries no weight"""
    r = O.curve(curve).r
    out = []
    for m, R in (SMALL if small else FULL)["F"]:
        n = m + 1 + R
        rng = _rng(curve, f"F:{m}:{R}")
        polys = [rand_poly(rng, n, r), rand_poly(rng, n, r), rand_poly(rng, n - 2, r)]
        points = [rng.randrange(1, r), rng.randrange(1, r), r - 1, 0]
        weights = [[rng.randrange(1, r) for _ in points] for _ in polys]
        weights[1][2] = 0                                                    # a zero weight beside non-zero ones
        _cancel_over_points(polys, points, weights, m, r)
        tag = f"F:m{m}:R{R}"
        out.append(PointsCase(tag + ":t4:cancel", m, [list(p) for p in polys], points, weights))
        off = [list(p) for p in polys]
        off[0][n - 1] = (off[0][n - 1] + 1) % r
        out.append(PointsCase(tag + ":t4:high", m, off, points, weights))
        out.append(PointsCase(tag + ":zero-weights", m, [rand_poly(rng, n, r), rand_poly(rng, n - 1, r)], points[:2],
                              [[0, 0], [0, 0]]))
        out.append(PointsCase(tag + ":long-unweighted", m, [rand_poly(rng, m + 1, r), rand_poly(rng, n, r), rand_poly(rng, m, r)],
                              points[2:], [[rng.randrange(1, r), rng.randrange(1, r)], [0, 0], [0, rng.randrange(1, r)]]))
    return out


def expect_points(curve, pc):
    """ExpectPoints(verdict, the restated quotient with its zeros beyond the key, [q(tau)] G1 when accepted)"""
    key = (curve, pc.label)
    if key not in _EXPECT:
        cv = O.curve(curve)
        q = quotient_points(pc.polys, pc.points, pc.weights, cv.r)
        if len(O.poly_normalize(q)) > pc.m:
            _EXPECT[key] = ExpectPoints("refuse", q, None)
        else:
            _EXPECT[key] = ExpectPoints("accept", q, O.normalize(O.commit_trapdoor(q, tau_of(curve), cv), cv))
    return _EXPECT[key]

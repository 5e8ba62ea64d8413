"""Shared inputs of the compressed-G2 tests (a plain helper module, no fixtures): the host shim, the golden vectors, a
seeded generator of points of the twist and the subgroup matrix of both curves, with every expected verdict taken from
kzg_snark_amd/curve.py's single-point helpers ([r] Q = O)."""
import ctypes
import json
import os
import random
import subprocess
from functools import lru_cache

from kzg_snark_amd import curve as C

HERE = os.path.dirname(os.path.abspath(__file__))
CURVE_IDS = {"bn254": 0, "bls12_381": 1}
SHIM_DIR = os.path.join(HERE, "shim")
SHIM_SRC = os.path.join(SHIM_DIR, "g2_bytes_shim.cpp")
INF2 = ((1, 0), (1, 0), (0, 0))


@lru_cache(maxsize=None)
def build_shim(audit=False):
    """csrc/g2_bytes.h compiled for the host (tests/shim/g2_bytes_shim.cpp), loaded"""
    kind = "audit" if audit else "plain"
    so = os.path.join(SHIM_DIR, f"libg2_bytes_shim_{kind}.so")
    subprocess.run(["g++", "-O1", "-std=c++17", *(["-DKZG_AUDIT"] if audit else []), "-shared", "-fPIC",
                    SHIM_SRC, "-o", so], check=True)
    return ctypes.CDLL(so)


def fp_words(cv):
    return (cv.p.bit_length() + 31) // 32


def g2_generator(cv):
    return (cv.g2[0], cv.g2[1], (1, 0))


def point_value(pt, nw):
    """the integer whose 4 nw little-endian words are x.c0 | x.c1 | y.c0 | y.c1 (0 for infinity)"""
    if pt[2] == (0, 0):
        return 0
    sh = 32 * nw
    return pt[0][0] | (pt[0][1] << sh) | (pt[1][0] << (2 * sh)) | (pt[1][1] << (3 * sh))


def value_point(v, nw, inf=False):
    if inf:
        return INF2
    sh, m = 32 * nw, (1 << (32 * nw)) - 1
    return ((v & m, (v >> sh) & m), ((v >> (2 * sh)) & m, (v >> (3 * sh)) & m), (1, 0))


def twist_rhs(x, cv):
    K = C._Fp2(cv.p)
    return K.add(K.mul(K.mul(x, x), x), cv.b2)


def random_twist_point(cv, rng):
    """a uniformly random finite point of E'(Fp2), y of either sign"""
    while True:
        x = (rng.randrange(cv.p), rng.randrange(cv.p))
        y = C.sqrt_fp2(twist_rhs(x, cv), cv.p)
        if y is not None:
            return (x, y if rng.randrange(2) else C._Fp2(cv.p).neg(y), (1, 0))


@lru_cache(maxsize=None)
def golden():
    with open(os.path.join(HERE, "golden", "g2_bytes_vectors.json")) as f:
        return json.load(f)


def _pt(e):
    return ((int(e["x0"], 16), int(e["x1"], 16)), (int(e["y0"], 16), int(e["y1"], 16)), (1, 0))


def golden_points(name):
    """[(blob, point)] of the golden file, infinity last"""
    g = golden()[name]
    return [(bytes.fromhex(p["blob"]), _pt(p)) for p in g["points"]] + [(bytes.fromhex(g["infinity"]), INF2)]


def golden_failures(name):
    """[(blob, status, case)]"""
    g = golden()[name]
    return [(bytes.fromhex(e["blob"]), st, e["case"]) for st in (1, 2, 3) for e in g["status%d" % st]]


def golden_real_rhs(name):
    """[(blob, point, kind)]: points whose x^3 + b' lies in Fp -- kind "residue" (a real y) or "non-residue" (a purely
    imaginary y) -- the two special branches of the square root through decompression"""
    return [(bytes.fromhex(e["blob"]), _pt(e), e["kind"]) for e in golden()[name]["real_rhs"]]


@lru_cache(maxsize=None)
def subgroup_matrix_g2(name, seed=0x62b):
    """[(point, in_subgroup, what)] -- 16 random points Q of the twist (none in G2: asserted), their cofactor parts
    T = [r] Q (all finite: asserted), P + T for random P in G2, 16 points P of G2, infinity.  Verdicts are [r] Q = O."""
    cv = C.CURVES[name]
    G = C.g2_group(cv)
    g = g2_generator(cv)
    rng = random.Random(seed + CURVE_IDS[name])
    rows = []
    for i in range(16):
        q = random_twist_point(cv, rng)
        t = G.multiply(q, cv.r)
        assert t[2] == (1, 0), "a random point of the twist fell into G2"
        p = G.multiply(g, rng.randrange(1, cv.r))
        rows += [(q, "Q%d" % i), (t, "T%d = [r] Q%d" % (i, i)), (G.add(p, t), "P + T%d" % i), (p, "P%d in G2" % i)]
    rows += [(INF2, "infinity")]
    out = [(pt, C.in_subgroup_g2(pt, cv), what) for pt, what in rows]
    assert all(C.on_curve_g2(pt, cv) for pt, _, _ in out)
    assert not any(ok for _, ok, what in out if what.startswith("Q"))
    assert sum(1 for _, ok, _ in out if not ok) >= 48 and sum(1 for _, ok, _ in out if ok) >= 17
    return out

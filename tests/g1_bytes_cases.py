"""Shared inputs of the compressed-point tests (a plain helper module, no fixtures): the golden vectors and the seeded
subgroup matrix, with every expected verdict taken from kzg_snark_amd/curve.py's single-point helpers ([r] P = O)."""
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
SHIM_SRC = os.path.join(SHIM_DIR, "g1_bytes_shim.cpp")


@lru_cache(maxsize=None)
def build_shim(audit=False):
    """csrc/g1_bytes.h and g1_words.h compiled for the host (tests/shim/g1_bytes_shim.cpp), loaded"""
    kind = "audit" if audit else "plain"
    so = os.path.join(SHIM_DIR, f"libg1_bytes_shim_{kind}.so")
    subprocess.run(["g++", "-O0" if audit else "-O1", "-std=c++17", *(["-DKZG_AUDIT"] if audit else []), "-shared", "-fPIC",
                    SHIM_SRC, "-o", so], check=True)
    return ctypes.CDLL(so)


def words(x, nw):
    """x as nw little-endian 32-bit words"""
    return (ctypes.c_uint32 * nw)(*[(x >> (32 * i)) & 0xffffffff for i in range(nw)])


def key_point_with_x_plus_p(cv, k=3):
    """(x + p, y) for the point [k] G1 = (x, y): not canonical, and the same point modulo p"""
    G = C.g1_group(cv)
    x, y, _ = G.multiply((cv.g1[0], cv.g1[1], 1), k)
    return x + cv.p, y


@lru_cache(maxsize=None)
def golden():
    with open(os.path.join(HERE, "golden", "g1_bytes_vectors.json")) as f:
        return json.load(f)


def golden_points(name):
    """[(blob, point)] of the golden file, infinity last"""
    g = golden()[name]
    out = [(bytes.fromhex(p["blob"]), (int(p["x"], 16), int(p["y"], 16), 1)) for p in g["points"]]
    return out + [(bytes.fromhex(g["infinity"]), (1, 1, 0))]


def golden_failures(name):
    """[(blob, status, case)]"""
    g = golden()[name]
    return [(bytes.fromhex(e["blob"]), st, e["case"]) for st in (1, 2, 3) for e in g["status%d" % st]]


def random_curve_point(cv, rng):
    while True:
        x = rng.randrange(cv.p)
        y = C.sqrt_fp((x * x * x + cv.b) % cv.p, cv.p)
        if y is not None:
            return (x, y if rng.randrange(2) else cv.p - y, 1)


@lru_cache(maxsize=None)
def subgroup_matrix(seed=0x5b6):
    """bls12_381: [(point, in_subgroup, what)] -- 16 random points Q of the curve (none in G1: asserted, so the
    reject class is not empty), their cofactor-torsion parts T = [r] Q, P + T for random P in G1, the point (0, 2) of
    order 3, 16 points of G1, infinity.  The verdicts are [r] P = O."""
    cv = C.BLS12_381
    G = C.g1_group(cv)
    g = (cv.g1[0], cv.g1[1], 1)
    rng = random.Random(seed)
    rows = []
    for i in range(16):
        q = random_curve_point(cv, rng)
        t = G.multiply(q, cv.r)
        assert t[2] == 1, "a random point of the curve fell into G1"
        p = G.multiply(g, rng.randrange(1, cv.r))
        rows += [(q, "Q%d" % i), (t, "T%d = [r] Q%d" % (i, i)), (G.add(p, t), "P + T%d" % i), (p, "P%d in G1" % i)]
    rows += [((0, 2, 1), "(0, 2), order 3"), ((1, 1, 0), "infinity")]
    out = [(pt, C.in_subgroup_g1(pt, cv), what) for pt, what in rows]
    assert all(C.on_curve_g1(pt, cv) for pt, _, _ in out)
    assert sum(1 for _, ok, _ in out if not ok) == 49 and sum(1 for _, ok, _ in out if ok) == 17
    return out

"""Shared inputs of the per-point scalar multiplication tests (a plain helper module, no fixtures): the scalars, the
points of both groups of both curves -- infinity, the generator, points outside the subgroup and points of small prime
order included -- the host shim of csrc/g_mul.h, and the expected products from curve.Group.multiply, which is exact
for any point and any integer (KZG.multiply reduces modulo r and is NOT the reference here)."""
import ctypes
import math
import os
import random
import subprocess
from functools import lru_cache

import numpy as np

from g2_bytes_cases import CURVE_IDS, INF2, fp_words, g2_generator, point_value, random_twist_point, value_point
from kzg_snark_amd import curve as C

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "shim")
SHIM_SRC = os.path.join(SHIM_DIR, "g_mul_shim.cpp")
CURVES = ["bls12_381", "bn254"]
INF1 = (1, 1, 0)
U32 = ctypes.c_uint32
# the curves' parameters u: t = 6 u^2 + 1 (BN254), t = u + 1 (BLS12-381) is the trace of Frobenius of E(Fp)
U = {"bn254": 0x44e992b44a6909f1, "bls12_381": -0xd201000000010000}
# a small prime q with q^2 (bls12_381: the 13-part of E'(Fp2) is not cyclic) or q (bn254) dividing the twist's cofactor
SMALL_PRIME = {"bls12_381": (13, 169), "bn254": (10069, 10069)}


def group(name, g):
    cv = C.CURVES[name]
    return C.g1_group(cv) if g == 1 else C.g2_group(cv)


@lru_cache(maxsize=None)
def orders(name):
    """(#E(Fp), #E'(Fp2)) from p, r and u.  With t the trace over Fp, the trace over Fp2 is t2 = t^2 - 2p, and the
    sextic twists of E over Fp2 have p^2 + 1 - (+-t2 +- 3f) / 2 points, f^2 = (4p^2 - t2^2) / 3; E' is the one whose
    order r divides and which annihilates a random point of the twist."""
    cv = C.CURVES[name]
    p, r, u = cv.p, cv.r, U[name]
    t = 6 * u * u + 1 if name == "bn254" else u + 1
    n1 = p + 1 - t
    assert n1 % r == 0 and C.g1_group(cv).is_inf(C.g1_group(cv).multiply((cv.g1[0], cv.g1[1], 1), n1))
    t2 = t * t - 2 * p
    f = math.isqrt((4 * p * p - t2 * t2) // 3)
    assert 3 * f * f == 4 * p * p - t2 * t2
    q = random_twist_point(cv, random.Random(5))
    G2 = C.g2_group(cv)
    n2 = [c for c in (p * p + 1 - (s2 * t2 + s3 * 3 * f) // 2 for s2 in (1, -1) for s3 in (1, -1))
          if c % r == 0 and G2.is_inf(G2.multiply(q, c))]
    assert len(n2) == 1
    return n1, n2[0]


@lru_cache(maxsize=None)
def scalars(name):
    """every scalar of the case list: the special ones first (special_scalars), then 16^j, the neighbourhoods of r and
    2r, seeded random 256-bit values"""
    r = C.CURVES[name].r
    assert 2 * r + 40 < 1 << 256 and r % 16 == 1
    rng = random.Random(0x6d75 + CURVE_IDS[name])
    out = list(special_scalars(name))
    out += [16 ** j for j in range(64)]
    out += list(range(r - 40, r + 41)) + list(range(2 * r - 40, 2 * r + 41))
    out += [rng.getrandbits(256) for _ in range(36)]
    assert all(0 <= k < 1 << 256 for k in out)
    return out


def special_scalars(name):
    r = C.CURVES[name].r
    ones = int("1" * 64, 16)
    return [0, 1, 2, 15, 16, 17, 1 << 255, (1 << 256) - 1, 8 * ones, 7 * ones, ones,
            r - 1, r, r + 1, 2 * r - 4, 2 * r - 2, 2 * r - 1, 2 * r, 2 * r + 1, 3, 13, 10069, 169]


@lru_cache(maxsize=None)
def points(name, g):
    """[(point, what)]: infinity, G, -G, random points of the subgroup, one point on the curve outside the subgroup and
    one of small prime order where the group has a cofactor (bn254's G1 has none)"""
    cv = C.CURVES[name]
    G = group(name, g)
    rng = random.Random(0x70 + 2 * CURVE_IDS[name] + g)
    n1, n2 = orders(name)
    gen = (cv.g1[0], cv.g1[1], 1) if g == 1 else g2_generator(cv)
    out = [(INF1 if g == 1 else INF2, "infinity"), (gen, "G"), (G.neg(gen), "-G")]
    out += [(G.multiply(gen, rng.randrange(1, cv.r)), "random subgroup point %d" % i) for i in range(3)]
    if g == 1 and name == "bls12_381":
        while True:
            x = rng.randrange(cv.p)
            y = C.sqrt_fp((x ** 3 + cv.b) % cv.p, cv.p)
            if y is not None and not G.is_inf(G.multiply((x, y, 1), cv.r)):
                break
        out.append(((x, y, 1), "outside the subgroup"))
        assert n1 % 3 == 0 and G.is_inf(G.multiply((0, 2, 1), 3))
        out.append(((0, 2, 1), "order 3"))
    if g == 2:
        q = random_twist_point(cv, rng)
        assert not G.is_inf(G.multiply(q, cv.r))
        out.append((q, "outside the subgroup"))
        prime, part = SMALL_PRIME[name]
        assert n2 % part == 0
        for _ in range(64):
            t = G.multiply(random_twist_point(cv, rng), n2 // part)
            if not G.is_inf(t):
                break
        assert not G.is_inf(t) and G.is_inf(G.multiply(t, prime)), "no point of order %d found" % prime
        out.append((t, "order %d" % prime))
    on = C.on_curve_g1 if g == 1 else C.on_curve_g2
    assert all(on(pt, cv) for pt, _ in out)
    return out


@lru_cache(maxsize=None)
def cases(name, g):
    """[(point, scalar, expected, what)]: every point against the special scalars, every scalar against G"""
    G = group(name, g)
    pts = points(name, g)
    pairs = [(pt, k, what) for pt, what in pts for k in special_scalars(name)]
    pairs += [(pts[1][0], k, "G") for k in scalars(name)[len(special_scalars(name)):]]
    return [(pt, k, G.normalize(G.multiply(pt, k)), what) for pt, k, what in pairs]


# ---- words ------------------------------------------------------------------------------------------------------------

def is_inf(pt, g):
    return pt[2] == 0 if g == 1 else tuple(pt[2]) == (0, 0)


def to_value(pt, g, nw):
    """the integer whose little-endian words are the point in the C layout (0 for infinity)"""
    if g == 2:
        return point_value(pt, nw)
    return 0 if pt[2] == 0 else pt[0] | (pt[1] << (32 * nw))


def from_value(v, inf, g, nw):
    if g == 2:
        return value_point(v, nw, inf)
    return INF1 if inf else (v & ((1 << (32 * nw)) - 1), v >> (32 * nw), 1)


def words(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


# ---- outputs with guard bytes behind them (the GPU tests through the C ABI) -----------------------------------------

GUARD = 0xA5
PAD = 192                     # guard bytes behind every output


def guarded(nbytes):
    return np.full(nbytes + PAD, GUARD, dtype=np.uint8)


def guard_ok(a, nbytes):
    return bool((a[nbytes:] == GUARD).all())


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@lru_cache(maxsize=None)
def build_shim():
    so = os.path.join(SHIM_DIR, "libg_mul_shim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", SHIM_SRC, "-o", so], check=True)
    return ctypes.CDLL(so)


def shim_consts(lib):
    """{group: (lanes per workgroup, lanes per launch)} and the largest n of a call, as csrc/g_mul.h states them"""
    lib.gm_const.restype = ctypes.c_uint64
    v = [int(lib.gm_const(i)) for i in range(5)]
    return {1: (v[0], v[2]), 2: (v[1], v[3])}, v[4]


def shim_plan(lib, n, g):
    """GmPlan of a call of n points of group g -> (blocks, launch_blocks)"""
    blocks, launch_blocks = U32(), U32()
    lib.gm_plan(ctypes.c_uint64(n), g, ctypes.byref(blocks), ctypes.byref(launch_blocks))
    return blocks.value, launch_blocks.value


def shim_table(lib, name, g, grid, launch_blocks):
    """a launch of `grid` workgroups over the table of a plan -> (pieces per entry, the largest index the launch touches
    by the kernels' 32-bit arithmetic, the vectors allocated for launch_blocks)"""
    pieces, top, vectors = U32(), U32(), ctypes.c_uint64()
    assert lib.gm_table(CURVE_IDS[name], g, grid, launch_blocks, ctypes.byref(pieces), ctypes.byref(top),
                        ctypes.byref(vectors)) == 0
    return pieces.value, top.value, vectors.value


def launches(lib, n, g):
    """[(first lane, end lane)] of the launches of a call of n points, as g_mul.hip's drivers loop: b0 = 0, launch_blocks,
    ... below blocks, each of min(launch_blocks, blocks - b0) workgroups (the last range ends at n)"""
    tb = shim_consts(lib)[0][g][0]
    blocks, launch_blocks = shim_plan(lib, n, g)
    out, b0 = [], 0
    while b0 < blocks:
        grid = min(launch_blocks, blocks - b0)
        out.append((b0 * tb, min(n, (b0 + grid) * tb)))
        b0 += launch_blocks
    return out


# ---- inputs of calls of more than one launch (tests/test_g_mul_launches_gpu.py): arrays, no group operation per lane --

def random_rows(seed, n, limbs=4):
    """n seeded random rows of `limbs` 64-bit limbs"""
    return np.frombuffer(np.random.default_rng(seed).bytes(8 * limbs * n), dtype=np.uint64).reshape(n, limbs).copy()


def edge_lanes(spans, n, offsets, rng, extra):
    """the lanes `offsets` away from every launch start, lane n - 1 and `extra` seeded lanes, those of [0, n) sorted"""
    lanes = {f + d for f, _ in spans for d in offsets} | {n - 1} | {rng.randrange(n) for _ in range(extra)}
    return sorted(i for i in lanes if 0 <= i < n)


def each_scalars(name, n, spans, seed):
    """(uint64[n, 4], the lanes that were overwritten): seeded 256-bit integers, NOT reduced, with 0, r, r - 1 and
    2^256 - 1 in turn at lanes first - 1, first, first + 1 of every launch, at n - 1 and at a few seeded lanes"""
    from kzg_snark_amd import _native
    r = C.CURVES[name].r
    k = random_rows(seed, n)
    lanes = edge_lanes(spans, n, (-1, 0, 1), random.Random(seed), 8)
    special = [0, r, r - 1, (1 << 256) - 1]
    k[lanes] = _native.ints_to_limbs([special[j % 4] for j in range(len(lanes))])
    return k, lanes


def rho_rows(seed, n):
    """n seeded random coefficients below 2^253 (below r on both curves) as canonical limbs"""
    rho = random_rows(seed, n)
    rho[:, 3] >>= np.uint64(3)
    return rho


@lru_cache(maxsize=None)
def g2_pool(name):
    """(8 points, 12 scalars, the 96 products, product of point a and scalar b at a * 12 + b): infinity, G, -G, three
    random points of the subgroup, the point outside the subgroup and the one of small prime order; 0, 1, the
    neighbourhood of r, 2r - 4, 2^256 - 1, 2^255 and four random 256-bit values"""
    cv, G = C.CURVES[name], group(name, 2)
    pts = [pt for pt, _ in points(name, 2)]
    what = [w for _, w in points(name, 2)]
    assert len(pts) == 8 and what[0] == "infinity" and what[6] == "outside the subgroup" and what[7].startswith("order ")
    rng = random.Random(0xc2 + CURVE_IDS[name])
    r = cv.r
    ks = [0, 1, r - 1, r, r + 1, 2 * r - 4, (1 << 256) - 1, 1 << 255] + [rng.getrandbits(256) for _ in range(4)]
    return pts, ks, [G.normalize(G.multiply(pt, k)) for pt in pts for k in ks]


def odd_order_scalar(name):
    """(s, m): s of odd multiplicative order m modulo r, so that s^i = s^(i mod m) and s^2048 has order m as well"""
    r = C.CURVES[name].r
    base, m = {"bls12_381": (2, 33), "bn254": (5, 39)}[name]
    assert (r - 1) % m == 0
    s = pow(base, (r - 1) // m, r)
    assert pow(s, m, r) == 1 and all(pow(s, m // q, r) != 1 for q in (3, 11, 13) if m % q == 0)
    assert m % 2 == 1 and math.gcd(2048, m) == 1
    return s, m


def shim_mul(lib, name, g, pt, k):
    """[k] pt through the shim -> (status, point)"""
    nw = fp_words(C.CURVES[name])
    n = 2 * g * nw
    out, out_inf = (U32 * n)(), ctypes.c_int(-1)
    st = lib.gm_mul(CURVE_IDS[name], g, (U32 * n)(*words(to_value(pt, g, nw), n)), int(is_inf(pt, g)),
                    (U32 * 8)(*words(k, 8)), out, ctypes.byref(out_inf))
    v = sum(int(w) << (32 * i) for i, w in enumerate(out))
    return st, from_value(v, bool(out_inf.value), g, nw)


def replay_file(path, lib):
    """the whole case list as the records g_mul_shim.cpp's main() replays; returns the number of cases"""
    total, count = lib.gm_case_words(), 0
    with open(path, "wb") as f:
        for name in CURVES:
            nw = fp_words(C.CURVES[name])
            for g in (1, 2):
                for pt, k, want, _ in cases(name, g):
                    rec = [CURVE_IDS[name], g, int(is_inf(pt, g))] + words(to_value(pt, g, nw), 48) + words(k, 8)
                    rec += [int(is_inf(want, g))] + words(to_value(want, g, nw), 48)
                    assert len(rec) == total
                    f.write(b"".join(w.to_bytes(4, "little") for w in rec))
                    count += 1
    return count

"""Shared helpers of the G2 linear-combination tests (a plain module, no fixtures): the host shim of csrc/g2_lincomb.h,
Jacobian points as the opaque limb rows that cross it, the wave sum and the fold of csrc/g2_lincomb.hip restated over
the shim's addition, the plan of a call restated in Python integers, and the lane pattern of the GPU size tests."""
import ctypes
import os
import subprocess
from functools import lru_cache

import g_mul_cases as gm
from g2_bytes_cases import CURVE_IDS, INF2, fp_words
from kzg_snark_amd import curve as C

SHIM_SRC = os.path.join(gm.SHIM_DIR, "g2_lincomb_shim.cpp")
U32 = ctypes.c_uint32
WAVE = 64


@lru_cache(maxsize=None)
def build_shim():
    so = os.path.join(gm.SHIM_DIR, "libg2_lincomb_shim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", SHIM_SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.gl_const.restype = ctypes.c_uint64
    return lib


def consts(lib):
    """(lanes per workgroup, lanes per launch, fold lanes, fold span, largest n, most fold levels) of csrc/g2_lincomb.h"""
    return tuple(int(lib.gl_const(i)) for i in range(6))


class Jac:
    """Jacobian points of one curve's twist through the shim: a point is a tuple of 6 N limbs"""

    def __init__(self, name):
        self.name, self.lib, self.id = name, build_shim(), CURVE_IDS[name]
        self.cv = C.CURVES[name]
        self.G = C.g2_group(self.cv)
        self.nw = fp_words(self.cv)
        self.limbs = self.lib.gl_point_limbs(self.id)
        assert self.limbs > 0

    def _arr(self, limbs):
        return (U32 * self.limbs)(*limbs)

    def lift(self, pt):
        """an affine point (a curve.py tuple, normalised here) -> Jacobian limbs with Z = 1, or infinity"""
        pt = self.G.normalize(pt)
        inf = gm.is_inf(pt, 2)
        out = (U32 * self.limbs)()
        st = self.lib.gl_from_affine(self.id, (U32 * (4 * self.nw))(*gm.words(gm.to_value(pt, 2, self.nw), 4 * self.nw)),
                                     int(inf), out)
        assert st == 0, st
        return tuple(out)

    def add(self, a, b):
        out = (U32 * self.limbs)()
        assert self.lib.gl_add(self.id, self._arr(a), self._arr(b), out) == 0
        return tuple(out)

    def rescale(self, a, lam):
        """the same point as (X l^2, Y l^3, Z l), 0 < l < p"""
        assert 0 < lam < self.cv.p
        out = (U32 * self.limbs)()
        assert self.lib.gl_rescale(self.id, self._arr(a), (U32 * self.nw)(*gm.words(lam, self.nw)), out) == 0
        return tuple(out)

    def affine(self, a):
        """Jacobian limbs -> the normalised curve.py tuple"""
        out, inf = (U32 * (4 * self.nw))(), ctypes.c_int(-1)
        assert self.lib.gl_to_affine(self.id, self._arr(a), out, ctypes.byref(inf)) == 0
        v = sum(int(w) << (32 * i) for i, w in enumerate(out))
        return gm.from_value(v, bool(inf.value), 2, self.nw)

    # ---- csrc/g2_lincomb.hip restated ---------------------------------------------------------------------------------
    def wave_sum(self, lanes):
        """gl_wave_sum: rounds s = 32 .. 1, lane t < s adds lane t + s; the sum is lane 0's"""
        lanes = list(lanes)
        assert len(lanes) == WAVE
        s = WAVE // 2
        while s >= 1:
            for t in range(s):
                lanes[t] = self.add(lanes[t], lanes[t + s])
            s //= 2
        return lanes[0]

    def fold_level(self, points, span):
        """one launch of g2_lincomb_fold_kernel: workgroup b adds points[b * span : (b + 1) * span], lane t the points
        lo + t, lo + t + 64, ..., then the wave sum"""
        inf = self.lift(INF2)
        out = []
        for lo in range(0, len(points), span):
            hi = min(len(points), lo + span)
            lanes = []
            for t in range(WAVE):
                acc = inf
                for b in range(lo + t, hi, WAVE):
                    acc = self.add(acc, points[b])
                lanes.append(acc)
            out.append(self.wave_sum(lanes))
        return out

    def fold(self, points, span):
        """every level of the fold down to one point (at least one level, as the driver launches them)"""
        levels = 0
        while levels == 0 or len(points) > 1:
            points = self.fold_level(points, span)
            levels += 1
        return points[0], levels


# ---- the plan -----------------------------------------------------------------------------------------------------------

def shim_plan(lib, name, n):
    """GlPlan of a call of n points -> dict"""
    levels_max = consts(lib)[5]
    out, vectors, partial_limbs = (U32 * (8 + levels_max + 1))(), ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.gl_plan(CURVE_IDS[name], ctypes.c_uint64(n), out, ctypes.byref(vectors), ctypes.byref(partial_limbs)) == 0
    v = [int(x) for x in out]
    w = 5 + levels_max + 1
    return dict(blocks=v[0], launch_blocks=v[1], launches=v[2], partials=v[3], levels=v[4], width=v[5:w], table_top=v[w],
                ok=bool(v[w + 1]), pieces=v[w + 2], vectors=vectors.value, partial_limbs=partial_limbs.value)


def shim_table_top(lib, name, grid):
    top = U32()
    assert lib.gl_table_top(CURVE_IDS[name], grid, ctypes.byref(top)) == 0
    return top.value


def widths_of(partials, span):
    """the points entering every level of the fold and, last, the one point leaving it ([] for no partials)"""
    if partials == 0:
        return []
    out = [partials]
    while len(out) == 1 or out[-1] > 1:
        out.append(-(-out[-1] // span))
    return out


# ---- the lanes of the GPU size tests ------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def lane_pool(name):
    """[(point, scalar, product)]: g_mul_cases' special scalars against G, a random point of the subgroup, the point
    outside the subgroup and the one of small prime order -- 92 host products"""
    G = gm.group(name, 2)
    pts = {w: pt for pt, w in gm.points(name, 2)}
    small = next(w for w in pts if w.startswith("order "))
    four = [pts["G"], pts["random subgroup point 0"], pts["outside the subgroup"], pts[small]]
    pool = [(pt, k, G.multiply(pt, k)) for k in gm.special_scalars(name) for pt in four]
    assert len(pool) <= 96
    return pool


def lanes_and_sum(name, n):
    """n lanes cycling over lane_pool -> (points, scalars, the expected sum): lane i holds pool entry i mod 92, so the
    sum is sum_j [count_j] product_j"""
    G = gm.group(name, 2)
    pool = lane_pool(name)
    pts = [pool[i % len(pool)][0] for i in range(n)]
    ks = [pool[i % len(pool)][1] for i in range(n)]
    acc = INF2
    for j, (_, _, prod) in enumerate(pool):
        count = len(range(j, n, len(pool)))
        if count:
            acc = G.add(acc, G.multiply(prod, count))
    return pts, ks, G.normalize(acc)

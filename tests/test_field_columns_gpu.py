"""The Fp381 multiplier's column schedule (field.h: plan_columns, the high-word cut) through the real MSM kernels.

tests/test_field_columns_host.py checks the schedule itself; here BLS12-381 commitments over imported keys
(kzg_srs_load_g1) whose coordinates carry the extreme limb patterns of tests/limb_patterns.py -- with negatives, exact
duplicates and points at infinity among the records, and r - 1, 1 and 0 among the scalars -- are compared with
oracle/kzg_oracle.c, bit for bit: once at 2^12 records (16-bit windows) and once at 2^18 + 5 (c = 20 and the 13-window
table, what the benchmark runs).

The oracle adds one double-and-add multiple per record, minutes at 2^18 records.  The large key therefore tiles 256
distinct points (sign flipping every 256 records), so that the commitment is sum_j k_j P_j with 256 INTEGER coefficients
k_j = sum +-s_i below 2^266 (the points are outside the r-torsion: nothing is reduced mod r).  The oracle's scalars have
256 bits, so |k_j| = a_j + 2^128 b_j + 2^256 c_j and the expected point is
commit(P, a) + commit(2^128 P, b) + commit(2^256 P, c), every multiple and every commit by oracle/kzg_oracle.c."""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import py_oracle as O
from test_limb_extremes_gpu import adversarial_points, got_point, load_key, neg, scalars

pytestmark = pytest.mark.gpu

CURVE = "bls12_381"


def plant(sc, r):
    """r - 1, 1 and 0 at fixed places (scalars() plants them too, at seeded ones)"""
    sc[0], sc[1], sc[2], sc[-1], sc[-2], sc[-3] = r - 1, 1, 0, r - 1, 0, 1
    return sc


def test_commit_2_12_over_extreme_limbs_against_the_c_oracle(native):
    cv = O.curve(CURVE)
    ctx = native.get_context(CURVE)
    pts = adversarial_points(CURVE, 256, 17)
    key = []
    for i in range(4096):
        pt = pts[(i * 7 + i // 256) % 256]
        key.append(neg(pt, cv) if (i // 128) % 2 else pt)
    for i in (3, 500, 501, 4095):
        key[i] = None                                            # points at infinity
    key[1000] = key[999] = key[998]                              # duplicates side by side
    srs, kxy, kinf = load_key(native, ctx, key)
    sc = plant(scalars(CURVE, 4096, 61), cv.r)
    sc[3], sc[998], sc[999], sc[1000] = cv.r - 1, cv.r - 1, cv.r - 1, 1
    raw = native.ints_to_limbs(sc)
    xy, inf = ctx.commit(srs, raw.reshape(1, 4096, 4), [4096], 4096)
    srs.close()
    wxy, winf = c_oracle.commit(CURVE, kxy, raw, kinf)
    assert int(inf[0]) == winf and (winf or np.array_equal(xy[0], wxy))


def test_commit_2_18_plus_5_over_extreme_limbs_against_the_c_oracle(native):
    cv = O.curve(CURVE)
    ctx = native.get_context(CURVE)
    n = (1 << 18) + 5
    pts = adversarial_points(CURVE, 256, 19)
    L = ctx.fp_limbs

    def rows(points):
        return np.ascontiguousarray(native.ints_to_limbs([c for pt in points for c in pt], L).reshape(len(points), 2 * L))
    base, nbase = rows(pts), rows([neg(pt, cv) for pt in pts])
    # records 0 .. 2^18 - 1: +-P_(i mod 256); the last five: infinity, +P_3, infinity, -P_7, +P_3
    tail = [(None, 0), (3, 1), (None, 0), (7, -1), (3, 1)]
    xy = np.concatenate([np.tile(np.concatenate([base, nbase]), ((1 << 18) // 512, 1)),
                         np.stack([np.zeros(2 * L, dtype=np.uint64) if j is None else (base if s > 0 else nbase)[j]
                                   for j, s in tail])])
    xy = np.ascontiguousarray(xy)
    kinf = np.zeros(n, dtype=np.uint8)
    kinf[[(1 << 18) + t for t, (j, _) in enumerate(tail) if j is None]] = 1
    assert xy.shape == (n, 2 * L)
    srs = ctx.srs_load_g1(xy, kinf)
    sc = plant(scalars(CURVE, n, 63), cv.r)                      # sc[-1] = r - 1 multiplies +P_3, sc[-3] = 1 an infinity
    raw = native.ints_to_limbs(sc)
    got_xy, got_inf = ctx.commit(srs, raw.reshape(1, n, 4), [n], n)
    srs.close()
    coeff = [0] * 256
    for i, s in enumerate(sc[:1 << 18]):
        coeff[i % 256] += -s if (i // 256) % 2 else s
    for (j, sign), s in zip(tail, sc[1 << 18:]):
        if j is not None:
            coeff[j] += sign * s
    assert max(abs(k) for k in coeff) < 1 << 266
    # |k_j| = a_j + 2^128 b_j + 2^256 c_j against P_j, 2^128 P_j, 2^256 P_j (the sign of k_j goes into the point)
    parts = []
    level = [(base if k >= 0 else nbase)[j] for j, k in enumerate(coeff)]
    level_inf = [0] * 256
    for shift in (0, 128, 256):
        digits = [(abs(k) >> shift) & ((1 << 128) - 1) for k in coeff]
        wxy, winf = c_oracle.commit(CURVE, np.ascontiguousarray(np.stack(level)), native.ints_to_limbs(digits),
                                    np.array(level_inf, dtype=np.uint8))
        parts.append(None if winf else tuple(native.limbs_to_ints(np.ascontiguousarray(wxy).reshape(2, L))))
        if shift < 256:
            nxt = [c_oracle.g1_mul(CURVE, np.ascontiguousarray(q), 1 << 128, bool(qi)) for q, qi in zip(level, level_inf)]
            level, level_inf = [q for q, _ in nxt], [qi for _, qi in nxt]
    want = O.Z1()
    for pt in parts:
        if pt is not None:
            want = O.add(want, O.from_affine(pt), cv)
    assert got_point(native, ctx, got_xy[0], got_inf[0]) == O.normalize(want, cv)

"""The adversarial operands of tests/limb_patterns.py through the REAL kernels, via the C ABI like every other GPU test.

tests/test_field_bounds_host.py pins the limb-level bounds of field.h / ec.h on the CPU; here the same limb images --
all-ones 29/30-bit limbs, values at the top of the canonical range -- reach the device code paths that the CPU shim can
only restate: the vector primitives and kzg_fr_poly_eval, the NTT (data AND a root whose Montgomery image w*R mod r has
adversarial limbs), the MSM on both window widths over keys of points whose Montgomery-form x has adversarial limbs,
one opening and one FK20 open_domain.  No tolerances: every comparison is integer equality with Python integers, the
oracle's group law or oracle/kzg_oracle.c.

The adversarial points lie on the curve but, for BLS12-381 (cofactor != 1), NOT in the r-torsion.  A commitment is a sum
of scalar multiples with the scalars taken as INTEGERS in [0, r) -- the oracle does exactly that -- so it is well defined
for them; expected values below never reduce a coefficient mod r after combining."""
import random

import numpy as np
import pytest

from limb_patterns import adversarial, header_layout
from oracle import c_oracle
from oracle import py_oracle as O

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
FR_STRUCT = {"bn254": "BnFr", "bls12_381": "BlsFr"}
FP_STRUCT = {"bn254": "BnFp", "bls12_381": "BlsFp"}
# cofactor of G1: BN254 has none; BLS12-381: (z - 1)^2 / 3 with z = -0xd201000000010000 (public parameter)
COFACTOR = {"bn254": 1, "bls12_381": 0x396c8c005555e1568c00aaab0000aaab}


def fr_patterns(curve, count, seed):
    """canonical scalars (< r) with adversarial 29-bit limb images"""
    L, N = header_layout(FR_STRUCT[curve])
    return adversarial(O.curve(curve).r, L, N, 1, count, seed)


def fr_vector(curve, n, seed):
    pats = fr_patterns(curve, 200, seed)
    rng = random.Random(seed)
    return [pats[i] if i < len(pats) and n >= len(pats) else rng.choice(pats) for i in range(n)]


def adversarial_points(curve, count, seed):
    """`count` distinct affine points whose Montgomery-form x (x * 2^(L*N) mod p, what the device keeps) has an adversarial
    limb image: x~ from the generator, x = x~ / R, kept if x^3 + b is a square (both p are 3 mod 4).  A candidate off the
    curve is rejected here, with a fixed seed -- construction, not a skipped case."""
    cv = O.curve(curve)
    p = cv.p
    assert p % 4 == 3
    L, N = header_layout(FP_STRUCT[curve])
    Rinv = pow(1 << (L * N), -1, p)
    out, seen = [], set()
    for xm in adversarial(p, L, N, 1, 4 * count + 100, seed):
        x = xm * Rinv % p
        v = (x * x * x + cv.b) % p
        y = pow(v, (p + 1) // 4, p)
        if y * y % p != v or y == 0 or x in seen:
            continue
        seen.add(x)
        out.append((x, y if len(out) % 2 else p - y))
        if len(out) == count:
            break
    assert len(out) == count
    assert all(O.is_on_curve(pt, cv) for pt in out)
    return out


def neg(pt, cv):
    return None if pt is None else (pt[0], (-pt[1]) % cv.p)


def load_key(native, ctx, pts):
    """list of affine points / None (infinity) -> (device key, xy array, inf array)"""
    L = ctx.fp_limbs
    flat = []
    for pt in pts:
        flat += [0, 0] if pt is None else [pt[0], pt[1]]
    xy = np.ascontiguousarray(native.ints_to_limbs(flat, L).reshape(len(pts), 2 * L))
    inf = np.array([1 if pt is None else 0 for pt in pts], dtype=np.uint8)
    return ctx.srs_load_g1(xy, inf), xy, inf


def oracle_pts(pts):
    return [O.Z1() if pt is None else O.from_affine(pt) for pt in pts]


def got_point(native, ctx, xy, inf):
    return None if inf else tuple(native.limbs_to_ints(np.ascontiguousarray(xy).reshape(2, ctx.fp_limbs)))


def scalars(curve, n, seed):
    """uniform over [0, r) with the digit-edge values of test_commit_2_20_with_extreme_coefficients and adversarial limb
    images planted"""
    r = O.curve(curve).r
    rng = random.Random(seed)
    vals = [rng.randrange(r) for _ in range(n)]
    half = sum(1 << (20 * j + 19) for j in range(13)) % r
    ones = sum(((1 << 20) - 1) << (20 * j) for j in range(13)) % r
    special = [r - 1, r - 2, r - (1 << 20), half, ones, (1 << 255) % r, ((1 << 255) - 1) % r, ((1 << 255) - 19) % r,
               (1 << 253), (1 << 253) - 1, 0, 1]
    special += [1 << (20 * j) for j in range(13) if (1 << (20 * j)) < r] + [(1 << (20 * j)) - 1 for j in range(1, 13)]
    special += [(1 << (20 * j + 19)) for j in range(12)] + [(1 << (16 * j + 15)) for j in range(15)]
    special += fr_patterns(curve, 40, seed)
    special = special[:max(1, n // 2)]
    for pos, v in zip(rng.sample(range(n), len(special)), special):
        vals[pos] = v
    return vals


# ---- vector primitives and kzg_fr_poly_eval ----------------------------------------------------------------

def dev(native, vals):
    import torch
    return torch.from_numpy(native.ints_to_limbs(vals).view(np.int64)).to("cuda:0")


def host(native, t):
    return native.limbs_to_ints(t.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 1000, 1025, 40000])
def test_vector_primitives_on_adversarial_limbs(native, curve, n):
    import torch
    r = O.curve(curve).r
    ctx = native.get_context(curve)
    a, b = fr_vector(curve, n, 1000 + n), fr_vector(curve, n, 2000 + n)[::-1]
    rng = random.Random(n)
    pats = fr_patterns(curve, 0, 0)
    da, db = dev(native, a), dev(native, b)
    out = torch.empty_like(da)
    for op, f in (("add", lambda x, y: (x + y) % r), ("sub", lambda x, y: (x - y) % r), ("mul", lambda x, y: x * y % r)):
        ctx.vec_op(op, n, da.data_ptr(), db.data_ptr(), out.data_ptr())
        ctx.synchronize()
        assert host(native, out) == [f(x, y) for x, y in zip(a, b)], op
    s, c0 = pats[1], pats[0]                               # all-ones limbs under the top limb of r - 1; r - 1
    ctx.vec_mul_powers(n, da.data_ptr(), s, c0, out.data_ptr())
    ctx.synchronize()
    want, pw = [], c0
    for x in a:
        want.append(x * pw % r)
        pw = pw * s % r
    assert host(native, out) == want
    ctx.vec_inverse(n, da.data_ptr(), out.data_ptr())
    ctx.synchronize()
    assert host(native, out) == [pow(x, -1, r) if x else 0 for x in a]
    ctx.vec_prefix_product(n, db.data_ptr(), out.data_ptr())
    ctx.synchronize()
    want, acc = [], 1
    for y in b:
        want.append(acc)
        acc = acc * y % r
    assert host(native, out) == want
    for z in (pats[1], pats[0], rng.choice(pats)):
        assert ctx.poly_eval(n, da.data_ptr(), z) == O.poly_eval(a, z, r), hex(z)
    c = fr_vector(curve, max(1, n // 2), 3000 + n)
    dc = dev(native, c)
    sc = [pats[1], pats[0], pats[4 % len(pats)]]
    ctx.vec_lincomb(n, [da.data_ptr(), db.data_ptr(), dc.data_ptr()], [n, n, len(c)], sc, out.data_ptr())
    ctx.synchronize()
    assert host(native, out) == [(sc[0] * a[i] + sc[1] * b[i] + sc[2] * (c[i] if i < len(c) else 0)) % r for i in range(n)]


# ---- NTT / INTT ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [12, 14])
def test_ntt_with_adversarial_data_and_root(native, curve, log_n):
    """2^12 is a single pass (12 lazy levels, reduce_wide / n^-1 epilogue), 2^14 two passes with the twist between them.
    The entry point takes ANY w and so does the recursion of fft_ff.py (oracle/kzg_oracle.c): w is chosen so that its
    Montgomery image w * 2^261 mod r -- the first twiddle the kernels multiply by -- has adversarial limbs."""
    cv = O.curve(curve)
    r = cv.r
    L, N = header_layout(FR_STRUCT[curve])
    Rinv = pow(1 << (L * N), -1, r)
    n = 1 << log_n
    pats = fr_patterns(curve, 300, 40 + log_n)
    rng = random.Random(50 + log_n)
    x = [pats[i % len(pats)] if i < 2 * len(pats) else rng.choice(pats) for i in range(n)]
    raw = native.ints_to_limbs(x)
    ctx = native.get_context(curve)
    for wm in (pats[1], pats[0], pats[-1]):
        w = wm * Rinv % r
        assert w not in (0, 1) and w * (1 << (L * N)) % r == wm
        for inverse in (False, True):
            got = raw.copy()
            ctx.ntt(got, log_n, native.int_to_words(w), inverse)
            want = raw.copy()
            c_oracle.fft(curve, want, w, inverse=inverse)
            assert np.array_equal(got, want), (curve, log_n, hex(wm), inverse)


# ---- MSM: both window widths ------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_commit_16_bit_windows_over_adversarial_keys(native, curve):
    """Keys below 2^18 points take 16-bit windows: 64 distinct adversarial points against the Python oracle's commit, the
    same with negatives, exact duplicates and an infinity record, and 4096 records (256 distinct points, their negatives,
    duplicates, one infinity) against oracle/kzg_oracle.c.  All loaded through kzg_srs_load_g1."""
    cv = O.curve(curve)
    ctx = native.get_context(curve)
    pts = adversarial_points(curve, 256, 7)
    key64 = pts[:64]
    mixed64 = list(pts[:40]) + [neg(pt, cv) for pt in pts[:12]] + pts[:6] + [None] + pts[40:45]
    assert len(mixed64) == 64
    for key in (key64, mixed64):
        srs, _, _ = load_key(native, ctx, key)
        polys = [scalars(curve, 64, 11), [cv.r - 1] * 64, fr_patterns(curve, 0, 0)[:64], [1] * 64,
                 scalars(curve, 17, 12)]
        arr = np.zeros((len(polys), 64, 4), dtype=np.uint64)
        for i, pl in enumerate(polys):
            arr[i, :len(pl)] = native.ints_to_limbs(pl)
        xy, inf = ctx.commit(srs, arr, [len(pl) for pl in polys], 64)
        want = O.commit(oracle_pts(key), polys, cv)
        for i in range(len(polys)):
            assert got_point(native, ctx, xy[i], inf[i]) == O.normalize(want[i], cv), i
        srs.close()
    rng = random.Random(13)
    key = []
    for i in range(4096):
        pt = pts[i % 256] if i < 2048 else rng.choice(pts)
        key.append(neg(pt, cv) if (i // 256) % 2 else pt)
    key[777] = None
    key[778] = key[776]
    srs, kxy, kinf = load_key(native, ctx, key)
    for seed in (21, 22):
        sc = scalars(curve, 4096, seed)
        raw = native.ints_to_limbs(sc)
        xy, inf = ctx.commit(srs, raw.reshape(1, 4096, 4), [4096], 4096)
        wxy, winf = c_oracle.commit(curve, kxy, raw, kinf)
        assert int(inf[0]) == winf and (winf or np.array_equal(xy[0], wxy)), seed
    srs.close()


@pytest.mark.parametrize("curve", CURVES)
def test_commit_20_bit_windows_over_a_tiled_adversarial_key(native, curve):
    """Keys of 2^18 points and more take 20-bit windows.  The key tiles 256 distinct adversarial points with alternating
    sign (record i = +-P_(i mod 256), the sign flipping every 256 records), so every bucket fills with P + P and P - P
    collisions.  Expected: sum_j (sum_(i = j mod 256) +-s_i) P_j, 256 scalar multiplications by the Python oracle with the
    INTEGER coefficient (not reduced mod r: on BLS12-381 the points are outside the r-torsion)."""
    cv = O.curve(curve)
    ctx = native.get_context(curve)
    n = 1 << 18
    pts = adversarial_points(curve, 256, 9)
    L = ctx.fp_limbs
    base = np.ascontiguousarray(native.ints_to_limbs([c for pt in pts for c in pt], L).reshape(256, 2 * L))
    nbase = np.ascontiguousarray(native.ints_to_limbs([c for pt in pts for c in neg(pt, cv)], L).reshape(256, 2 * L))
    xy = np.ascontiguousarray(np.tile(np.concatenate([base, nbase]), (n // 512, 1)))
    assert xy.shape == (n, 2 * L)
    srs = ctx.srs_load_g1(xy, np.zeros(n, dtype=np.uint8))
    sc = scalars(curve, n, 31)
    raw = native.ints_to_limbs(sc)
    got_xy, got_inf = ctx.commit(srs, raw.reshape(1, n, 4), [n], n)
    srs.close()
    coeff = [0] * 256
    for i, s in enumerate(sc):
        coeff[i % 256] += -s if (i // 256) % 2 else s
    acc = O.Z1()
    for pt, k in zip(pts, coeff):
        acc = O.add(acc, O.multiply(O.from_affine(pt if k >= 0 else neg(pt, cv)), abs(k), cv), cv)
    assert got_point(native, ctx, got_xy[0], got_inf[0]) == O.normalize(acc, cv)


# ---- one opening and one open_domain over the adversarial key -----------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_open_over_the_adversarial_key(native, curve):
    cv = O.curve(curve)
    r = cv.r
    ctx = native.get_context(curve)
    key = adversarial_points(curve, 64, 7)
    srs, _, _ = load_key(native, ctx, key)
    pats = fr_patterns(curve, 0, 0)
    polys = [scalars(curve, 64, 41), fr_vector(curve, 40, 42), [r - 1] * 7]
    arr = np.zeros((len(polys), 64, 4), dtype=np.uint64)
    for i, pl in enumerate(polys):
        arr[i, :len(pl)] = native.ints_to_limbs(pl)
    for z, xi in ((pats[1], pats[0]), (pats[0], pats[1])):
        xy, inf, ev = ctx.open(srs, arr, [len(pl) for pl in polys], 64, native.int_to_words(z), native.int_to_words(xi))
        want, pz = O.open_(oracle_pts(key), polys, z, xi, cv)
        assert native.limbs_to_ints(ev.reshape(1, 4))[0] == pz
        assert got_point(native, ctx, xy, inf[0]) == O.normalize(want, cv)
    srs.close()


@pytest.mark.parametrize("curve", CURVES)
def test_open_domain_over_the_adversarial_key(native, curve):
    """All 64 FK20 proofs against the oracle's opening at each w^i: the commitment (oracle/kzg_oracle.c) of the quotient
    (p(X) - p(w^i)) / (X - w^i).  FK20 transforms the key's points with scalars that are only defined mod r, so proofs
    are comparable only for points of order r: the BN254 key is used as it is (cofactor 1); the BLS12-381 points are
    multiplied by the cofactor first (the oracle's multiply), the polynomial keeps its adversarial limbs."""
    cv = O.curve(curve)
    r = cv.r
    ctx = native.get_context(curve)
    n, log_n = 64, 6
    key = adversarial_points(curve, n + 16, 7)
    if COFACTOR[curve] != 1:
        # x~ = 0 is one of the patterns: (0, 2) has order 3 on y^2 = x^3 + 4 and goes to infinity here; it is left out
        key = [O.normalize(O.multiply(O.from_affine(pt), COFACTOR[curve], cv), cv) for pt in key]
        key = [pt for pt in key if pt is not None]
        assert all(O.multiply(O.from_affine(pt), r, cv)[2] == 0 for pt in key[:4])
    key = key[:n]
    assert len(key) == n
    srs, kxy, kinf = load_key(native, ctx, key)
    table = ctx.domain_table(srs, log_n)
    poly = fr_vector(curve, n, 51)
    w = cv.root_of_unity(n)
    xy, inf, ev = ctx.open_domain(table, native.ints_to_limbs(poly).reshape(1, n, 4), [n], n, w)
    evals = native.limbs_to_ints(ev.reshape(n, 4))
    for i in range(n):
        z = pow(w, i, r)
        quot, pz = O.poly_divide_linear(poly, z, r)
        assert evals[i] == pz, i
        wxy, winf = c_oracle.commit(curve, kxy, native.ints_to_limbs(quot).reshape(-1, 4), kinf)
        assert int(inf[0, i]) == winf and (winf or np.array_equal(xy[0, i], wxy)), i
    table.close()
    srs.close()

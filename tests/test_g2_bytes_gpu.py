"""GPU tests of compressed G2 points and subgroup checks on the twist (csrc/g2_bytes.hip through the C ABI and the
facade).  Every expected byte, point and verdict comes from kzg_snark_amd/curve.py's single-point helpers ([r] Q = O
for membership) or from the golden file.  The kernels run one wave per workgroup, so a wave's edge is a workgroup's:
sizes 63 / 64 / 65 straddle one, 255 / 256 / 257 the fourth."""
import ctypes

import numpy as np
import pytest

from g2_bytes_cases import INF2, g2_generator, golden_failures, golden_points, golden_real_rhs, subgroup_matrix_g2
from kzg_snark_amd import curve as C

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
GUARD = 0xA5
PAD = 192                     # guard bytes behind every output
EDGES = (0, 63, 64, 255, 256)


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


_BASE = {}


def base_points(kzg, native):
    """257 points P_i = P_(i-1) + D of G2 as (xy, tuples, blobs): y of either sign (asserted), blobs from curve.py"""
    if kzg.curve_type not in _BASE:
        cv = kzg._cv
        G = kzg._g2
        g = g2_generator(cv)
        d = G.multiply(g, 0x5eed_0bad_cafe)
        pts = [G.multiply(g, 0x1234_5678_9abc_def1)]
        for _ in range(256):
            pts.append(G.add(pts[-1], d))
        assert {C._fp2_larger(p[1], cv.p) for p in pts} == {True, False}
        xy, inf = native.g2_points_to_limbs(pts, kzg._context().fp_limbs)
        assert not inf.any()
        _BASE[kzg.curve_type] = (xy, pts, [C.compress_g2(p, cv) for p in pts])
    return _BASE[kzg.curve_type]


def batch(kzg, native, n):
    """n points with infinities at both ends of a wave (= a workgroup): (xy, inf, tuples, blobs)"""
    cv = kzg._cv
    xy, pts, blobs = base_points(kzg, native)
    xy, pts, blobs = xy[:n].copy(), list(pts[:n]), list(blobs[:n])
    inf = np.zeros(n, dtype=np.uint8)
    for i in EDGES + (n - 1,):
        if i < n and n > 1:
            inf[i] = 1
            xy[i] = 0
            pts[i] = INF2
            blobs[i] = C.compress_g2(INF2, cv)
    return xy, inf, pts, blobs


def guarded(nbytes):
    return np.full(nbytes + PAD, GUARD, dtype=np.uint8)


def guard_ok(a, nbytes):
    return bool((a[nbytes:] == GUARD).all())


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def g2_rows(native, pts, L):
    return native.g2_points_to_limbs(pts, L)


# ---- round trips -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_round_trip_with_guards_and_the_device_form(kzgs, native, curve, n):
    import torch
    kzg = kzgs[curve]
    ctx = kzg._context()
    L, size = ctx.fp_limbs, ctx.g2_bytes
    assert size == C.g2_compressed_size(kzg._cv)
    lib = native.lib()
    xy, inf, pts, blobs = batch(kzg, native, n)
    want_bytes = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    out = guarded(n * size)
    assert lib.kzg_g2_compress(ctx._h, vp(xy), vp(inf), n, vp(out)) == 0
    assert (out[:n * size] == want_bytes).all() and guard_ok(out, n * size)
    assert kzg.compress_g2(pts) == blobs and kzg.compress_g2((xy, inf)) == blobs
    for check in (1, 0):
        o_xy, o_inf, o_st = guarded(n * 4 * L * 8), guarded(n), guarded(n)
        assert lib.kzg_g2_decompress(ctx._h, vp(out), n, check, vp(o_xy), vp(o_inf), vp(o_st)) == 0
        assert guard_ok(o_xy, n * 4 * L * 8) and guard_ok(o_inf, n) and guard_ok(o_st, n)
        assert not o_st[:n].any()
        assert (o_inf[:n] == inf).all()
        assert (o_xy[:n * 4 * L * 8].view(np.uint64).reshape(n, 4 * L) == xy).all()
    o_st = guarded(n)
    assert lib.kzg_g2_check_subgroup(ctx._h, vp(xy), vp(inf), n, vp(o_st)) == 0
    assert not o_st[:n].any() and guard_ok(o_st, n)
    assert kzg.decompress_g2(blobs) == pts
    assert kzg.in_subgroup_g2(pts).all() and kzg.in_subgroup_g2((xy, inf)).all()
    # the device form: the same bytes out of device buffers, guards behind them intact
    dev = f"cuda:{ctx.device}"
    d_in = torch.from_numpy(want_bytes.copy()).to(dev)
    d_xy, d_inf, d_st = (torch.from_numpy(guarded(k)).to(dev) for k in (n * 4 * L * 8, n, n))
    torch.cuda.synchronize(ctx.device)
    ctx.g2_decompress_device(d_in.data_ptr(), n, True, d_xy.data_ptr(), d_inf.data_ptr(), d_st.data_ptr())
    ctx.synchronize()
    h_xy, h_inf, h_st = d_xy.cpu().numpy(), d_inf.cpu().numpy(), d_st.cpu().numpy()
    o_xy, o_inf, o_st = guarded(n * 4 * L * 8), guarded(n), guarded(n)
    assert lib.kzg_g2_decompress(ctx._h, vp(out), n, 1, vp(o_xy), vp(o_inf), vp(o_st)) == 0
    assert (h_xy == o_xy).all() and (h_inf == o_inf).all() and (h_st == o_st).all()


def test_sizes_and_arguments(kzgs, native):
    for curve in CURVES:
        kzg = kzgs[curve]
        ctx = kzg._context()
        lib = native.lib()
        L, size = ctx.fp_limbs, ctx.g2_bytes
        one = np.zeros(4 * size, dtype=np.uint8)
        assert lib.kzg_g2_compress(ctx._h, vp(one), None, 0, vp(one)) == 0
        assert lib.kzg_g2_decompress(ctx._h, vp(one), 0, 1, vp(one), vp(one), vp(one)) == 0
        assert lib.kzg_g2_decompress_device(ctx._h, vp(one), 0, 1, vp(one), vp(one), vp(one)) == 0
        assert lib.kzg_g2_check_subgroup(ctx._h, vp(one), None, 0, vp(one)) == 0
        assert kzg.compress_g2([]) == [] and kzg.decompress_g2([]) == [] and kzg.in_subgroup_g2([]).size == 0
        big = (1 << 24) + 1
        assert lib.kzg_g2_compress(ctx._h, vp(one), None, big, vp(one)) == -1
        assert lib.kzg_g2_decompress(ctx._h, vp(one), big, 1, vp(one), vp(one), vp(one)) == -1
        assert lib.kzg_g2_decompress_device(ctx._h, vp(one), big, 1, vp(one), vp(one), vp(one)) == -1
        assert lib.kzg_g2_check_subgroup(ctx._h, vp(one), None, big, vp(one)) == -1
        cv = kzg._cv
        g = g2_generator(cv)
        off = (g[0], ((g[1][0] + 1) % cv.p, g[1][1]), g[2])
        with pytest.raises(ValueError):
            kzg.compress_g2([g, off])
        bad = native.ints_to_limbs([g[0][0] + cv.p, g[0][1], g[1][0], g[1][1]], L).reshape(1, 4 * L)
        with pytest.raises(native.NativeError) as e:
            ctx.g2_compress(np.ascontiguousarray(bad))
        assert e.value.code == -1
        assert kzg.compress_g2([g]) == [C.compress_g2(g, cv)]                      # the context is still usable
        rows = np.concatenate([bad, g2_rows(native, [off, g], L)[0]])
        assert list(ctx.g2_check_subgroup(rows)) == [2, 2, 0]
        with pytest.raises(ValueError, match="expected %d" % size):
            kzg.decompress_g2([b"\x00" * (size - 1)])


# ---- status cases ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_every_status_case_at_the_edges_of_a_wave(kzgs, native, curve):
    kzg = kzgs[curve]
    cv = kzg._cv
    ctx = kzg._context()
    L, size = ctx.fp_limbs, ctx.g2_bytes
    n = 257
    xy, inf, pts, blobs = batch(kzg, native, n)
    lanes = (0, 63, 64, n - 1)
    fails = golden_failures(curve)
    assert {st for _, st, _ in fails} == {1, 2, 3}
    assert [c for _, st, c in fails if st == 1 and "first failure wins" in c]
    for blob, st, case in fails:
        mixed = list(blobs)
        for i in lanes:
            mixed[i] = blob
        arr = np.frombuffer(b"".join(mixed), dtype=np.uint8).reshape(n, size)
        for check in (True, False):
            got_xy, got_inf, got_st = ctx.g2_decompress(arr, check)
            unchecked = C.decompress_g2_status(blob, cv, check_subgroup=False)
            want_st = st if check or st != 3 else 0
            want_xy, want_inf = xy.copy(), inf.copy()
            for i in lanes:
                want_inf[i] = 0
                want_xy[i] = 0 if want_st else g2_rows(native, [unchecked[0]], L)[0][0]
            want_status = np.zeros(n, dtype=np.uint8)
            want_status[list(lanes)] = want_st
            assert (got_st == want_status).all(), (case, check)
            assert (got_xy == want_xy).all() and (got_inf == want_inf).all(), (case, check)     # neighbours untouched
    blob, st, case = fails[0]
    mixed = list(blobs)
    for i in lanes:
        mixed[i] = blob
    with pytest.raises(ValueError, match=r"point 0\b"):
        kzg.decompress_g2(mixed)
    points, status = kzg.decompress_g2(mixed, strict=False)
    assert [i for i, p in enumerate(points) if p is None] == sorted(lanes) and list(np.flatnonzero(status)) == sorted(lanes)
    assert [p for i, p in enumerate(points) if i not in lanes] == [p for i, p in enumerate(pts) if i not in lanes]
    mixed = list(blobs)
    mixed[200] = fails[-1][0]
    with pytest.raises(ValueError, match=r"point 200\b.*subgroup"):
        kzg.decompress_g2(mixed)
    assert kzg.decompress_g2(mixed, check_subgroup=False)[200] == C.decompress_g2(fails[-1][0], cv, check_subgroup=False)
    for blob, pt in golden_points(curve):
        assert kzg.decompress_g2([blob]) == [pt] and kzg.compress_g2([pt]) == [blob]
    for blob, pt, kind in golden_real_rhs(curve):                # the special branches of the square root
        assert kzg.decompress_g2([blob], check_subgroup=False) == [pt], kind
        assert kzg.compress_g2([pt]) == [blob]


# ---- subgroup membership ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_subgroup_matrix(kzgs, native, curve):
    kzg = kzgs[curve]
    cv = kzg._cv
    rows = subgroup_matrix_g2(curve)
    pts = [pt for pt, _, _ in rows]
    want = np.array([ok for _, ok, _ in rows])
    assert (~want).sum() >= 48 and want.sum() >= 17
    assert (kzg.in_subgroup_g2(pts) == want).all()
    blobs = [C.compress_g2(pt, cv) for pt in pts]
    assert kzg.compress_g2(pts) == blobs                         # compress asks for a point of the twist, no more
    points, status = kzg.decompress_g2(blobs, strict=False)
    assert (status == np.where(want, 0, 3)).all()
    assert points == [pt if ok else None for pt, ok in zip(pts, want)]
    points, status = kzg.decompress_g2(blobs, check_subgroup=False, strict=False)
    assert not status.any() and points == pts


# ---- pairing checks that test membership first ---------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_pairing_check_with_subgroup_test(kzgs, native, curve):
    kzg = kzgs[curve]
    cv = kzg._cv
    a, b = 0x1234567, 0x89abcde
    q = kzg.multiply(kzg.G2, b)
    honest = [(kzg.multiply(kzg.G1, a), q), (kzg.neg(kzg.multiply(kzg.G1, a * b)), kzg.G2)]
    wrong = [(kzg.multiply(kzg.G1, a + 1), q), honest[1]]
    t = next(pt for pt, ok, what in subgroup_matrix_g2(curve) if what.startswith("T"))
    tampered = [(honest[0][0], kzg._g2.add(q, t)), honest[1]]
    assert kzg.pairing_check(honest) is True and kzg.pairing_check(honest, check_subgroup=True) is True
    assert kzg.pairing_check(wrong) is False and kzg.pairing_check(wrong, check_subgroup=True) is False
    assert kzg.pairing_check([honest, wrong], check_subgroup=True) == [True, False]
    assert kzg.pairing_product(honest, check_subgroup=True) == kzg.pairing_product(honest)
    # the default path: no membership test, the verdict it gave before (a bool, no exception)
    assert kzg.pairing_check(tampered) in (True, False)
    assert kzg.pairing_check(tampered) == kzg.pairing_check(tampered, check_subgroup=False)
    with pytest.raises(ValueError, match=r"equation 0, pair 0: the G2 point is outside"):
        kzg.pairing_check(tampered, check_subgroup=True)
    with pytest.raises(ValueError, match=r"equation 1, pair 0: the G2 point is outside"):
        kzg.pairing_check([honest, tampered], check_subgroup=True)
    with pytest.raises(ValueError, match=r"equation 0, pair 0: the G2 point is outside"):
        kzg.pairing_product(tampered, check_subgroup=True)
    if curve == "bls12_381":                                     # a G1 point outside G1: (0, 2) has order 3
        with pytest.raises(ValueError, match=r"equation 0, pair 1: the G1 point is outside"):
            kzg.pairing_check([honest[0], ((0, 2, 1), kzg.G2)], check_subgroup=True)
        assert kzg.pairing_check([honest[0], ((0, 2, 1), kzg.G2)]) in (True, False)


# ---- profiling ----------------------------------------------------------------------------------------------------------

def test_one_span_per_call(kzgs, native):
    kzg = kzgs["bls12_381"]
    ctx = kzg._context()
    xy, inf, pts, blobs = batch(kzg, native, 65)
    arr = np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(65, ctx.g2_bytes)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for check in (True, False):
            ctx.g2_decompress(arr, check)
        for _ in range(3):
            ctx.g2_check_subgroup(xy, inf)
        ms, count = ctx.prof_read("g2_decompress")
        assert count == 2 and ms > 0
        ms, count = ctx.prof_read("g2_subgroup")
        assert count == 3 and ms > 0
    finally:
        ctx.prof_enable(False)

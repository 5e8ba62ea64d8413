"""GPU tests of compressed G1 points and subgroup checks (csrc/g1_bytes.hip through the C ABI and the facade).  Every
expected byte, point and verdict comes from kzg_snark_amd/curve.py's single-point helpers ([r] P = O for membership)
or from the golden file; sizes straddle a wave (63 / 64 / 65) and a workgroup (255 / 256 / 257)."""
import ctypes
import random

import numpy as np
import pytest

from g1_bytes_cases import golden_failures, golden_points, random_curve_point, subgroup_matrix
from kzg_snark_amd import curve as C

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x7a11_5eed_0bad_cafe_1234_5678_9abc
GUARD = 0xA5
PAD = 192                     # guard bytes behind every output


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


_BASE = {}


def base_points(kzg, native):
    """257 points [tau^i] G as (xy, inf, tuples, blobs): y of either sign (asserted), expected blobs from curve.py"""
    if kzg.curve_type not in _BASE:
        cv = kzg._cv
        ck, _ = kzg.setup(256, tau=TAU)
        xy, inf = ck.srs.export()
        pts = native.limbs_to_points(xy, inf)
        assert {p[1] > (cv.p - 1) // 2 for p in pts} == {True, False}
        _BASE[kzg.curve_type] = (xy, pts, [C.compress_g1(p, cv) for p in pts])
    return _BASE[kzg.curve_type]


def batch(kzg, native, n):
    """n points with infinities at both ends of a wave and of a workgroup: (xy, inf, tuples, blobs)"""
    cv = kzg._cv
    xy, pts, blobs = base_points(kzg, native)
    xy, pts, blobs = xy[:n].copy(), list(pts[:n]), list(blobs[:n])
    inf = np.zeros(n, dtype=np.uint8)
    for i in (0, 63, 64, 255, 256, n - 1):
        if i < n and n > 1:
            inf[i] = 1
            xy[i] = 0
            pts[i] = (1, 1, 0)
            blobs[i] = C.compress_g1((1, 1, 0), cv)
    return xy, inf, pts, blobs


def guarded(nbytes):
    a = np.full(nbytes + PAD, GUARD, dtype=np.uint8)
    return a


def guard_ok(a, nbytes):
    return bool((a[nbytes:] == GUARD).all())


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- round trips -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_round_trip_with_guards_and_the_device_form(kzgs, native, curve, n):
    import torch
    kzg = kzgs[curve]
    ctx = kzg._context()
    L, size = ctx.fp_limbs, ctx.g1_bytes
    assert size == C.g1_compressed_size(kzg._cv)
    lib = native.lib()
    xy, inf, pts, blobs = batch(kzg, native, n)
    want_bytes = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    # compress: byte for byte what curve.py writes, nothing behind the output touched
    out = guarded(n * size)
    assert lib.kzg_g1_compress(ctx._h, vp(xy), vp(inf), n, vp(out)) == 0
    assert (out[:n * size] == want_bytes).all() and guard_ok(out, n * size)
    assert kzg.compress_g1(pts) == blobs and kzg.compress_g1((xy, inf)) == blobs
    # decompress(compress(P)) == P, every status 0, guards intact
    for check in (1, 0):
        o_xy, o_inf, o_st = guarded(n * 2 * L * 8), guarded(n), guarded(n)
        assert lib.kzg_g1_decompress(ctx._h, vp(out), n, check, vp(o_xy), vp(o_inf), vp(o_st)) == 0
        assert guard_ok(o_xy, n * 2 * L * 8) and guard_ok(o_inf, n) and guard_ok(o_st, n)
        assert not o_st[:n].any()
        assert (o_inf[:n] == inf).all()
        assert (o_xy[:n * 2 * L * 8].view(np.uint64).reshape(n, 2 * L) == xy).all()
    assert kzg.decompress_g1(blobs) == pts
    assert kzg.in_subgroup(pts).all() and kzg.in_subgroup((xy, inf)).all()
    # the device form: the same bytes out of device buffers, guards behind them intact
    dev = f"cuda:{ctx.device}"
    d_in = torch.from_numpy(want_bytes.copy()).to(dev)
    d_xy, d_inf, d_st = (torch.from_numpy(guarded(k)).to(dev) for k in (n * 2 * L * 8, n, n))
    torch.cuda.synchronize(ctx.device)
    ctx.g1_decompress_device(d_in.data_ptr(), n, True, d_xy.data_ptr(), d_inf.data_ptr(), d_st.data_ptr())
    ctx.synchronize()
    h_xy, h_inf, h_st = d_xy.cpu().numpy(), d_inf.cpu().numpy(), d_st.cpu().numpy()
    assert (h_xy == o_xy).all() and (h_inf == o_inf).all() and (h_st == o_st).all()


def test_sizes_and_arguments(kzgs, native):
    for curve in CURVES:
        kzg = kzgs[curve]
        ctx = kzg._context()
        lib = native.lib()
        L, size = ctx.fp_limbs, ctx.g1_bytes
        one = np.zeros(4 * size, dtype=np.uint8)
        # n = 0: nothing to do;  more than 2^24 points: refused before anything is read
        assert lib.kzg_g1_compress(ctx._h, vp(one), None, 0, vp(one)) == 0
        assert lib.kzg_g1_decompress(ctx._h, vp(one), 0, 1, vp(one), vp(one), vp(one)) == 0
        assert lib.kzg_g1_check_subgroup(ctx._h, vp(one), None, 0, vp(one)) == 0
        assert kzg.compress_g1([]) == [] and kzg.decompress_g1([]) == [] and kzg.in_subgroup([]).size == 0
        big = (1 << 24) + 1
        assert lib.kzg_g1_compress(ctx._h, vp(one), None, big, vp(one)) == -1
        assert lib.kzg_g1_decompress(ctx._h, vp(one), big, 1, vp(one), vp(one), vp(one)) == -1
        assert lib.kzg_g1_check_subgroup(ctx._h, vp(one), None, big, vp(one)) == -1
        h = ctypes.c_void_p()
        assert lib.kzg_srs_load_g1_compressed(ctx._h, vp(one), big, 1, ctypes.byref(h)) == -1 and not h.value
        # compress validates like kzg_verify_cosets: off the curve or a coordinate >= p is an argument error
        cv = kzg._cv
        g = (cv.g1[0], cv.g1[1], 1)
        with pytest.raises(ValueError):
            kzg.compress_g1([g, (g[0], (g[1] + 1) % cv.p, 1)])
        bad = native.ints_to_limbs([g[0] + cv.p, g[1]], L).reshape(1, 2 * L)
        with pytest.raises(native.NativeError) as e:
            ctx.g1_compress(np.ascontiguousarray(bad))
        assert e.value.code == -1
        assert kzg.compress_g1([g]) == [C.compress_g1(g, cv)]                      # the context is still usable
        # kzg_g1_check_subgroup reports such input as status 2
        st = ctx.g1_check_subgroup(np.concatenate([bad, native.ints_to_limbs([g[0], g[1] ^ 1], L).reshape(1, 2 * L),
                                                   native.ints_to_limbs([g[0], g[1]], L).reshape(1, 2 * L)]))
        assert list(st) == [2, 2, 0]


# ---- status cases ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_every_status_case_at_the_edges_of_a_wave_and_a_workgroup(kzgs, native, curve):
    kzg = kzgs[curve]
    cv = kzg._cv
    ctx = kzg._context()
    L, size = ctx.fp_limbs, ctx.g1_bytes
    n = 257
    xy, inf, pts, blobs = batch(kzg, native, n)
    lanes = (0, 63, 64, n - 1)
    fails = golden_failures(curve)
    assert {st for _, st, _ in fails} == ({1, 2, 3} if curve == "bls12_381" else {1, 2})
    first = [c for _, st, c in fails if st == 1 and "not a square" in c]
    assert first, "the case where bad encoding must win over a non-residue"
    for blob, st, case in fails:
        mixed = list(blobs)
        for i in lanes:
            mixed[i] = blob
        arr = np.frombuffer(b"".join(mixed), dtype=np.uint8).reshape(n, size)
        for check in (True, False):
            got_xy, got_inf, got_st = ctx.g1_decompress(arr, check)
            unchecked = C.decompress_g1_status(blob, cv, check_subgroup=False)
            want_st = st if check or st != 3 else 0
            want_xy, want_inf = xy.copy(), inf.copy()
            for i in lanes:
                want_inf[i] = 0
                want_xy[i] = 0 if want_st else native.ints_to_limbs(list(unchecked[0][:2]), L).reshape(-1)
            want_status = np.zeros(n, dtype=np.uint8)
            want_status[list(lanes)] = want_st
            assert (got_st == want_status).all(), (case, check)
            assert (got_xy == want_xy).all() and (got_inf == want_inf).all(), (case, check)     # neighbours untouched
        with pytest.raises(ValueError, match=r"point 0\b"):
            kzg.decompress_g1(mixed)
        points, status = kzg.decompress_g1(mixed, strict=False)
        assert [i for i, p in enumerate(points) if p is None] == sorted(lanes) and list(np.flatnonzero(status)) == sorted(lanes)
        assert [p for i, p in enumerate(points) if i not in lanes] == [p for i, p in enumerate(pts) if i not in lanes]
    # the first bad index is the one the facade names
    mixed = list(blobs)
    mixed[200] = fails[0][0]
    with pytest.raises(ValueError, match=r"point 200\b"):
        kzg.decompress_g1(mixed)
    for blob, pt in golden_points(curve):
        assert kzg.decompress_g1([blob]) == [pt] and kzg.compress_g1([pt]) == [blob]


# ---- subgroup membership ----------------------------------------------------------------------------------------------

def test_subgroup_matrix_bls12_381(kzgs, native):
    kzg = kzgs["bls12_381"]
    cv = kzg._cv
    rows = subgroup_matrix()
    pts = [pt for pt, _, _ in rows]
    want = np.array([ok for _, ok, _ in rows])
    assert (~want).sum() >= 16 and want.sum() >= 16
    assert (kzg.in_subgroup(pts) == want).all()
    blobs = [C.compress_g1(pt, cv) for pt in pts]
    assert kzg.compress_g1(pts) == blobs                         # compress asks for a point of the curve, no more
    points, status = kzg.decompress_g1(blobs, check_subgroup=True, strict=False)
    assert (status == np.where(want, 0, 3)).all()
    assert points == [pt if ok else None for pt, ok in zip(pts, want)]
    points, status = kzg.decompress_g1(blobs, check_subgroup=False, strict=False)
    assert not status.any() and points == pts                    # every point of the curve is accepted
    assert kzg.decompress_g1(blobs, check_subgroup=False) == pts
    order3 = C.compress_g1((0, 2, 1), cv)
    assert order3 == bytes([0x80]) + bytes(47)                   # x = 0: only the flags are set
    with pytest.raises(ValueError, match="subgroup"):
        kzg.decompress_g1([order3])


def test_bn254_every_point_of_the_curve_passes(kzgs, native):
    kzg = kzgs["bn254"]
    cv = kzg._cv
    rng = random.Random(3)
    pts = [random_curve_point(cv, rng) for _ in range(16)] + [(1, 1, 0)]
    assert kzg.in_subgroup(pts).all()
    blobs = [C.compress_g1(p, cv) for p in pts]
    points, status = kzg.decompress_g1(blobs, check_subgroup=True, strict=False)
    assert not status.any() and points == pts


# ---- keys ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_compressed_key_files(kzgs, native, curve, tmp_path):
    kzg = kzgs[curve]
    cv = kzg._cv
    ctx = kzg._context()
    size = ctx.g1_bytes
    rng = random.Random(17)
    ck, _ = kzg.setup(max_degree=300, tau=TAU + 1)
    n = len(ck)
    assert n == 301
    path2, path1 = str(tmp_path / "key.v2"), str(tmp_path / "key.v1")
    kzg.save_key(ck, path2, compressed=True)
    kzg.save_key(ck, path1)
    raw = open(path2, "rb").read()
    assert raw[:8] == b"KZGSRS2\0" and len(raw) == 24 + n * size and raw[8:24] == open(path1, "rb").read()[8:24]
    xy, inf = ck.srs.export()
    want_blobs = b"".join(C.compress_g1(p, cv) for p in native.limbs_to_points(xy, inf))
    assert raw[24:] == want_blobs
    assert ck.srs.export_compressed(7, 3).tobytes() == want_blobs[7 * size:10 * size]
    poly = [rng.randrange(cv.r) for _ in range(n)]
    want_commit = kzg.commit(ck, [poly])
    for path in (path2, path1):                                 # a version-1 file still loads
        back = kzg.load_key(path)
        bxy, binf = back.srs.export()
        assert (bxy == xy).all() and (binf == inf).all()
        assert kzg.commit(back, [poly]) == want_commit
        back.srs.close()
    # one byte of point 257's x flipped so that the point no longer decompresses: load_key names the index
    body = bytearray(raw)
    at = 24 + 257 * size + size - 1
    for delta in range(1, 256):
        body[at] = raw[at] ^ delta
        status = C.decompress_g1_status(bytes(body[24 + 257 * size:24 + 258 * size]), cv)[1]
        if status:
            break
    assert status
    bad = str(tmp_path / "bad.v2")
    open(bad, "wb").write(bytes(body))
    with pytest.raises(ValueError, match=r"point 257 has status %d" % status):
        kzg.load_key(bad)
    if curve == "bls12_381":
        # point 5 replaced by P + T, T in the cofactor torsion: on the curve, outside the subgroup
        G = C.g1_group(cv)
        t = next(pt for pt, ok, what in subgroup_matrix() if what.startswith("T"))
        p5 = native.limbs_to_points(xy[5:6], inf[5:6])[0]
        body = bytearray(raw)
        body[24 + 5 * size:24 + 6 * size] = C.compress_g1(G.add(p5, t), cv)
        open(bad, "wb").write(bytes(body))
        with pytest.raises(ValueError, match=r"point 5 has status 3"):
            kzg.load_key(bad)
        loose = kzg.load_key(bad, check_subgroup=False)
        assert len(loose) == n and loose[5] == G.add(p5, t) and loose[6] == ck[6]
        loose.srs.close()
    ck.srs.close()


# ---- verification -----------------------------------------------------------------------------------------------------

def test_verify_cosets_with_the_subgroup_check_bls12_381(kzgs, native):
    kzg = kzgs["bls12_381"]
    cv = kzg._cv
    r = cv.r
    rng = random.Random(23)
    n, l = 64, 4
    ck, rk = kzg.setup(n - 1, tau=TAU)
    rk_l = kzg.coset_verification_key(l, TAU)
    polys = [[rng.randrange(r) for _ in range(n)]]
    comms = kzg.commit(ck, polys)
    proofs, values = kzg.open_cosets_each(ck, polys, l, n=n, with_values=True)
    cells = n // l
    ci, ki = [0] * cells, list(range(cells))
    rho = 99991
    checked = kzg.verify_cosets(ck, rk_l, comms, ci, ki, values[0], proofs[0], l, n, r=rho, check_subgroup=True)
    default = kzg.verify_cosets(ck, rk_l, comms, ci, ki, values[0], proofs[0], l, n, r=rho)
    assert checked is True and default is True
    # pi + T satisfies the pairing equation whenever pi does; only the subgroup check tells them apart
    t = next(pt for pt, ok, what in subgroup_matrix() if what.startswith("T"))
    forged = list(proofs[0])
    forged[3] = C.g1_group(cv).add(forged[3], t)
    assert C.on_curve_g1(forged[3], cv) and not C.in_subgroup_g1(forged[3], cv)
    assert kzg.verify_cosets(ck, rk_l, comms, ci, ki, values[0], forged, l, n, r=rho, check_subgroup=True) is False
    # a commitment outside the subgroup is refused as well
    assert kzg.verify_cosets(ck, rk_l, [C.g1_group(cv).add(comms[0], t)], ci, ki, values[0], proofs[0], l, n, r=rho,
                             check_subgroup=True) is False
    # verify_domain hands the flag on (l = 1)
    dproofs = kzg.open_domain_each(ck, polys, n=n)[0]
    w = int(kzg.Fq.root_of_unity(n))
    dvalues = [sum(c * pow(w, i * j, r) for j, c in enumerate(polys[0])) % r for i in range(n)]
    assert kzg.verify_domain(ck, rk, comms[0], dvalues, dproofs, r=rho, check_subgroup=True) is True
    dforged = list(dproofs)
    dforged[0] = C.g1_group(cv).add(dforged[0], t)
    assert kzg.verify_domain(ck, rk, comms[0], dvalues, dforged, r=rho, check_subgroup=True) is False
    ck.srs.close()


# ---- profiling ----------------------------------------------------------------------------------------------------------

def test_one_span_per_call(kzgs, native):
    kzg = kzgs["bls12_381"]
    ctx = kzg._context()
    xy, inf, pts, blobs = batch(kzg, native, 65)
    arr = np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(65, ctx.g1_bytes)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for check in (True, False):
            ctx.g1_decompress(arr, check)
        for _ in range(3):
            ctx.g1_check_subgroup(xy, inf)
        ms, count = ctx.prof_read("g1_decompress")
        assert count == 2 and ms > 0
        ms, count = ctx.prof_read("g1_subgroup")
        assert count == 3 and ms > 0
    finally:
        ctx.prof_enable(False)

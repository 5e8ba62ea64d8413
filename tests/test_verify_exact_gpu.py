"""GPU tests of the folded points of bulk verification at every launch regime (csrc/verify.hip, csrc/verify_points.hip
through the C ABI): kzg_verify_cosets, kzg_verify_cosets_bytes and kzg_verify_points return EXACTLY the points
tests/verify_scalars.py expects -- canonical limbs and infinity flags equal, no tolerance.

Proofs and commitments are points [tau^e] G of one generated key of 4096 points, drawn with repetition, with proofs
at infinity and a repeated proof in every case (verify_scalars.draw_proofs); values, indices and points z are random
and nobody's honest claims.  The fold is linear in the points, so L and R are multiples of G that Python integers give
for any such input: a wrong weight r_k, a tile never processed or a dropped share of a commitment sum changes a limb,
where the relation L == tau^l R of the older large tests holds for any weights the kernels agree on.  The shapes are
the table of verify_scalars (A: the rho table, B: the w table, C: tiles, D: the grid stride, E: commitment sums,
F: slices, G: kzg_verify_points, H: the bytes form); tests/test_verify_scalars_host.py shows that each reaches the
regime it names."""
import random

import numpy as np
import pytest

import verify_scalars as VS
from oracle import py_oracle as O

pytestmark = pytest.mark.gpu

CURVES = VS.CURVES
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba


@pytest.fixture(scope="module")
def keys(native):
    """per curve: (context, the key's handle, its points uint64[4096, 2 * fp_limbs]); the first device call of the
    module is made here"""
    from kzg_snark_amd.kzg import KZG
    out = {}
    for curve in CURVES:
        kzg = KZG(curve)
        ck = kzg.setup(VS.KEY_N - 1, tau=TAU)[0]
        kxy, kinf = ck.srs.export()
        assert kxy.shape[0] == VS.KEY_N and not kinf.any()
        out[curve] = (kzg._context(), ck, kxy)
    return out


def assert_points(curve, kxy, got, Ls, Rs, what):
    """the library's (xy, inf) are [Ls] G and [Rs] G: every limb and both flags"""
    xy, inf = got
    for q, (name, scalar) in enumerate((("L", Ls), ("R", Rs))):
        want_xy, want_inf = VS.expected(curve, kxy[0], scalar)
        assert int(inf[q]) == want_inf, (what, name, "infinity flag")
        assert np.array_equal(np.asarray(xy[q]), want_xy), (what, name)


def run_cosets(keys, curve, c, rho=None, seed=0):
    """one coset case through kzg_verify_cosets -> (inputs, library points, expected scalars)"""
    cv = O.curve(curve)
    ctx, ck, kxy = keys[curve]
    e_comm, comm_idx, coset_idx, values, e_proof, drawn_rho = VS.draw_case(c, cv, seed)
    rho = drawn_rho if rho is None else rho
    l, N = 1 << c.log_l, 1 << c.log_N
    w = cv.root_of_unity(N)
    cxy, cinf = VS.key_points(kxy, e_comm)
    pxy, pinf = VS.key_points(kxy, e_proof)
    got = ctx.verify_cosets(ck.srs, c.log_N, c.log_l, w, cxy, cinf, comm_idx, coset_idx, values, pxy, pinf, rho)
    Ls, Rs = VS.coset_fold_scalars(e_comm, comm_idx, coset_idx, values, e_proof, l, N, w, rho, TAU, cv.r)
    return (w, cxy, cinf, comm_idx, coset_idx, values, pxy, pinf, rho), got, (Ls, Rs)


def curve_cases(cases):
    return [pytest.param(curve, c, id=f"{curve}-{VS.case_id(c)}") for c in cases for curve in c.curves]


# ---- A .. F: kzg_verify_cosets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,c", curve_cases(VS.A_CASES))
def test_a_rho_table(keys, curve, c):
    """l = 1, K around 2048 and 4096: r_k = rho^(k+1) from the second level of the rho table (the coset indices stay
    below 2048, the first level of the w table, so that what goes wrong here from K = 2048 on is the rho table)"""
    _, got, (Ls, Rs) = run_cosets(keys, curve, c)
    assert_points(curve, keys[curve][2], got, Ls, Rs, VS.case_id(c))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("which", ["zero", "one", "minus_one"])
def test_a_rho_table_at_special_rho(keys, curve, which):
    """K = 2049 with rho = 0 (every weight zero: two infinities), 1 (every weight one) and r - 1 (weights +-1)"""
    r = O.curve(curve).r
    c = next(c for c in VS.A_CASES if c.K == VS.A_RHO_K)
    rho = {"zero": 0, "one": 1, "minus_one": r - 1}[which]
    _, got, (Ls, Rs) = run_cosets(keys, curve, c, rho=rho)
    assert_points(curve, keys[curve][2], got, Ls, Rs, which)
    if rho == 0:
        assert (Ls, Rs) == (0, 0) and list(got[1]) == [1, 1] and not got[0].any()


@pytest.mark.parametrize("curve,c", curve_cases(VS.B_CASES))
def test_b_w_table(keys, curve, c):
    """coset indices around the exponent 2048 and at both ends of the domain: w^(i l), the butterflies' twiddles and
    h_k^-j from the second level of the w table, up to its entry 1023 at N = 2^21"""
    _, got, (Ls, Rs) = run_cosets(keys, curve, c)
    assert_points(curve, keys[curve][2], got, Ls, Rs, VS.case_id(c))


@pytest.mark.parametrize("curve,c", curve_cases(VS.C_CASES))
def test_c_tiles(keys, curve, c):
    """every l from 2 to 4096: one cell, a whole tile, a tail tile with whole cells missing, a tile and a half;
    128 KiB of LDS at l = 4096; l = 64 with M below, at and above the 2^15 threads of the column sum"""
    _, got, (Ls, Rs) = run_cosets(keys, curve, c)
    assert_points(curve, keys[curve][2], got, Ls, Rs, VS.case_id(c))


@pytest.mark.parametrize("curve,c", curve_cases(VS.D_CASES))
def test_d_grid_stride(keys, curve, c):
    """4097 tiles on 4096 workgroups: workgroup 0 takes a second tile into the LDS it has used; every cell dense"""
    (_, _, _, _, _, values, _, _, _), got, (Ls, Rs) = run_cosets(keys, curve, c)
    assert values[-1].any() and values[4096].any()
    assert_points(curve, keys[curve][2], got, Ls, Rs, VS.case_id(c))


@pytest.mark.parametrize("curve,c", curve_cases(VS.E_CASES))
def test_e_commitment_sums(keys, curve, c):
    """20,000 cells over 1 .. 300 commitments: 64 shares or one per commitment, a commitment without a cell, with one,
    with 16,421, and two at infinity"""
    _, got, (Ls, Rs) = run_cosets(keys, curve, c)
    assert_points(curve, keys[curve][2], got, Ls, Rs, VS.case_id(c))


@pytest.mark.parametrize("curve,c", curve_cases(VS.F_CASES))
def test_f_slices(keys, curve, c):
    """2^18 - 1 proofs: 16-bit windows, 17 slices of 15 bits; 2^18: 20-bit windows, 14 slices of 19 bits; rho near r"""
    (_, _, _, _, _, _, _, _, rho), got, (Ls, Rs) = run_cosets(keys, curve, c)
    assert rho >> (O.curve(curve).r.bit_length() - 8)
    assert_points(curve, keys[curve][2], got, Ls, Rs, VS.case_id(c))


# ---- G: kzg_verify_points at arbitrary z ---------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("K", VS.G_KS)
def test_g_points(keys, curve, K):
    """z anywhere in the field: the rho table's second level from K = 2048, a thread's second claim in
    vpt_weights_kernel from 16,385, a second ladder launch at 65,792"""
    cv = O.curve(curve)
    r = cv.r
    ctx, _, kxy = keys[curve]
    rng = random.Random(f"G-{K}-{curve}")
    e_proof = VS.draw_proofs(rng, K, VS.KEY_N)
    e_comm = [rng.randrange(VS.KEY_N) for _ in range(3)]
    comm_idx = [rng.randrange(3) for _ in range(K)]
    nrng = np.random.default_rng(K)
    zs, ys = VS.random_reduced(nrng, (K,), r), VS.random_reduced(nrng, (K,), r)
    zs[0], ys[1] = VS.ints_to_limbs([r - 1])[0], VS.ints_to_limbs([r - 1])[0]
    zs[2], ys[K - 1] = 0, 0
    rho = rng.randrange(2, r)
    cxy, cinf = VS.key_points(kxy, e_comm)
    pxy, pinf = VS.key_points(kxy, e_proof)
    got = ctx.verify_points(cxy, cinf, comm_idx, zs, ys, pxy, pinf, rho)
    Ls, Rs = VS.point_fold_scalars(e_comm, comm_idx, zs, ys, e_proof, rho, TAU, r)
    assert_points(curve, kxy, got, Ls, Rs, K)


# ---- H: the bytes form ---------------------------------------------------------------------------------------------------
def bit_reverse(t, bits):
    return int(format(t, f"0{bits}b")[::-1], 2) if bits else 0


@pytest.mark.parametrize("curve,c", curve_cases(VS.H_CASES))
def test_h_bytes_form(keys, curve, c):
    """kzg_verify_cosets_bytes on the same claims as 32-byte big-endian elements, in natural order and with element t
    of a cell holding value bitrev(t): the same expected points"""
    ctx, ck, kxy = keys[curve]
    (w, cxy, cinf, comm_idx, coset_idx, values, pxy, pinf, rho), got, (Ls, Rs) = run_cosets(keys, curve, c)
    assert_points(curve, kxy, got, Ls, Rs, "limbs")
    l = 1 << c.log_l
    natural = values.view(np.uint8).reshape(c.K, l, 32)[:, :, ::-1]            # little-endian limbs -> big-endian bytes
    perm = [bit_reverse(t, c.log_l) for t in range(l)]
    for bit_reversed, cells in ((0, natural), (1, natural[:, perm])):
        cells = np.ascontiguousarray(cells).reshape(c.K, 32 * l)
        xy, inf, status = ctx.verify_cosets_bytes(ck.srs, c.log_N, c.log_l, w, cxy, cinf, comm_idx, coset_idx, cells,
                                                  pxy, pinf, rho, bit_reversed=bool(bit_reversed))
        assert status == 0
        assert_points(curve, kxy, (xy, inf), Ls, Rs, f"bit_reversed={bit_reversed}")

"""The exact-point expectations of bulk verification without a GPU (tests/verify_scalars.py): the scalar formulas times
the generator equal the restatements over the group law (verify_restated.restated_LR,
points_restated.restated_LR_points) on both curves up to (l, N) = (16, 64), with infinite and repeated proofs, an
infinite commitment and rho in {0, 1, random}; the interpolation through the C oracle's transform equals
coset_interpolate; and every shape of tests/test_verify_exact_gpu.py reaches the launch regime it is there for,
according to the plan that csrc/ver_layout.h computes (printed by tests/shim/workspace_shim.cpp) and the constants of
the power table and of verify_points.hip (CPU suite)."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import msm_profiles
import verify_scalars as VS
from oracle import py_oracle as O
from points_restated import restated_LR_points
from verify_restated import coset_interpolate, restated_LR

CURVES = VS.CURVES
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "shim", "workspace_shim.cpp")
ROCM_INCLUDES = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "/opt/rocm/include"]

needs_shim = pytest.mark.skipif(
    shutil.which("g++") is None or not any(os.path.exists(os.path.join(d, "hip", "hip_runtime_api.h")) for d in ROCM_INCLUDES),
    reason="needs g++ and the ROCm headers")


def generator_limbs(cv):
    L = (cv.p.bit_length() + 63) // 64
    return np.frombuffer(b"".join(int(v).to_bytes(8 * L, "little") for v in cv.g1), dtype="<u8").copy()


def same(curve, cv, scalar, point):
    """[scalar] G through the C oracle equals the oracle point, coordinate for coordinate"""
    xy, inf = VS.expected(curve, generator_limbs(cv), scalar)
    aff = O.normalize(point, cv)
    if aff is None:
        return inf == 1 and not xy.any()
    L = xy.size // 2
    got = [int.from_bytes(xy[q * L:(q + 1) * L].tobytes(), "little") for q in range(2)]
    return inf == 0 and tuple(got) == tuple(aff)


def pt(ck, e):
    return O.Z1() if e is None else ck[e]


# ---- the formulas -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("l,N", [(1, 8), (4, 16), (8, 32), (16, 64)])
def test_coset_scalars_times_the_generator_are_the_restated_points(curve, l, N):
    """9 cells that are nobody's honest claims: random values, proofs [tau^e] G with two at infinity and one repeated,
    three commitments with one at infinity"""
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(100 * l + N + len(curve))
    n, K = max(l, 8), 9
    ck = O.setup(n - 1, TAU, cv)
    w = cv.root_of_unity(N)
    e_proof = VS.draw_proofs(rng, K, n)
    assert e_proof.count(None) == 2 and len(set(e_proof)) < K - 1
    e_comm = [rng.randrange(n), None, rng.randrange(n)]
    comm_idx = [rng.randrange(3) for _ in range(K)]
    comm_idx[:2] = [1, 0]
    coset_idx = [rng.randrange(N // l) for _ in range(K)]
    coset_idx[:2] = [N // l - 1, 0]
    values = VS.random_reduced(np.random.default_rng(l + N), (K, l), r)
    ints = [VS.limbs_to_ints(values[k]) for k in range(K)]
    for rho in [rng.randrange(2, r)] + ([0, 1, r - 1] if (l, N) == (4, 16) else []):
        Ls, Rs = VS.coset_fold_scalars(e_comm, comm_idx, coset_idx, values, e_proof, l, N, w, rho, TAU, r)
        wantL, wantR = restated_LR(ck, [pt(ck, e) for e in e_comm], comm_idx, coset_idx, ints,
                                   [pt(ck, e) for e in e_proof], l, N, w, rho, cv)
        assert same(curve, cv, Ls, wantL), rho
        assert same(curve, cv, Rs, wantR), rho
        if rho == 0:
            assert (Ls, Rs) == (0, 0)


@pytest.mark.parametrize("curve", CURVES)
def test_point_scalars_times_the_generator_are_the_restated_points(curve):
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(len(curve))
    n, K = 16, 9
    ck = O.setup(n - 1, TAU, cv)
    e_proof = VS.draw_proofs(rng, K, n)
    e_comm = [rng.randrange(n), None, rng.randrange(n)]
    comm_idx = [1, 0] + [rng.randrange(3) for _ in range(K - 2)]
    zs = [0, r - 1] + [rng.randrange(r) for _ in range(K - 2)]
    ys = [r - 1, 0] + [rng.randrange(r) for _ in range(K - 2)]
    for rho in (rng.randrange(2, r), 0, 1, r - 1):
        wantL, wantR = restated_LR_points([pt(ck, e) for e in e_comm], comm_idx, zs, ys, [pt(ck, e) for e in e_proof],
                                          rho, cv)
        for z_in, y_in in ((zs, ys), (VS.ints_to_limbs(zs), VS.ints_to_limbs(ys))):
            Ls, Rs = VS.point_fold_scalars(e_comm, comm_idx, z_in, y_in, e_proof, rho, TAU, r)
            assert same(curve, cv, Ls, wantL), rho
            assert same(curve, cv, Rs, wantR), rho


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_l,log_N", [(0, 3), (1, 4), (3, 5), (6, 13), (9, 21)])
def test_the_fast_interpolation_is_coset_interpolate(curve, log_l, log_N):
    cv = O.curve(curve)
    r = cv.r
    l, N = 1 << log_l, 1 << log_N
    w = cv.root_of_unity(N)
    zeta = pow(w, N // l, r)
    rng = random.Random(log_l)
    cell = VS.random_reduced(np.random.default_rng(log_N), (l,), r)
    cell[0] = VS.ints_to_limbs([r - 1])[0]
    before = cell.copy()
    for i in (0, 1, N // l - 1, rng.randrange(N // l)):
        h = pow(w, i, r)
        assert VS.cell_interpolate(cell, h, zeta, r) == coset_interpolate(VS.limbs_to_ints(cell), h, zeta, r)
    assert (cell == before).all()


def test_the_drawn_proofs_carry_the_promised_edges():
    rng = random.Random(1)
    for K in (4, 8, 2049):
        e = VS.draw_proofs(rng, K, VS.KEY_N)
        finite = [x for x in e if x is not None]
        assert len(e) == K and e.count(None) == 2 and len(set(finite)) < len(finite)
    assert [VS.draw_proofs(rng, K, VS.KEY_N).count(None) for K in (1, 2, 3)] == [0, 1, 2]


# ---- every row of the table reaches its regime --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    inc = next(d for d in ROCM_INCLUDES if os.path.exists(os.path.join(d, "hip", "hip_runtime_api.h")))
    exe = str(tmp_path_factory.mktemp("plan") / "workspace_shim")
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, SRC, "-o", exe],
                   check=True)

    def plan(K, log_l, n_comm, curve):
        """the plan of a call whose proofs make a key of K points: wide windows from 2^WIDE_KEY_LOG points on"""
        win_bits = msm_profiles.WIDTHS[1] if K >= 1 << msm_profiles.WIDE_KEY_LOG else msm_profiles.WIDTHS[0]
        res = subprocess.run([exe, "plan", *map(str, (K, log_l, n_comm, win_bits, O.curve(curve).r.bit_length()))],
                             capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
        return {k: int(v) for k, v in (line.split() for line in res.stdout.splitlines())}
    return plan


POW_TLO = 1 << VS.source_constant("fr_util.h", r"constexpr uint32_t POW_TLOG = (\d+);")


def reached(c, p, coset_idx):
    """the regime facts of one case from its plan p, under the names the table uses"""
    l = 1 << c.log_l
    return dict(ntiles=p["ntiles"], tail=p["M"] % (1 << p["log_e"]) != 0, strided=p["ntiles"] > p["cell_grid"],
                lds_bytes=p["lds_bytes"], m_vs_sum=(p["M"] > p["sum_threads"]) - (p["M"] < p["sum_threads"]),
                shares=p["shares"], slice_bits=p["slice_bits"], slices=p["slices"], rho_hi=c.K >= POW_TLO,
                w_hi=max(i * l for i in coset_idx) >= POW_TLO)


@needs_shim
@pytest.mark.parametrize("c", VS.COSET_CASES, ids=VS.case_id)
def test_every_coset_shape_reaches_the_regime_it_names(plan_of, c):
    cv = O.curve(c.curves[0])
    _, comm_idx, coset_idx, values, e_proof, _ = VS.draw_case(c, cv, 0)
    assert len(e_proof) == len(comm_idx) == len(coset_idx) == values.shape[0] == c.K and values.shape[1] == 1 << c.log_l
    assert max(coset_idx) < 1 << (c.log_N - c.log_l) and max(comm_idx) < c.n_comm
    for curve in c.curves:
        p = plan_of(c.K, c.log_l, c.n_comm, curve)
        got = reached(c, p, coset_idx)
        if "slices" in c.reach and curve == "bn254":
            assert p["slices"] == -(-254 // p["slice_bits"])               # 254-bit scalars: 17 and 14 as well
        assert {k: got[k] for k in c.reach} == c.reach, (curve, p)
        assert p["sum_cnt"] << c.log_l == p["sum_threads"] and p["sum_threads"] % 256 == 0
        assert p["lds_bytes"] <= 160 * 1024 and p["cell_grid"] == min(p["ntiles"], 4096)


def test_the_table_holds_the_shapes_it_promises():
    ids = [VS.case_id(c) for c in VS.COSET_CASES]
    assert len(set(ids)) == len(ids)
    assert sorted({c.log_l for c in VS.C_CASES}) == list(range(1, 13))
    assert {c.reach["lds_bytes"] for c in VS.C_CASES if c.log_l == 12} == {128 * 1024}
    for log_l in range(1, 8):                                               # whole tile, tail with cells missing, between
        rows = [c for c in VS.C_CASES if c.log_l == log_l and "lds_bytes" in c.reach]
        assert {(c.reach["ntiles"], c.reach["tail"]) for c in rows} >= {(1, True), (1, False), (2, True)}
        assert any(256 < (c.K << log_l) < 512 for c in rows) and any(c.K << log_l == 256 + (1 << log_l) for c in rows)
    assert len(VS.H_CASES) == 4 and {c.group for c in VS.H_CASES} == {"B", "C"}
    # case B: the index whose exponent i l is exactly the first of the table's second level, and entry 1023 at 2^21
    for c in VS.B_CASES:
        idx = VS.w_table_indices(c, random.Random(0))
        l, N = 1 << c.log_l, 1 << c.log_N
        assert len(idx) == 8 and {0, 1, N // l // 2, N // l - 1} <= set(idx)
        if l <= 2048:
            assert {POW_TLO // l - 1, POW_TLO // l, POW_TLO // l + 1} <= set(idx)
        if c.log_N == 21:                                                    # h_k^-j or the butterflies read w^(N - 1 ..)
            assert (N - 1) >> 11 == 1023 and (l > 1 or ((N // l - 1) * l) >> 11 == 1023)
    # case E: no cell, one cell, a count above 16,384 that 64 does not divide, two commitments at infinity with cells
    for c in VS.E_CASES:
        ci = VS.commitment_cells(c, random.Random(0))
        counts = [ci.count(j) for j in range(c.n_comm)]
        assert sum(counts) == c.K and any(n > 16384 and n % 64 for n in counts)
        if c.n_comm >= 2:
            assert 1 in counts
        if c.n_comm > 2:
            assert counts[0] == 0 and counts[1] == 1 and counts[2] == 16421
            inf = VS.infinite_commitments(c)
            assert len(inf) == 2 and all(counts[j] > 0 for j in inf)


def test_the_point_cases_reach_the_second_claim_and_the_second_launch():
    """kzg_verify_points: the rho table's second level from K = 2048; vpt_weights_kernel has 2^14 threads, so claim
    16,384 is a thread's second; 2 nb + nc workgroups above 512 make a second ladder launch"""
    src = "verify_points.hip"
    assert VS.VPT_TB == VS.source_constant(src, r"constexpr uint32_t VPT_TB = (\d+);")
    assert VS.VPT_LAUNCH_BLOCKS == VS.source_constant(src, r"constexpr uint32_t VPT_LAUNCH_BLOCKS = (\d+);")
    assert VS.VPT_WEIGHT_THREADS == 1 << VS.source_constant(src, r"constexpr uint32_t VPT_WEIGHT_THREADS = 1u << (\d+);")
    assert POW_TLO == 2048 and {K >= POW_TLO for K in VS.G_KS[:3]} == {False, True}
    assert VS.G_KS[:3] == [POW_TLO - 1, POW_TLO, POW_TLO + 1]
    assert VS.G_KS[3:5] == [VS.VPT_WEIGHT_THREADS, VS.VPT_WEIGHT_THREADS + 1]
    launches = [-(-(2 * -(-K // VS.VPT_TB) + 1) // VS.VPT_LAUNCH_BLOCKS) for K in VS.G_KS]
    assert launches == [1, 1, 1, 1, 1, 2]

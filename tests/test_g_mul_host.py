"""Per-point scalar multiplication on the CPU: csrc/g_mul.h -- the text the gfx950 kernels of g_mul.hip compile -- built
for the host (tests/shim/g_mul_shim.cpp) against curve.Group.multiply on the whole case list of g_mul_cases.py, both
groups, both curves, word for word; the case list itself; the same shim as a program under the sanitizers; the launch
plan and the table indices that g_mul.hip's drivers and kernels take from that header."""
import os
import re
import subprocess

import pytest

import g_mul_cases as gm
from kzg_snark_amd import curve as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["kzg_g1_mul_each", "kzg_g1_mul_each_device", "kzg_g1_mul_powers", "kzg_srs_mul_powers", "kzg_g2_mul_each",
               "kzg_g2_mul_powers"]


def test_symbols_are_declared_defined_and_listed():
    from kzg_snark_amd import _native
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    api = open(os.path.join(ROOT, "kzg_snark_amd", "csrc", "api.hip")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(kzg_ctx\* ctx" % name, header, re.M), name
        assert re.search(r"^int %s\(kzg_ctx\* ctx" % name, api, re.M), name
        assert name in _native.SIGNATURES, name
    from kzg_snark_amd.kzg import KZG
    for method in ("multiply_each", "multiply_each_g2", "scale_key", "unit_setup", "contribute", "verify_contribution",
                   "verify_contributions"):
        assert callable(getattr(KZG, method)), method


@pytest.mark.parametrize("name", gm.CURVES)
def test_the_case_list_holds_what_it_promises(name):
    r = C.CURVES[name].r
    ks = set(gm.scalars(name))
    assert {0, 1, 2, 15, 16, 17, 1 << 255, (1 << 256) - 1, 2 * r - 4} <= ks
    assert all(16 ** j in ks for j in range(64))
    assert all(r + d in ks and 2 * r + d in ks for d in range(-40, 41))
    for g in (1, 2):
        what = [w for _, w in gm.points(name, g)]
        assert what[:3] == ["infinity", "G", "-G"]
        cofactor = g == 2 or name == "bls12_381"
        assert ("outside the subgroup" in what) == cofactor
        assert any(w.startswith("order ") for w in what) == cofactor
        G = gm.group(name, g)
        for pt, w in gm.points(name, g):
            if w == "outside the subgroup":
                assert not G.is_inf(G.multiply(pt, r))          # [r] Q != O: the scalar must not be reduced mod r
            if w.startswith("order "):
                q = int(w.split()[1])
                assert not G.is_inf(pt) and G.is_inf(G.multiply(pt, q))


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("name", gm.CURVES)
def test_every_case_equals_the_host_reference(name, g):
    lib = gm.build_shim()
    rows = gm.cases(name, g)
    assert len(rows) >= 400 if (g == 2 or name == "bls12_381") else len(rows) >= 350
    for pt, k, want, what in rows:
        assert gm.shim_mul(lib, name, g, pt, k) == (0, want), (what, hex(k))


@pytest.mark.parametrize("name", gm.CURVES)
def test_points_that_are_not_points_are_refused(name):
    lib = gm.build_shim()
    cv = C.CURVES[name]
    for g in (1, 2):
        gen = gm.points(name, g)[1][0]
        if g == 1:
            off, big = (gen[0], gen[1] ^ 1, 1), (gen[0] + cv.p, gen[1], 1)
        else:
            off, big = (gen[0], (gen[1][0] ^ 1, gen[1][1]), (1, 0)), ((gen[0][0] + cv.p, gen[0][1]), gen[1], (1, 0))
        assert gm.shim_mul(lib, name, g, off, 5)[0] == 1
        if (gen[0] if g == 1 else gen[0][0]) + cv.p < 1 << (32 * gm.fp_words(cv)):
            assert gm.shim_mul(lib, name, g, big, 5)[0] == 1


def plan_sizes(tb, cap, limit):
    ns = {0, 1, tb - 1, tb, tb + 1, limit}
    ns |= {c * cap + d for c in range(1, 17) for d in (-tb - 1, -tb, -1, 0, 1, tb, tb + 1)}
    return sorted({min(max(n, 0), limit) for n in ns})


def test_the_shim_states_the_constants_of_the_python_layer():
    from kzg_snark_amd import _native
    consts, limit = gm.shim_consts(gm.build_shim())
    ctx = _native.Context
    assert consts == {1: (ctx.G1_MUL_LANES, ctx.G1_MUL_LAUNCH_LANES), 2: (ctx.G2_MUL_LANES, ctx.G2_MUL_LAUNCH_LANES)}
    assert limit == 1 << 21


@pytest.mark.parametrize("g", [1, 2])
def test_the_plan_covers_every_block_once_in_the_fewest_launches(g):
    """GmPlan (csrc/g_mul.h) as the drivers of g_mul.hip loop over it: launches b0 = 0, launch_blocks, ... of
    min(launch_blocks, blocks - b0) workgroups."""
    lib = gm.build_shim()
    consts, limit = gm.shim_consts(lib)
    tb, cap = consts[g]
    assert cap % tb == 0
    cap_blocks = cap // tb
    sizes = plan_sizes(tb, cap, limit)
    assert {0, 1, cap, cap + 1, 2 * cap + 1, limit} <= set(sizes)
    for n in sizes:
        blocks, launch_blocks = gm.shim_plan(lib, n, g)
        assert blocks == -(-n // tb), n
        grids, b0 = [], 0
        while b0 < blocks:
            assert launch_blocks > 0, n
            grids.append((b0, min(launch_blocks, blocks - b0)))
            b0 += launch_blocks
        # [0, blocks) exactly once and in order, no launch empty or above the cap, and no launch more than needed
        at = 0
        for b0, grid in grids:
            assert b0 == at and 1 <= grid <= cap_blocks, (n, grids)
            at += grid
        assert at == blocks, (n, grids)
        assert len(grids) == -(-blocks // cap_blocks), (n, grids)
        if n == 0:
            assert grids == [] and launch_blocks == 0
        # the same ranges in lanes, as the GPU tests take them
        assert gm.launches(lib, n, g) == [(b0 * tb, min(n, (b0 + grid) * tb)) for b0, grid in grids]


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("name", gm.CURVES)
def test_every_launch_grid_stays_inside_the_table_and_below_2_pow_25(name, g):
    """The largest index of a launch -- entry 7, last piece, last slot, slots = grid * TB -- by the kernels' own 32-bit
    arithmetic (gm_entry_index / gm_piece_index): equal to the same index in Python integers (nothing wrapped), inside
    what the drivers allocate for launch_blocks workgroups, and below the 2^25 vectors csrc/g_mul.h promises."""
    lib = gm.build_shim()
    consts, limit = gm.shim_consts(lib)
    tb, cap = consts[g]
    seen = set()
    for n in plan_sizes(tb, cap, limit):
        launch_blocks = gm.shim_plan(lib, n, g)[1]
        if launch_blocks in seen:
            continue
        seen.add(launch_blocks)
        for grid in range(1, launch_blocks + 1):
            pieces, top, vectors = gm.shim_table(lib, name, g, grid, launch_blocks)
            assert vectors == 8 * pieces * tb * launch_blocks
            assert top == 8 * pieces * grid * tb - 1, (n, grid)
            assert top < vectors and top < 1 << 25, (n, grid)
    assert cap // tb in seen and 1 in seen


def test_the_case_list_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """g_mul_shim.cpp with its own main(), built with -fsanitize=address,undefined and run as a program of its own over
    the whole case list.  The exit status is the verdict: 0 = no sanitizer report and every product as expected."""
    exe, data = str(tmp_path / "g_mul_shim_san"), str(tmp_path / "cases.bin")
    count = gm.replay_file(data, gm.build_shim())
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DG_MUL_SHIM_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", gm.SHIM_SRC, "-o", exe], check=True)
    res = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert f"{count} cases, 0 mismatches" in res.stdout

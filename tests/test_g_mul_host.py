"""Per-point scalar multiplication on the CPU: csrc/g_mul.h -- the text the gfx950 kernels of g_mul.hip compile -- built
for the host (tests/shim/g_mul_shim.cpp) against curve.Group.multiply on the whole case list of g_mul_cases.py, both
groups, both curves, word for word; the case list itself; the same shim as a program under the sanitizers."""
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

"""The Shplonk opening without a GPU: the plain-Python restatement (tests/multi_restated.py: long
division by Z_S, not the library's partial fractions) satisfies the check equation in the exponent and stops satisfying
it after any one change -- which pins what the GPU tests compare the library against; with every set equal to [z] its
first proof point is the reference opening's; the facade's verifier accepts it with the Python pairing; bad arguments
are ValueErrors before any device call; the new symbols are declared, exported and bound; the new kernels keep the
register budget of the single-point kernels they stand beside (CPU suite)."""
import os
import random
import re
import subprocess

import pytest

from oracle import py_oracle as O
from multi_restated import (check_in_the_exponent, interpolate, poly_divmod, quotient_points, restate_open_multi,
                            union, vanishing)
from restated import g1_mul, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_0f_5410_0ca7_1234_5678_9abc_def0
NEW_SYMBOLS = {"kzg_fr_poly_eval_batch": 8, "kzg_open_points_device": 12, "kzg_open_points": 12}


@pytest.fixture(scope="module")
def built():
    from kzg_snark_amd import build
    return build.build(verbose=False)


def case(curve, seed=0):
    """5 polynomials of lengths 37, 1, 20, 5, 37 over 4 points: sets of 1 to 4 points, one polynomial (length 1) shorter
    than its set of two"""
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(1000 * seed + len(curve))
    polys = [[rng.randrange(r) for _ in range(n)] for n in (37, 1, 20, 5, 37)]
    z = [rng.randrange(r) for _ in range(4)]
    sets = [[z[0]], [z[1], z[0]], [z[0], z[2], z[3]], [z[3], z[2], z[1], z[0]], [z[2]]]
    gamma, zeta = rng.randrange(1, r), rng.randrange(r)
    comms = [O.commit_trapdoor(p, TAU, cv) for p in polys]
    return cv, polys, sets, gamma, zeta, comms


def test_the_polynomial_helpers():
    r = O.curve("bn254").r
    assert vanishing([2, 3], r) == [6, r - 5, 1]
    assert poly_divmod([6, r - 5, 1], [r - 2, 1], r) == ([r - 3, 1], [0])
    assert interpolate([1, 2, 3], [1, 4, 9], r) == [0, 0, 1]
    assert union([[5, 1], [1, 7], [5]]) == [5, 1, 7]
    # sum of single-point quotients: (X^2 - 1)/(X - 1) + 2 (X^2 - 0)/(X - 0) = (X + 1) + 2 X
    assert quotient_points([[0, 0, 1]], [1, 0], [[1, 2]], r) == [1, 3]


@pytest.mark.parametrize("curve", CURVES)
def test_restated_proof_satisfies_the_check_equation_in_the_exponent(curve):
    cv, polys, sets, gamma, zeta, comms = case(curve)
    r = cv.r
    m = restate_open_multi(polys, sets, gamma, zeta, TAU, cv)
    assert m.evaluations[1] == [polys[1][0]] * 2
    assert len(m.T) == 4 and len(m.q) == 36

    def holds(comms=comms, evals=m.evaluations, W=m.W, W2=m.W2, gamma=gamma, zeta=zeta):
        return check_in_the_exponent(comms, sets, evals, W, W2, gamma, zeta, TAU, cv)

    assert holds()
    for i, j in ((0, 0), (2, 1), (3, 3)):
        bad = [list(v) for v in m.evaluations]
        bad[i][j] = (bad[i][j] + 1) % r
        assert not holds(evals=bad)                                        # one altered evaluation
    assert not holds(W=m.W2, W2=m.W)                                       # W and W' swapped
    assert not holds(gamma=(gamma + 1) % r)
    assert not holds(zeta=(zeta + 1) % r)
    assert not holds(comms=[comms[2]] + comms[1:])                         # a commitment replaced
    # the first proof point as the library forms it: weights gamma^(i+1) / prod_(m in S_i, m != z) (z - m)
    weights, g = [[0] * 4 for _ in polys], 1
    for i, S in enumerate(sets):
        g = g * gamma % r
        for z in S:
            d = 1
            for other in S:
                if other != z:
                    d = d * (z - other) % r
            weights[i][m.T.index(z)] = g * pow(d, -1, r) % r
    assert quotient_points(polys, m.T, weights, r) == m.q


@pytest.mark.parametrize("curve", CURVES)
def test_single_point_sets_give_the_reference_opening(curve):
    """every set [z]: q is the reference's witness polynomial and W its commitment through the key (kzg.py:122-159)"""
    cv, polys, _, gamma, zeta, _ = case(curve, seed=1)
    polys = [p[:9] for p in polys]
    z = 0x1234567
    m = restate_open_multi(polys, [[z]] * len(polys), gamma, zeta, TAU, cv)
    ck = O.setup(8, TAU, cv)
    proof, _ = O.open_(ck, polys, z, gamma, cv)
    assert O.eq(m.W, proof, cv)
    assert O.poly_normalize(m.q) == O.poly_divide_linear(O.combine(polys, gamma, cv.r), z, cv.r)[0]


def test_check_multi_accepts_the_restated_proof_with_the_python_pairing():
    from kzg_snark_amd.kzg import KZG, OpenMulti
    cv, polys, sets, gamma, zeta, _ = case("bn254", seed=2)
    polys = [p[:16] for p in polys]
    comms = [O.commit_trapdoor(p, TAU, cv) for p in polys]
    m = restate_open_multi(polys, sets, gamma, zeta, TAU, cv)
    kzg = KZG("bn254")
    rk = kzg.multiply(kzg.G2, TAU % cv.r)
    proof = OpenMulti(m.W, m.W2, zeta, m.evaluations)
    assert kzg.check_multi(rk, comms, sets, m.evaluations, proof, gamma, zeta, pairing="host") is True
    bad = [list(v) for v in m.evaluations]
    bad[3][2] = (bad[3][2] + 1) % cv.r
    assert kzg.check_multi(rk, comms, sets, bad, (m.W, m.W2), gamma, zeta, pairing="host") is False
    off_curve = (m.W[0], (m.W[1] + 1) % cv.p, m.W[2])
    assert kzg.check_multi(rk, comms, sets, m.evaluations, (off_curve, m.W2), gamma, zeta, pairing="host") is False


@pytest.mark.parametrize("curve", CURVES)
def test_facade_rejects_bad_arguments_before_the_device(curve, monkeypatch):
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_native, "get_context", no_device)
    monkeypatch.setattr(KZG, "_key", lambda self, ck: ck)
    kzg = KZG(curve)
    G, rk = kzg.G1, kzg.G2
    polys = [[1, 2, 3], [4, 5]]
    for sets in ([[5], []], [[5, 5], [6]], [[5, 5 + kzg.curve_order], [6]], [[5]], [[5], [6], [7]]):
        with pytest.raises(ValueError):
            kzg.open_multi([G] * 4, polys, sets, 3, 9)                     # empty, repeated (mod r too), wrong count
        with pytest.raises(ValueError):
            kzg.check_multi(rk, [G, G], sets, [[1] * len(S) for S in sets], (G, G), 3, 9)
    with pytest.raises(ValueError):
        kzg.check_multi(rk, [G, G], [[5], [6, 7]], [[1], [2]], (G, G), 3, 9)      # values do not follow the sets
    with pytest.raises(ValueError):
        kzg.check_multi(rk, [G, G], [[5], [6]], [[1], [2]], (G, G), 3, 9, pairing="gpu")
    with pytest.raises(ValueError):
        kzg.open_multi([G] * 4, [[1]] * 64, [[5]] * 64, 3, 9)              # q is the 64th polynomial of the second call
    with pytest.raises(ValueError):
        kzg.evaluate_each([[1]] * 65, [5])
    assert kzg.evaluate_each([], [5]) == []
    assert kzg.evaluate_each([[1], [2]], []) == [[], []]


def test_the_symbols_are_declared_exported_and_bound(built):
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from kzg_snark_amd import _native
    _native.lib()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared
        assert name in exported
        assert name in _native.SIGNATURES
        assert name not in _native.MISSING
        assert len(_native.SIGNATURES[name][1]) == nargs
    assert _native.lib().kzg_abi_version() == 1
    from kzg_snark_amd.kzg import KZG
    for method in ("evaluate_each", "open_multi", "check_multi"):
        assert callable(getattr(KZG, method))


# ---- kernel budget ---------------------------------------------------------------------------------------------------
def waves_per_simd(vgpr):
    """512 VGPRs per SIMD lane, allocated in blocks of 8"""
    return 512 // ((vgpr + 7) // 8 * 8)


def by_tile_width(rows):
    """a tile kernel's rows [(vgpr, lds, scratch)] split by tile width -- told apart by their LDS, which doubles with the
    tile -- each half sorted by registers (the lighter scalar field first, in every kernel)"""
    cut = (min(lds for _, lds, _ in rows) + max(lds for _, lds, _ in rows)) / 2
    return (sorted(k for k in rows if k[1] < cut), sorted(k for k in rows if k[1] >= cut))


def test_new_kernels_keep_the_budget_of_the_single_point_kernels(built):
    """No scratch; and as many waves per SIMD by registers as the kernel of the same role: tile_combine_multi_kernel
    against tile_combine_kernel of the same tile width, field by field, the existing kernel's figures read from the same
    library.  Pass 2 of the several points is tile_fill_kernel itself: it exists once per field and tile width (no
    second fill kernel beside it), with the LDS of its two tiles, and keeps the waves per SIMD that the 71 and 84 VGPRs
    of the single-point kernel gave it before it took the points' `zero` and `add`."""
    out, listing = kernel_resources(built)
    rows = {}
    for raw, vgpr, _, _, lds, scratch in listing:
        k = re.search(r"(\w+_kernel)\b", raw)
        rows.setdefault(k.group(1) if k else raw, []).append((vgpr, lds, scratch))
    for name, count in (("tile_combine_multi_kernel", 6), ("tile_fill_kernel", 4), ("tile_eval_batch_kernel", 2)):
        assert len(rows.get(name, [])) == count, (name, out)              # two fields x (two widths [+ evaluation form])
        assert all(scratch == 0 for _, _, scratch in rows[name]), (name, rows[name])
    assert not [name for name in rows if "tile_fill" in name and name != "tile_fill_kernel"], sorted(rows)
    for mine, theirs in zip(by_tile_width(rows["tile_combine_multi_kernel"]), by_tile_width(rows["tile_combine_kernel"])):
        assert len(mine) == len(theirs) and mine, (mine, theirs)
        for (v_new, _, _), (v_old, _, _) in zip(mine, theirs):
            assert waves_per_simd(v_new) >= waves_per_simd(v_old), (v_new, v_old)
    for half, lds_bytes in zip(by_tile_width(rows["tile_fill_kernel"]), (35588, 71108)):
        assert [lds for _, lds, _ in half] == [lds_bytes] * 2, half
        for (vgpr, _, _), v_parent in zip(half, (71, 84)):                # the lighter scalar field first
            assert waves_per_simd(vgpr) >= waves_per_simd(v_parent), (vgpr, v_parent)
    assert (waves_per_simd(71), waves_per_simd(84)) == (7, 5)
    for vgpr, lds, _ in rows["tile_eval_batch_kernel"]:
        assert vgpr <= 128 and lds <= 2048

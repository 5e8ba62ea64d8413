"""Bulk verification at arbitrary points without a GPU: kzg_verify_points and the batched barycentric evaluation are
declared, exported and bound; the plain-Python restatement of the two folded points (tests/points_restated.py)
satisfies L == tau R on oracle-made openings at arbitrary points and fails after any one claim is changed -- which pins
the formula the GPU tests compare the library against; the facade rejects bad arguments before any device call; the
new kernels fit their budget (CPU suite)."""
import os
import random
import re
import subprocess

import pytest

from oracle import py_oracle as O
from points_restated import restated_LR_points
from restated import g1_mul, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
NEW_SYMBOLS = {"kzg_verify_points": 13, "kzg_fr_eval_lagrange_batch": 9, "kzg_fr_eval_lagrange_batch_device": 9}
NEW_G1_KERNELS = ["vpt_ladder_kernel", "vpt_fold_kernel"]                       # one per curve
NEW_FR_KERNELS = ["vpt_weights_kernel", "lagr_batch_denom_kernel", "lagr_batch_sums_kernel",
                  "lagr_batch_value_kernel"]                                    # one per scalar field


@pytest.fixture(scope="module")
def built():
    from kzg_snark_amd import build
    return build.build(verbose=False)


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
    for listed in ('"verify_points"', '"verify_points_device_bytes"', '"eval_lagrange_batch"', '"eval_batch_chunk"'):
        assert listed in text                                            # spans, counter and tuning key are documented
    from kzg_snark_amd.kzg import KZG
    for method in ("verify_points", "verify_blobs", "evaluate_evaluations_each"):
        assert callable(getattr(KZG, method))


# ---- the formula: L == tau R on honest claims, != after one change ---------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_restated_points_satisfy_the_pairing_equation_through_the_trapdoor(curve):
    """one polynomial of degree < 8 opened by the oracle at 5 arbitrary points (0 and r - 1 among them), and a second
    commitment (a constant: its proof is infinity) so that the grouping by commitment is exercised"""
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(len(curve))
    ck = O.setup(7, TAU, cv)
    polys = [[rng.randrange(r) for _ in range(8)], [rng.randrange(1, r)]]
    comms = O.commit(ck, polys, cv)
    comm_idx = [0, 1, 0, 0, 0, 1, 0]
    zs = [rng.randrange(r), rng.randrange(r), 0, r - 1, rng.randrange(r), 5, rng.randrange(r)]
    opened = [O.open_(ck, [polys[c]], z, 1, cv) for c, z in zip(comm_idx, zs)]
    proofs, ys = [p for p, _ in opened], [y for _, y in opened]
    assert all(y == O.poly_eval(polys[c], z, r) for c, z, y in zip(comm_idx, zs, ys))
    assert all(O.is_inf(p) for c, p in zip(comm_idx, proofs) if c == 1)
    rho = rng.randrange(1, r)

    def holds(ci=comm_idx, z=zs, y=ys, ps=proofs, rho=rho):
        L, R = restated_LR_points(comms, ci, z, y, ps, rho, cv)
        return O.eq(L, g1_mul(R, TAU % r, cv), cv)

    assert holds()
    assert holds(rho=1)
    bad = list(ys)
    bad[3] = (bad[3] + 1) % r
    assert not holds(y=bad)                                                # one value
    bad = list(zs)
    bad[0] = (bad[0] + 1) % r
    assert not holds(z=bad)                                                # one point
    bad = list(proofs)
    bad[0], bad[4] = bad[4], bad[0]
    assert not O.eq(proofs[0], proofs[4], cv)
    assert not holds(ps=bad)                                               # two proofs swapped
    bad = list(comm_idx)
    bad[2] = 1
    assert not holds(ci=bad)                                               # one commitment index


# ---- facade argument checks (no device call is reached) -------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_facade_rejects_bad_arguments_before_the_device(curve, monkeypatch):
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_native, "get_context", no_device)
    kzg = KZG(curve)
    G, rk = kzg.G1, kzg.G2
    w16 = int(kzg.Fq.root_of_unity(16))
    claims = dict(commitments=[G], commitment_indices=[0, 0], z_list=[5, 6], evaluations=[1, 2], proofs=[G, G])

    def call(rk=rk, **over):
        return kzg.verify_points(rk, **{**claims, **over})

    with pytest.raises(ValueError):
        call(z_list=[5])                                                   # lengths disagree
    with pytest.raises(ValueError):
        call(evaluations=[1, 2, 3])
    with pytest.raises(ValueError):
        call(proofs=[G])
    with pytest.raises(ValueError):
        call(commitment_indices=[0])
    with pytest.raises(ValueError):
        call(commitment_indices=[0, 1])                                    # index beyond the commitments
    with pytest.raises(ValueError):
        call(commitment_indices=[0, -1])
    with pytest.raises(ValueError):
        call(commitments=[])
    with pytest.raises(TypeError):
        call(rk=G)                                                         # a G1 point is no verification key
    with pytest.raises(TypeError):
        call(rk=None)
    assert call(commitment_indices=[], z_list=[], evaluations=[], proofs=[]) is True       # no claims: no device

    blobs = dict(commitments=[G, G], value_lists=[[1, 2], [3]], z_list=[5, 6], proofs=[G, G])
    with pytest.raises(TypeError):
        kzg.verify_blobs(w16, G, **blobs)
    with pytest.raises(ValueError):
        kzg.verify_blobs(w16, rk, **{**blobs, "z_list": [5]})
    with pytest.raises(ValueError):
        kzg.verify_blobs(w16, rk, **{**blobs, "proofs": [G]})
    with pytest.raises(ValueError):
        kzg.verify_blobs(w16, rk, **{**blobs, "commitments": [G]})
    with pytest.raises(ValueError):
        kzg.verify_blobs(w16, rk, **{**blobs, "value_lists": [[1] * 17, [3]]})             # longer than the domain
    with pytest.raises(ValueError):
        kzg.verify_blobs(3, rk, **blobs)                                   # 3 is no root of unity of power-of-two order
    assert kzg.verify_blobs(w16, rk, [], [], [], []) is True
    with pytest.raises(ValueError):
        kzg.evaluate_evaluations_each(w16, [[1, 2], [3]], [5])
    with pytest.raises(ValueError):
        kzg.evaluate_evaluations_each(w16, [list(range(17))], [5])
    assert kzg.evaluate_evaluations_each(w16, [], []) == []


# ---- kernel budget -------------------------------------------------------------------------------------------------
def test_new_kernels_never_spill_and_fit_256_vgprs(built):
    out, listing = kernel_resources(built)
    rows = {}
    for raw, vgpr, _, _, lds, scratch in listing:
        k = re.search(r"(\w+_kernel)\b", raw)                             # demangled or plain
        rows.setdefault(k.group(1) if k else raw, []).append((vgpr, lds, scratch))
    for name in NEW_G1_KERNELS + NEW_FR_KERNELS:
        assert len(rows.get(name, [])) == 2, (name, out)
        for vgpr, lds, scratch in rows[name]:
            assert scratch == 0 and vgpr <= 256, (name, vgpr, scratch)
            if name in NEW_FR_KERNELS:
                assert vgpr <= 128 and lds <= 1024, (name, vgpr, lds)      # the budget of the other Fr kernels
            else:
                assert lds <= 32 * 1024, (name, lds)                       # 128 parked points of the block sum
    assert sorted(k for k in rows if k.startswith("vpt_")) == sorted(NEW_G1_KERNELS + ["vpt_weights_kernel"])

"""Bulk verification without a GPU: kzg_verify_cosets is declared, exported and bound; the plain-Python restatement of
the two folded points (tests/verify_restated.py) satisfies L == tau^l R on oracle-made proofs and fails after any one
claim is changed -- which pins the formula the GPU tests compare the library against; the slices the proof MSMs run
on stay below 2^(win_bits - 1) and recombine to the scalar; the facade rejects bad arguments before any device call;
the new kernels fit their budget (CPU suite)."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import py_oracle as O
from restated import g1_mul, kernel_resources
from verify_restated import honest_cell, restated_LR, slices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
NEW_FR_KERNELS = ["ver_weights_kernel", "ver_cell_kernel", "ver_colsum_kernel", "ver_colsum_final_kernel",
                  "ver_commsum_kernel"]                              # one per scalar field
NEW_PLAIN_KERNELS = ["ver_slice_kernel"]
# shared with key loading (msm.hip) and coset recovery (poly.hip): 2 curves x the range check on / off, 2 fields
SHARED_KERNELS = {"g1_import_kernel": 4, "fr_pow_table_kernel": 2}


@pytest.fixture(scope="module")
def built():
    from kzg_snark_amd import build
    return build.build(verbose=False)


def test_the_symbol_is_declared_exported_and_bound(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from kzg_snark_amd import _native
    _native.lib()
    name = "kzg_verify_cosets"
    assert name in declared
    assert name in exported
    assert name in _native.SIGNATURES
    assert name not in _native.MISSING
    assert len(_native.SIGNATURES[name][1]) == 17
    assert _native.lib().kzg_abi_version() == 1
    assert '"verify_cosets"' in open(HEADER).read()                  # the span is listed with the others


# ---- the formula: L == tau^l R on honest claims, != after one change ------------------------------------------------
def _claims(cv, n, l, N, rng):
    """three commitments (a full polynomial, one shorter than l or a single coefficient, the zero polynomial), 7 cells
    drawn with repetition, in random order"""
    r = cv.r
    ck = O.setup(n - 1, TAU, cv)
    polys = [[rng.randrange(r) for _ in range(n)], [rng.randrange(r) for _ in range(max(1, l - 1))], []]
    comms = O.commit(ck, polys, cv)
    w = cv.root_of_unity(N)
    comm_idx = [rng.randrange(3) for _ in range(7)]
    coset_idx = [rng.randrange(N // l) for _ in range(7)]
    cells = [honest_cell(ck, polys[c], i, l, N, w, cv) for c, i in zip(comm_idx, coset_idx)]
    return ck, polys, comms, w, comm_idx, coset_idx, [v for v, _ in cells], [p for _, p in cells]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,l,N", [(8, 1, 8), (8, 1, 16), (8, 2, 8), (8, 2, 16), (8, 4, 8), (8, 4, 16),
                                   (16, 1, 16), (16, 1, 32), (16, 2, 16), (16, 2, 32), (16, 4, 16), (16, 4, 32)])
def test_restated_points_satisfy_the_pairing_equation_through_the_trapdoor(curve, n, l, N):
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(n * 100 + l * 10 + N + len(curve))
    ck, polys, comms, w, comm_idx, coset_idx, values, proofs = _claims(cv, n, l, N, rng)
    rho = rng.randrange(1, r)
    tl = pow(TAU, l, r)

    def holds(ci=comm_idx, ki=coset_idx, vs=values, ps=proofs):
        L, R = restated_LR(ck, comms, ci, ki, vs, ps, l, N, w, rho, cv)
        return O.eq(L, g1_mul(R, tl, cv), cv)

    assert holds()
    # the proofs of the polynomial shorter than l (and of the zero polynomial) are the point at infinity
    assert all(O.is_inf(p) for c, p in zip(comm_idx, proofs) if len(polys[c]) <= l)
    k = next(k for k, c in enumerate(comm_idx) if c == 0) if 0 in comm_idx else 0
    bad_values = [list(v) for v in values]
    bad_values[k][l - 1] = (bad_values[k][l - 1] + 1) % r
    assert not holds(vs=bad_values)                                        # one value
    bad_proofs = list(proofs)
    bad_proofs[k] = O.add(proofs[k], O.from_affine(cv.g1), cv)
    assert not holds(ps=bad_proofs)                                        # one proof
    if 0 in comm_idx:                                                      # a cell of the full polynomial
        bad_cosets = list(coset_idx)
        bad_cosets[k] = (coset_idx[k] + 1) % (N // l)
        assert not holds(ki=bad_cosets)                                    # one coset index
        bad_comm = list(comm_idx)
        bad_comm[k] = 1
        assert not holds(ci=bad_comm)                                      # one commitment index


# ---- the slice identity of the proof MSMs ---------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("win_bits", [16, 20])
def test_slices_stay_below_half_a_window_and_recombine(curve, win_bits):
    r = O.curve(curve).r
    bits = r.bit_length()
    rng = random.Random(win_bits)
    sb = win_bits - 1
    for s in [0, 1, r - 1, (1 << sb) - 1, 1 << sb] + [rng.randrange(r) for _ in range(200)]:
        cut = slices(s, win_bits, bits)
        assert len(cut) == (bits + sb - 1) // sb
        assert all(0 <= d < (1 << sb) for d in cut)          # a signed-digit recoding never carries out of window 0
        assert sum(d << (i * sb) for i, d in enumerate(cut)) == s


# ---- facade argument checks (no device call is reached) -------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_facade_rejects_bad_arguments_before_the_device(curve, monkeypatch):
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG, DomainTable, LagrangeKey

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_native, "get_context", no_device)
    kzg = KZG(curve)
    r = kzg.curve_order
    ck = [kzg.G1] * 16
    rk = kzg.G2
    w16 = int(kzg.Fq.root_of_unity(16))
    G = kzg.G1
    cells = dict(commitments=[G], commitment_indices=[0, 0], coset_indices=[0, 1], values=[[1, 2, 3, 4]] * 2,
                 proofs=[G, G], l=4, N=16)

    def call(**over):
        return kzg.verify_cosets(ck, rk, **{**cells, **over})

    with pytest.raises(ValueError):
        call(l=3)                                                          # l not a power of two
    with pytest.raises(ValueError):
        call(N=12)                                                         # N not a power of two
    with pytest.raises(ValueError):
        call(l=16)                                                         # l > N/2
    with pytest.raises(ValueError):
        call(N=1 << 22)                                                    # N above 2^21
    with pytest.raises(ValueError):
        call(w=w16 * w16 % r)                                              # not a primitive 16th root
    with pytest.raises(ValueError):
        call(coset_indices=[0])                                            # lengths disagree
    with pytest.raises(ValueError):
        call(proofs=[G])
    with pytest.raises(ValueError):
        call(values=[[1, 2, 3, 4], [1, 2, 3]])                             # a cell with 3 values
    with pytest.raises(ValueError):
        call(commitment_indices=[0, 1])                                    # index beyond the commitments
    with pytest.raises(ValueError):
        call(coset_indices=[0, 4])                                         # index beyond N/l
    with pytest.raises(ValueError):
        kzg.verify_cosets(ck[:2], rk, **cells)                             # key shorter than l
    with pytest.raises(ValueError):
        call(commitments=[])
    lk = LagrangeKey.__new__(LagrangeKey)
    lk.n, lk.w, lk.log_n = 16, w16, 4
    with pytest.raises(TypeError):
        kzg.verify_cosets(lk, rk, **cells)
    dt = DomainTable.__new__(DomainTable)
    with pytest.raises(TypeError):
        kzg.verify_cosets(dt, rk, **cells)
    with pytest.raises(TypeError):
        kzg.verify_domain(lk, rk, G, [1, 2], [G, G])
    with pytest.raises(ValueError):
        kzg.verify_domain(ck, rk, G, [1, 2, 3], [G, G, G])                 # N defaults to 3: not a power of two
    with pytest.raises(ValueError):
        kzg.verify_domain(ck, rk, G, [1, 2], [G, G, G], N=4)               # values and proofs disagree
    # no claims: accepted without a device
    assert call(commitment_indices=[], coset_indices=[], values=[], proofs=[]) is True
    assert call(commitment_indices=[], coset_indices=[], values=np.zeros((0, 4, 4), dtype=np.uint64),
                proofs=(np.zeros((0, 2 * ((kzg._cv.p.bit_length() + 63) // 64)), dtype=np.uint64), None)) is True


# ---- kernel budget -------------------------------------------------------------------------------------------------
def test_new_kernels_never_spill_and_fit_256_vgprs(built):
    out, listing = kernel_resources(built)
    rows = {}
    for raw, vgpr, _, _, _, scratch in listing:
        k = re.search(r"(\w+_kernel)\b", raw)                             # demangled or plain
        rows.setdefault(k.group(1) if k else raw, []).append((vgpr, scratch))
    assert not [k for k in rows if k.startswith("ver_") and "prep_" in k]
    for names, count in ((NEW_FR_KERNELS, 2), (NEW_PLAIN_KERNELS, 1), *(([k], v) for k, v in SHARED_KERNELS.items())):
        for name in names:
            assert len(rows.get(name, [])) == count, (name, out)
            for vgpr, scratch in rows[name]:
                assert scratch == 0 and vgpr <= 256, (name, vgpr, scratch)
    assert sorted(k for k in rows if k.startswith("ver_")) == sorted(NEW_FR_KERNELS + NEW_PLAIN_KERNELS)

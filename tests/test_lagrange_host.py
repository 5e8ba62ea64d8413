"""Evaluation-form KZG without a GPU: the new C-ABI symbols are declared, exported and bound; the facade validates
its domain and value lists on the host; the new kernels fit their register budget and never spill (CPU suite)."""
import os
import re
import subprocess

import pytest

from restated import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")

NEW_SYMBOLS = ["kzg_srs_generate_lagrange", "kzg_srs_lagrange", "kzg_open_evals", "kzg_open_evals_device",
               "kzg_open_evals_device_async", "kzg_fr_eval_lagrange"]


@pytest.fixture(scope="module")
def built():
    from kzg_snark_amd import build
    return build.build(verbose=False)


def test_new_symbols_are_declared_exported_and_bound(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from kzg_snark_amd import _native
    _native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in _native.SIGNATURES, name
        assert name not in _native.MISSING, name
    assert _native.lib().kzg_abi_version() == 1


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_facade_validates_the_domain_without_a_gpu(curve):
    from kzg_snark_amd.kzg import KZG
    kzg = KZG(curve)
    r = kzg.curve_order
    w16 = int(kzg.Fq.root_of_unity(16))
    with pytest.raises(ValueError):
        kzg.setup_lagrange(12, tau=5)                                 # not a power of two
    with pytest.raises(ValueError):
        kzg.setup_lagrange(1, tau=5)                                  # a domain needs n >= 2
    with pytest.raises(ValueError):
        kzg.setup_lagrange(16, tau=5, w=w16 * w16 % r)                # an 8th root, not a primitive 16th one
    with pytest.raises(ValueError):
        kzg.setup_lagrange(16, tau=5, w=1)
    with pytest.raises(ValueError):
        kzg.lagrange_key([kzg.G1] * 16, 16, w=pow(w16, 2, r))         # non-primitive w
    with pytest.raises(ValueError):
        kzg.lagrange_key([kzg.G1] * 8, 16)                            # monomial key shorter than the domain
    with pytest.raises(ValueError):
        kzg.lagrange_key([kzg.G1] * 16, 24)
    with pytest.raises(ValueError):
        kzg.evaluate_evaluations(w16, list(range(17)), 3)             # more values than the domain has points
    with pytest.raises(ValueError):
        kzg.evaluate_evaluations(w16, [1, 2, 3] + [0] * 14, 3)        # trailing zeros still count as values
    with pytest.raises(ValueError):
        kzg.evaluate_evaluations(3, [1, 2, 3], 3)                     # 3 is no root of unity of power-of-two order


def test_new_kernels_never_spill_and_the_opening_kernels_fit_their_budget(built):
    out, listing = kernel_resources(built)
    rows = {}
    for name, vgpr, _, _, lds, scratch in listing:
        rows.setdefault(name, []).append((vgpr, lds, scratch))
    opening = ["lagr_denom_kernel", "lagr_sums_kernel", "lagr_value_kernel", "lagr_quotient_kernel"]
    others = ["lagr_wpow_kernel", "lagr_basis_scalars_kernel", "g1_intt_load_kernel", "g1_level_kernel",
              "g1_intt_finish_kernel"]
    for name in opening + others:
        assert len(rows.get(name, [])) == 2, (name, out)              # one instantiation per curve
        for vgpr, lds, scratch in rows[name]:
            assert scratch == 0, name
            if name in opening:
                assert vgpr <= 128 and lds <= 1024, name

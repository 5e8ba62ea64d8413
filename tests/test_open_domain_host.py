"""FK20 openings without a GPU: the new C-ABI symbols are declared, exported and bound; a plain-Python restatement of
the four steps (table, Fr transform, Hadamard product, inverse G1 transform, extraction, final G1 transform) over the
oracle's group law equals the oracle's opening at every point of the domain -- which pins the key reversal, the n - 1
offset and h_(n-1) = 0 --; the facade rejects bad arguments before any device call; the new kernels fit their budget
(CPU suite)."""
import os
import random
import re
import subprocess

import pytest

from oracle import py_oracle as O
from restated import fr_dft, g1_dft, g1_mul, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")

NEW_SYMBOLS = ["kzg_domain_table_create", "kzg_domain_table_size", "kzg_domain_table_free", "kzg_open_domain",
               "kzg_open_domain_device"]
NEW_KERNELS = ["dom_load_key_kernel", "g1_level_kernel", "dom_hadamard_kernel", "dom_extract_kernel",
               "dom_finish_table_kernel", "dom_finish_proofs_kernel"]
CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba


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


# ---- the algorithm restated over the oracle's group law ------------------------------------------------------------
def fk20_restated(coeffs, ck, n, w, cv):
    """all n proofs pi(w^i) of p = sum_j coeffs[j] X^j (len <= n) against the monomial key ck (>= n points)"""
    r, nn = cv.r, 2 * n
    omega = cv.root_of_unity(nn)
    # table: s^_u = s_(n-2-u) for u <= n-2, O above; S = DFT_N(s^)
    s_hat = [ck[n - 2 - u] if u <= n - 2 else O.Z1() for u in range(nn)]
    S = g1_dft(s_hat, omega, cv)
    # per polynomial
    c_hat = fr_dft([int(c) % r for c in coeffs] + [0] * (nn - len(coeffs)), omega, r)
    ninv = pow(nn, -1, r)
    u_hat = [g1_mul(S[i], c_hat[i] * ninv, cv) for i in range(nn)]       # the 1/N rides on the scalars
    u = g1_dft(u_hat, pow(omega, -1, r), cv)
    h = [u[n - 1 + m] for m in range(n - 1)] + [O.Z1()]                   # h_(n-1) = O
    return g1_dft(h, w, cv)


def cases(n, r, rng):
    yield "random", [rng.randrange(r) for _ in range(n)]
    if n > 8:
        return
    yield "r-1", [r - 1] * n
    yield "short", [rng.randrange(r) for _ in range(max(1, n // 2 + 1) if n > 2 else 1)]
    yield "len1", [rng.randrange(r)]
    yield "zero", []


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_restated_fk20_equals_the_oracle_opening_at_every_point(curve, n):
    cv = O.curve(curve)
    rng = random.Random(n * 7 + len(curve))
    ck = O.setup(n - 1, TAU, cv)
    w = cv.root_of_unity(n)
    for name, coeffs in cases(n, cv.r, rng):
        got = fk20_restated(coeffs, ck, n, w, cv)
        for i in range(n):
            want = O.open_(ck, [coeffs], pow(w, i, cv.r), 1, cv)[0]
            assert O.normalize(got[i], cv) == O.normalize(want, cv), (name, i)
        if n == 2 and coeffs:
            assert all(O.eq(p, g1_mul(ck[0], coeffs[-1] if len(coeffs) == 2 else 0, cv), cv) for p in got), name
        if len(coeffs) <= 1:
            assert all(O.is_inf(p) for p in got), name


# ---- facade argument checks (no device call is reached) -------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_facade_rejects_bad_arguments_before_the_device(curve, monkeypatch):
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG, LagrangeKey

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_native, "get_context", no_device)
    kzg = KZG(curve)
    r = kzg.curve_order
    ck = [kzg.G1] * 16
    w16 = int(kzg.Fq.root_of_unity(16))
    with pytest.raises(ValueError):
        kzg.domain_table(ck, 12)                                          # not a power of two
    with pytest.raises(ValueError):
        kzg.domain_table(ck, 1)
    with pytest.raises(ValueError):
        kzg.domain_table(ck, 32)                                          # key shorter than the domain
    with pytest.raises(ValueError):
        kzg.domain_table(ck, 1 << 21)                                     # above 2^20
    with pytest.raises(ValueError):
        kzg.open_domain(ck, [[1, 2, 3]], 5, n=12)
    with pytest.raises(ValueError):
        kzg.open_domain(ck, [[1, 2, 3]], 5, n=16, w=w16 * w16 % r)        # an 8th root, not a primitive 16th one
    with pytest.raises(ValueError):
        kzg.open_domain_each(ck, [[1, 2, 3]], n=16, w=1)
    with pytest.raises(ValueError):
        kzg.open_domain(ck, [list(range(1, 18))], 5, n=16)                # 17 coefficients on a domain of 16
    with pytest.raises(ValueError):
        kzg.open_domain_each(ck, [list(range(1, 18))])                    # default n = 32 > the key's 16 points
    lk = LagrangeKey.__new__(LagrangeKey)
    lk.n, lk.w, lk.log_n = 16, w16, 4
    with pytest.raises(TypeError):
        kzg.open_domain(lk, [[1, 2, 3]], 5)
    with pytest.raises(TypeError):
        kzg.domain_table(lk, 16)


# ---- kernel budget -------------------------------------------------------------------------------------------------
def test_new_kernels_never_spill_and_fit_256_vgprs(built):
    out, listing = kernel_resources(built)
    rows = {}
    for name, vgpr, _, _, _, scratch in listing:
        rows.setdefault(name, []).append((vgpr, scratch))
    for name in NEW_KERNELS:
        assert "prep_" not in name
        assert len(rows.get(name, [])) == 2, (name, out)                  # one instantiation per curve
        for vgpr, scratch in rows[name]:
            assert scratch == 0 and vgpr <= 256, (name, vgpr, scratch)

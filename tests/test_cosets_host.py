"""Coset openings without a GPU: the five new C-ABI symbols are declared, exported and bound; a plain-Python
restatement of the coset FK20 (sub-tables, de-interleave, Hadamard sum, inverse G1 DFT, extraction, final DFT with
w^l) over the oracle's group law equals the oracle's commitment of (p - rho) / (X^l - a) at every coset; the
cross-identity against single-point proofs holds; the host verifier accepts oracle-made proofs and rejects tampered
ones; the facade rejects bad arguments before any device call; the new kernels fit their budget (CPU suite)."""
import os
import random
import re
import subprocess

import pytest

from oracle import py_oracle as O
from restated import fr_dft, g1_dft, g1_mul, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")

NEW_SYMBOLS = ["kzg_coset_table_create", "kzg_open_cosets", "kzg_open_cosets_device", "kzg_open_coset",
               "kzg_open_coset_device"]
NEW_KERNELS = ["dom_scale_kernel", "dom_hadsum_kernel", "dom_group_sum_kernel", "coset_tile_kernel",
               "coset_fill_kernel", "dom_load_key_kernel", "dom_extract_kernel"]
NEW_FR_KERNELS = ["dom_deinterleave_kernel", "dom_coset_values_kernel"]      # curve-independent: one instantiation
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


# ---- helpers: division, interpolation, the algorithm restated over the oracle's group law ---------------------------
def coset_divide(coeffs, l, a, r):
    """(quotient, remainder) of p by X^l - a: S_t = c_t + a S_(t+l), q_t = S_(t+l), rho_j = S_j"""
    c = [int(x) % r for x in coeffs]
    S = c + [0] * l
    for t in range(len(c) - 1, -1, -1):
        S[t] = (c[t] + a * S[t + l]) % r
    return [S[t + l] for t in range(max(len(c) - l, 0))], [S[j] for j in range(l)]


def coset_interpolate(values, h, zeta, r):
    """rho_j = h^-j l^-1 sum_k y_k zeta^(-jk)"""
    l = len(values)
    zi, hi, li = pow(zeta, -1, r), pow(h, -1, r), pow(l, -1, r)
    return [sum(y * pow(zi, j * k, r) for k, y in enumerate(values)) * li * pow(hi, j, r) % r for j in range(l)]


def coset_table_restated(ck, n, l, cv):
    """S^(j) = DFT_G1,2m(s^(j)), s^(j)_u = s_((m-2-u) l + j) for u <= m-2, O above; [l][2m]"""
    m = n // l
    omega = cv.root_of_unity(2 * m)
    return [g1_dft([ck[(m - 2 - u) * l + j] if u <= m - 2 else O.Z1() for u in range(2 * m)], omega, cv)
            for j in range(l)]


def coset_fk20_restated(coeffs, table, n, l, N, w, cv):
    """the N/l coset proofs of p (len <= n) on {w^t, t < N}, coset i = (w^i, w^(N/l))"""
    r, m = cv.r, n // l
    mm = 2 * m
    omega = cv.root_of_unity(mm)
    c = [int(x) % r for x in coeffs] + [0] * (n - len(coeffs))
    chat = [fr_dft([c[s * l + j] for s in range(m)] + [0] * m, omega, r) for j in range(l)]   # de-interleave + NTT
    inv = pow(mm, -1, r)
    u_hat = []
    for i in range(mm):                                                  # Hadamard sum over the l sub-tables
        acc = O.Z1()
        for j in range(l):
            acc = O.add(acc, g1_mul(table[j][i], chat[j][i] * inv, cv), cv)
        u_hat.append(acc)
    u = g1_dft(u_hat, pow(omega, -1, r), cv)
    hvec = [u[m - 1 + x] for x in range(m - 1)] + [O.Z1()] * (N // l - m + 1)    # extraction, O-padded to N/l
    return g1_dft(hvec, pow(w, l, r), cv)


def cases(n, l, r, rng):
    yield "random", [rng.randrange(r) for _ in range(n)]
    if n > 8:
        return
    yield "r-1", [r - 1] * n
    yield "short", [rng.randrange(r) for _ in range(max(1, l - 1))]
    yield "len1", [rng.randrange(r)]
    yield "zero", []


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [4, 8, 16])
def test_restated_coset_fk20_equals_the_oracle_at_every_coset(curve, n):
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(n * 13 + len(curve))
    ck = O.setup(n - 1, TAU, cv)
    l = 1
    while l < n:
        table = coset_table_restated(ck, n, l, cv)
        for N in (n, 2 * n):
            w = cv.root_of_unity(N)
            for name, coeffs in cases(n, l, r, rng):
                got = coset_fk20_restated(coeffs, table, n, l, N, w, cv)
                assert len(got) == N // l
                for i in range(N // l):
                    a = pow(w, i * l, r)
                    q, _ = coset_divide(coeffs, l, a, r)
                    want = O.commit(ck, [q], cv)[0]
                    assert O.eq(got[i], want, cv), (name, l, N, i)
                if len(coeffs) <= l:
                    assert all(O.is_inf(p) for p in got), (name, l)
        l *= 2


@pytest.mark.parametrize("curve", CURVES)
def test_cross_identity_with_single_point_proofs(curve):
    """pi_i = sum_k (x_k / (l a_i)) pi(x_k): coset proofs from open_domain-style single-point proofs"""
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(3)
    n = 8
    ck = O.setup(n - 1, TAU, cv)
    p = [rng.randrange(r) for _ in range(n)]
    for l, N in ((2, 8), (4, 16)):
        w = cv.root_of_unity(N)
        single = [O.open_(ck, [p], pow(w, t, r), 1, cv)[0] for t in range(N)]
        for i in range(N // l):
            a = pow(w, i * l, r)
            q, _ = coset_divide(p, l, a, r)
            want = O.commit(ck, [q], cv)[0]
            acc = O.Z1()
            for k in range(l):
                t = i + k * (N // l)
                acc = O.add(acc, g1_mul(single[t], pow(w, t, r) * pow(l * a, -1, r), cv), cv)
            assert O.eq(acc, want, cv), (l, N, i)


def test_division_and_interpolation_helpers_agree():
    r = O.curve("bn254").r
    rng = random.Random(5)
    for l in (1, 2, 4, 8):
        zeta = O.curve("bn254").root_of_unity(l)
        h = rng.randrange(1, r)
        p = [rng.randrange(r) for _ in range(19)]
        q, rho = coset_divide(p, l, pow(h, l, r), r)
        ys = [O.poly_eval(p, h * pow(zeta, k, r) % r, r) for k in range(l)]
        assert coset_interpolate(ys, h, zeta, r) == rho
        x = rng.randrange(r)                                             # p = q Z + rho at a random point
        assert O.poly_eval(p, x, r) == (O.poly_eval(q, x, r) * (pow(x, l, r) - pow(h, l, r)) + O.poly_eval(rho, x, r)) % r


# ---- host verifier on oracle-made proofs (few pairings: one small key, l in {1, 4}) ---------------------------------
def _oracle_coset_proof(ck, polys, h, l, xi, cv):
    r = cv.r
    comb = O.combine(polys, xi, r)
    q, _ = coset_divide(comb, l, pow(h, l, r), r)
    return O.normalize(O.commit(ck, [q], cv)[0], cv)


@pytest.mark.parametrize("curve", ["bn254"])
def test_host_verifier_accepts_oracle_proofs_and_rejects_tampering(curve):
    from kzg_snark_amd.kzg import KZG
    kzg = KZG(curve)
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(17)
    n = 8
    ck = [O.normalize(p, cv) for p in O.setup(n - 1, TAU, cv)]
    ck = [(x, y, 1) for x, y, *_ in ck]
    polys = [[rng.randrange(r) for _ in range(n)], [rng.randrange(r) for _ in range(5)]]
    comms = [O.normalize(c, cv) for c in O.commit(ck, polys, cv)]
    comms = [(x, y, 1) for x, y, *_ in comms]
    xi, l = rng.randrange(r), 4
    zeta = int(kzg.Fq.root_of_unity(l))
    h = rng.randrange(1, r)
    vals = [[O.poly_eval(p, h * pow(zeta, k, r) % r, r) for k in range(l)] for p in polys]
    x, y, *_ = _oracle_coset_proof(ck, polys, h, l, xi, cv)
    proof = (x, y, 1)
    rk4 = kzg.coset_verification_key(l, TAU)
    assert kzg.coset_verification_key(1, TAU) == kzg.multiply(kzg.G2, TAU)
    assert kzg.check_coset(ck, rk4, comms, h, vals, proof, xi)
    bad = [v[:] for v in vals]
    bad[1][2] = (bad[1][2] + 1) % r
    assert not kzg.check_coset(ck, rk4, comms, h, bad, proof, xi)                       # a changed value
    assert not kzg.check_coset(ck, rk4, comms, h, vals, kzg.add(proof, kzg.G1), xi)    # a changed proof
    assert not kzg.check_coset(ck, rk4, comms, h + 1, vals, proof, xi)                 # a wrong h
    assert not kzg.check_coset(ck, kzg.coset_verification_key(2, TAU), comms, h, vals, proof, xi)  # rk of another l
    # batch: two claims, one weight; then one tampered value
    h2 = rng.randrange(1, r)
    vals2 = [[O.poly_eval(polys[0], h2 * pow(zeta, k, r) % r, r) for k in range(l)]]
    x2, y2, *_ = _oracle_coset_proof(ck, polys[:1], h2, l, 1, cv)
    args = (ck, rk4, [comms, comms[:1]], [h, h2], [vals, vals2], [proof, (x2, y2, 1)], [xi, 1])
    assert kzg.batch_check_cosets(*args, r=12345)
    bad2 = [[(vals2[0][0] + 1) % r] + vals2[0][1:]]
    assert not kzg.batch_check_cosets(ck, rk4, [comms, comms[:1]], [h, h2], [vals, bad2], [proof, (x2, y2, 1)],
                                      [xi, 1], r=12345)


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
        kzg.coset_table(ck, 16, 3)                                         # l not a power of two
    with pytest.raises(ValueError):
        kzg.coset_table(ck, 16, 16)                                        # l > n/2
    with pytest.raises(ValueError):
        kzg.coset_table(ck, 32, 4)                                         # key shorter than the domain
    with pytest.raises(ValueError):
        kzg.coset_table(ck, 12, 4)
    with pytest.raises(ValueError):
        kzg.open_cosets(ck, [[1, 2, 3]], 5, 4, n=16, N=8)                  # N < n
    with pytest.raises(ValueError):
        kzg.open_cosets(ck, [[1, 2, 3]], 5, 4, n=16, N=128)                # N > 4n
    with pytest.raises(ValueError):
        kzg.open_cosets(ck, [[1, 2, 3]], 5, 4, n=16, w=w16 * w16 % r)      # not a primitive 16th root
    with pytest.raises(ValueError):
        kzg.open_cosets_each(ck, [list(range(1, 18))], 4, n=16)            # 17 coefficients on a domain of 16
    with pytest.raises(ValueError):
        kzg.open_cosets_each(ck, [[1, 2]], 16, n=16)                       # l > n/2
    with pytest.raises(ValueError):
        kzg.open_coset(ck, [[1, 2, 3]], 0, 4, 5)                           # h = 0
    with pytest.raises(ValueError):
        kzg.open_coset(ck, [[1, 2, 3]], 7, 4, 5, zeta=w16)                 # a 16th root, not a primitive 4th one
    with pytest.raises(ValueError):
        kzg.open_coset(ck, [[1, 2, 3]], 7, 1, 5, zeta=r - 1)               # l = 1 needs zeta = 1
    with pytest.raises(ValueError):
        kzg.open_coset(ck, [[1, 2, 3]], 7, 1 << 13, 5)                     # l above 2^12
    with pytest.raises(ValueError):
        kzg.open_coset(ck, [list(range(1, 18))], 7, 4, 5)                  # longer than the key
    with pytest.raises(ValueError):
        kzg.open_coset(ck, [[1, 2, 3]], 7, 6, 5)                           # l not a power of two
    lk = LagrangeKey.__new__(LagrangeKey)
    lk.n, lk.w, lk.log_n = 16, w16, 4
    with pytest.raises(TypeError):
        kzg.open_cosets(lk, [[1, 2, 3]], 5, 4)
    with pytest.raises(TypeError):
        kzg.coset_table(lk, 16, 4)
    with pytest.raises(TypeError):
        kzg.open_coset(lk, [[1, 2, 3]], 7, 4, 5)


# ---- kernel budget -------------------------------------------------------------------------------------------------
def test_new_kernels_never_spill_and_fit_256_vgprs(built):
    out, listing = kernel_resources(built)
    rows = {}
    for raw, vgpr, _, _, _, scratch in listing:
        k = re.search(r"(\w+_kernel)\b", raw)                             # demangled or plain
        rows.setdefault(k.group(1) if k else raw, []).append((vgpr, scratch))
    for names, count in ((NEW_KERNELS, 2), (NEW_FR_KERNELS, 1)):
        for name in names:
            assert len(rows.get(name, [])) == count, (name, out)
            for vgpr, scratch in rows[name]:
                assert scratch == 0 and vgpr <= 256, (name, vgpr, scratch)

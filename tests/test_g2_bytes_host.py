"""Compressed G2 points, the square root in Fp2, the two subgroup tests and the trusted-setup text format on the CPU:
curve.py's single-point helpers against the public byte formats and the golden file; csrc/g2_bytes.h -- the text the
gfx950 kernels compile -- built for the host (tests/shim/g2_bytes_shim.cpp) against those helpers and Python integers,
plain and with -DKZG_AUDIT (field.h's column and precondition hooks must stay silent); the parser of trusted-setup
files on well-formed and broken texts."""
import ctypes
import os
import random
import re

import pytest

from g2_bytes_cases import (CURVE_IDS, INF2, build_shim, fp_words, g2_generator, golden, golden_failures, golden_points,
                            golden_real_rhs, point_value, random_twist_point, subgroup_matrix_g2, twist_rhs, value_point)
from kzg_snark_amd import curve as C
from limb_patterns import adversarial, header_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = ctypes.c_uint32
FP_STRUCT = {"bn254": "BnFp", "bls12_381": "BlsFp"}
CURVES = ["bls12_381", "bn254"]
NEW_SYMBOLS = ["kzg_g2_compress", "kzg_g2_decompress", "kzg_g2_decompress_device", "kzg_g2_check_subgroup"]


# ---- the interface ------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound():
    from kzg_snark_amd import _native
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    api = open(os.path.join(ROOT, "kzg_snark_amd", "csrc", "api.hip")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(kzg_ctx\* ctx" % name, header, re.M), name
        assert re.search(r"^int %s\(kzg_ctx\* ctx" % name, api, re.M), name
        assert name in _native.SIGNATURES, name
        assert hasattr(_native.lib(), name), name
    assert _native.lib().kzg_abi_version() == 1
    for method in ("g2_compress", "g2_decompress", "g2_decompress_device", "g2_check_subgroup", "g2_bytes"):
        assert hasattr(_native.Context, method), method
    from kzg_snark_amd.kzg import KZG
    for method in ("compress_g2", "decompress_g2", "in_subgroup_g2", "setup_g2", "save_trusted_setup",
                   "load_trusted_setup", "check_key"):
        assert callable(getattr(KZG, method)), method


# ---- the Python helpers ---------------------------------------------------------------------------------------------

def test_helpers_match_the_public_encodings():
    cv = C.BLS12_381
    pin = golden()["pins"]["bls12_381_g2_generator"]
    assert pin.startswith("93e02b6052719f60") and pin.endswith("d48056c8c121bdb8") and len(pin) == 192
    g = g2_generator(cv)
    assert C.compress_g2(g, cv).hex() == pin
    assert C.decompress_g2(bytes.fromhex(pin), cv) == g
    assert C.compress_g2(INF2, cv).hex() == "c0" + "00" * 95 and C.compress_g2(INF2, C.BN254).hex() == "40" + "00" * 63
    assert C.g2_compressed_size(cv) == 96 and C.g2_compressed_size(C.BN254) == 64
    assert set(C.G2_STATUS_TEXT) == {0, 1, 2, 3}


@pytest.mark.parametrize("name", CURVES)
def test_helpers_against_the_golden_file(name):
    cv = C.CURVES[name]
    pts = golden_points(name)
    assert len(pts) >= 9
    assert {C._fp2_larger(pt[1], cv.p) for _, pt in pts if pt[2] != (0, 0)} == {True, False}
    for blob, pt in pts:
        assert len(blob) == C.g2_compressed_size(cv)
        assert C.compress_g2(pt, cv) == blob and C.decompress_g2_status(blob, cv) == (pt, 0)
    real = golden_real_rhs(name)
    assert {k for _, _, k in real} == {"residue", "non-residue"}
    assert any(pt[1][1] == 0 for _, pt, _ in real) and any(pt[1][0] == 0 for _, pt, _ in real)
    for blob, pt, kind in real:
        assert twist_rhs(pt[0], cv)[1] == 0 and C.on_curve_g2(pt, cv)
        assert C.compress_g2(pt, cv) == blob and C.decompress_g2_status(blob, cv, check_subgroup=False) == (pt, 0)
    fails = golden_failures(name)
    assert {st for _, st, _ in fails} == {1, 2, 3}
    cases = " | ".join(c for _, st, c in fails if st == 1)
    for needle in ("top bits 00", "infinity with", "x.c1 = p", "x.c0 = p", "first failure wins"):
        assert needle in cases, needle
    for blob, st, case in fails:
        assert C.decompress_g2_status(blob, cv) == (None, st), case
        with pytest.raises(ValueError):
            C.decompress_g2(blob, cv)
        if st == 3:
            pt, st0 = C.decompress_g2_status(blob, cv, check_subgroup=False)
            assert st0 == 0 and C.on_curve_g2(pt, cv) and C.compress_g2(pt, cv) == blob


@pytest.mark.parametrize("name", CURVES)
def test_sqrt_fp2_helper(name):
    p = C.CURVES[name].p
    rng = random.Random(3)
    for _ in range(32):
        s = (rng.randrange(p), rng.randrange(p))
        a = C._fp2_mul(s, s, p)
        root = C.sqrt_fp2(a, p)
        assert root in (s, ((-s[0]) % p, (-s[1]) % p))
    assert C.sqrt_fp2((0, 0), p) == (0, 0)
    assert C.sqrt_fp2((p - 1, 0), p) in ((0, 1), (0, p - 1))                   # sqrt(-1) = i


# ---- g2_bytes.h on the host -----------------------------------------------------------------------------------------

class Shim:
    def __init__(self, lib, audit):
        self.lib, self.audit = lib, audit
        if audit:
            lib.g2b_audit_read.restype = ctypes.c_ulonglong
            lib.g2b_audit_reset()

    def assert_clean(self):
        if not self.audit:
            return
        fn, what, line = ctypes.create_string_buffer(128), ctypes.create_string_buffer(160), ctypes.c_int(0)
        n = self.lib.g2b_audit_read(fn, what, 128, ctypes.byref(line))
        assert n == 0, f"{n} violations, first in {fn.value.decode()} (line {line.value}): {what.value.decode()}"

    @staticmethod
    def words(x, nw):
        return (U32 * nw)(*[(x >> (32 * i)) & 0xffffffff for i in range(nw)])

    @staticmethod
    def val(w):
        return sum(int(v) << (32 * i) for i, v in enumerate(w))

    def sqrt(self, cid, a, nw):
        out = (U32 * (2 * nw))()
        ok = self.lib.g2b_sqrt(cid, self.words(a[0] | (a[1] << (32 * nw)), 2 * nw), out)
        assert ok in (0, 1)
        v = self.val(out)
        return bool(ok), (v & ((1 << (32 * nw)) - 1), v >> (32 * nw))

    def decode(self, cid, blob, check, nw):
        xy, inf = (U32 * (4 * nw))(), ctypes.c_int(0)
        st = self.lib.g2b_decode(cid, bytes(blob), int(check), xy, ctypes.byref(inf))
        return st, value_point(self.val(xy), nw, bool(inf.value))

    def encode(self, cid, pt, nw):
        out = ctypes.create_string_buffer(8 * nw)
        assert self.lib.g2b_encode(cid, self.words(point_value(pt, nw), 4 * nw), int(pt[2] == (0, 0)), out) == 0
        return out.raw

    def check(self, cid, pt, nw):
        return self.lib.g2b_check(cid, self.words(point_value(pt, nw), 4 * nw), int(pt[2] == (0, 0)))


ZERO_PT = ((0, 0), (0, 0), (1, 0))                       # what a failed decompression leaves: zeros, flag 0


@pytest.fixture(scope="module", params=["plain", "audit"])
def shim(request):
    audit = request.param == "audit"
    return Shim(build_shim(audit), audit)


@pytest.mark.parametrize("name", CURVES)
def test_fp2_sqrt_against_python(shim, name):
    cv, cid = C.CURVES[name], CURVE_IDS[name]
    p, nw = cv.p, fp_words(cv)
    assert shim.lib.g2b_size(cid) == 8 * nw == C.g2_compressed_size(cv)
    L, N = header_layout(FP_STRUCT[name])
    rng = random.Random(cid + 17)
    neg = lambda v: ((-v[0]) % p, (-v[1]) % p)
    sq = lambda v: C._fp2_mul(v, v, p)

    def expect_root(a):
        ok, root = shim.sqrt(cid, a, nw)
        assert ok and sq(root) == (a[0] % p, a[1] % p), a
        assert root in (C.sqrt_fp2(a, p), neg(C.sqrt_fp2(a, p)))
        return root

    squares = [sq((rng.randrange(p), rng.randrange(p))) for _ in range(64)]
    for a in squares:
        expect_root(a)
    # a non-square: a square times the non-residue xi (its norm is a non-residue of Fp on both curves)
    xi = (9, 1) if name == "bn254" else (1, 1)
    assert C.sqrt_fp2(xi, p) is None
    for a in squares:
        b = C._fp2_mul(a, xi, p)
        assert C.sqrt_fp2(b, p) is None
        assert shim.sqrt(cid, b, nw) == (False, (0, 0))
    assert shim.sqrt(cid, (0, 0), nw) == (True, (0, 0))
    # real input: a residue of Fp has a real root, a non-residue a purely imaginary one
    limbs = adversarial(p, L, N, 1, count=12, seed=cid + 3)
    reals = [1, 2, 3, 4, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2] + [v for v in limbs if v] + [rng.randrange(1, p) for _ in range(8)]
    kinds = set()
    for a0 in reals:
        root = expect_root((a0, 0))
        residue = C.sqrt_fp(a0, p) is not None
        assert (root[1] == 0 and root[0] != 0) if residue else (root[0] == 0 and root[1] != 0), a0
        kinds.add(residue)
    assert kinds == {True, False}
    # all-ones limbs at the top of the canonical range in both components, and their squares
    for a0, a1 in zip(limbs, reversed(limbs)):
        want = C.sqrt_fp2((a0, a1), p)
        ok, root = shim.sqrt(cid, (a0, a1), nw)
        assert ok == (want is not None) and (not ok or sq(root) == (a0, a1))
        expect_root(sq((a0, a1)))
    shim.assert_clean()


@pytest.mark.parametrize("name", CURVES)
def test_both_sign_conventions_and_the_special_branches_through_decompression(shim, name):
    cv, cid = C.CURVES[name], CURVE_IDS[name]
    nw = fp_words(cv)
    K = C._Fp2(cv.p)
    for blob, pt, kind in golden_real_rhs(name):                 # x^3 + b' in Fp: a real or a purely imaginary y
        for q in (pt, (pt[0], K.neg(pt[1]), pt[2])):
            b = C.compress_g2(q, cv)
            assert shim.encode(cid, q, nw) == b
            assert shim.decode(cid, b, False, nw) == (0, q), kind
            assert shim.decode(cid, b, True, nw) == (3, ZERO_PT), kind
    rng = random.Random(23)
    for _ in range(6):                                           # y of either sign decodes to itself
        pt = random_twist_point(cv, rng)
        for q in (pt, (pt[0], K.neg(pt[1]), pt[2])):
            assert shim.decode(cid, C.compress_g2(q, cv), False, nw) == (0, q)
    shim.assert_clean()


@pytest.mark.parametrize("name", CURVES)
def test_subgroup_tests_against_r_times_q(shim, name):
    """psi(Q) = [u] Q (bls12_381) and [u+1] Q + psi([u] Q) + psi^2([u] Q) = psi^3([2u] Q) (bn254) agree with
    [r] Q = O on the whole matrix."""
    cv, cid = C.CURVES[name], CURVE_IDS[name]
    nw = fp_words(cv)
    rows = subgroup_matrix_g2(name)
    assert sum(1 for _, ok, _ in rows if not ok) >= 48 and sum(1 for _, ok, _ in rows if ok) >= 17
    for pt, want, what in rows:
        assert shim.check(cid, pt, nw) == (0 if want else 3), what
        if pt[2] != (0, 0):
            blob = C.compress_g2(pt, cv)
            assert shim.decode(cid, blob, True, nw) == ((0, pt) if want else (3, ZERO_PT)), what
            assert shim.decode(cid, blob, False, nw) == (0, pt), what
    g = g2_generator(cv)
    assert shim.check(cid, (g[0], (g[1][0] ^ 1, g[1][1]), g[2]), nw) == 2           # off the twist
    assert shim.check(cid, ((g[0][0] + cv.p, g[0][1]), g[1], g[2]), nw) == 2          # a coordinate >= p
    shim.assert_clean()


@pytest.mark.parametrize("name", CURVES)
def test_encode_and_decode_of_every_golden_vector(shim, name):
    cv, cid = C.CURVES[name], CURVE_IDS[name]
    nw = fp_words(cv)
    for blob, pt in golden_points(name):
        assert shim.encode(cid, pt, nw) == blob
        assert shim.decode(cid, blob, True, nw) == (0, pt) and shim.decode(cid, blob, False, nw) == (0, pt)
    for blob, st, case in golden_failures(name):
        assert shim.decode(cid, blob, True, nw) == (st, ZERO_PT), case
        want = C.decompress_g2_status(blob, cv, check_subgroup=False)
        assert shim.decode(cid, blob, False, nw) == (want[1], want[0] or ZERO_PT), case
    shim.assert_clean()


# ---- trusted-setup text ---------------------------------------------------------------------------------------------

def _setup_text(name, n1=4, n2=3, tau=0x1234567):
    """a small honest file from curve.py alone (pure-Python stand-ins for the device calls): the Lagrange points by the
    inverse transform of the monomial ones written out, every point compressed by the helpers"""
    from kzg_snark_amd.field import GF
    from kzg_snark_amd.kzg import format_trusted_setup
    cv = C.CURVES[name]
    G1, G2 = C.g1_group(cv), C.g2_group(cv)
    g1, g2 = (cv.g1[0], cv.g1[1], 1), g2_generator(cv)
    r = cv.r
    w = int(GF(r).root_of_unity(n1))
    lag = []
    for i in range(n1):                                  # L_i(tau) = (tau^n - 1) w^i / (n (tau - w^i))
        wi = pow(w, i, r)
        lag.append((pow(tau, n1, r) - 1) * wi * pow(n1 * (tau - wi), -1, r) % r)
    mono = [C.compress_g1(G1.multiply(g1, pow(tau, i, r)), cv) for i in range(n1)]
    lagb = [C.compress_g1(G1.multiply(g1, v), cv) for v in lag]
    g2b = [C.compress_g2(G2.multiply(g2, pow(tau, j, r)), cv) for j in range(n2)]
    return format_trusted_setup(lagb, g2b, mono), lagb, g2b, mono


@pytest.mark.parametrize("name", CURVES)
def test_trusted_setup_text_round_trip(name):
    from kzg_snark_amd.kzg import bit_reverse_rows, parse_trusted_setup
    import numpy as np
    cv = C.CURVES[name]
    s1, s2 = C.g1_compressed_size(cv), C.g2_compressed_size(cv)
    text, lagb, g2b, mono = _setup_text(name)
    for t in (text, "\n  " + text.replace("\n", "  \n\n\t"), text.upper().replace("\n", "\r\n")):
        n1, n2, a, b, c = parse_trusted_setup(t, s1, s2)
        assert (n1, n2) == (4, 3)
        assert [r.tobytes() for r in a] == lagb and [r.tobytes() for r in b] == g2b and [r.tobytes() for r in c] == mono
    # the decoded sections are one tau: the sum of the Lagrange points is [1] G1 and point 1 of each chain is [tau]
    G1 = C.g1_group(cv)
    total = G1.Z
    for blob in lagb:
        total = G1.add(total, C.decompress_g1(blob, cv))
    assert total == (cv.g1[0], cv.g1[1], 1) == C.decompress_g1(mono[0], cv)
    assert C.decompress_g2(g2b[0], cv) == g2_generator(cv)
    rows = np.arange(8).reshape(8, 1)
    assert bit_reverse_rows(rows).reshape(-1).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]
    assert (bit_reverse_rows(bit_reverse_rows(rows)) == rows).all()


def test_trusted_setup_text_errors_name_the_line_or_section():
    from kzg_snark_amd.kzg import parse_trusted_setup
    name = "bn254"
    cv = C.CURVES[name]
    s1, s2 = C.g1_compressed_size(cv), C.g2_compressed_size(cv)
    text, _, _, _ = _setup_text(name)
    lines = text.splitlines()
    assert len(lines) == 2 + 4 + 3 + 4

    def broken(new_lines, match):
        with pytest.raises(ValueError, match=match):
            parse_trusted_setup("\n".join(new_lines) + "\n", s1, s2)

    broken(lines[:-2], r"truncated in the G1 monomial section: 2 of 4")                 # a truncated file
    broken(lines[:7], r"truncated in the G2 section: 1 of 3")
    broken(lines[:1], r"ends before the two counts")
    broken(["4", "2"] + lines[2:], r"line 9 \(G1 monomial section, point 0\): 128 hex digits, expected 64")   # a wrong count
    broken(lines + [lines[-1]], r"line 14: 1 lines more than the counts n1 = 4, n2 = 3")
    broken(["4", "4"] + lines[2:], r"line 10 \(G2 section, point 3\): 64 hex digits, expected 128")
    broken(lines[:4] + ["zz" + lines[4][2:]] + lines[5:], r"line 5 \(G1 Lagrange section, point 2\): not hexadecimal")
    broken(lines[:7] + [lines[7][:-2]] + lines[8:], r"line 8 \(G2 section, point 1\): 126 hex digits, expected 128")
    broken(lines[:9] + [lines[9] + "00"] + lines[10:], r"line 10 \(G1 monomial section, point 0\): 66 hex digits")
    broken(["3", "3"] + lines[2:], r"line 1: n1 = 3 is not a power of two")             # a non-power-of-two n1
    broken(["4", "x"] + lines[2:], r"line 2: expected n2")
    broken(["4", "0"] + lines[2:], r"line 2: n2 = 0")

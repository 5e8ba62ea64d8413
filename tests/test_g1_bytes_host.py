"""Compressed G1 points and the subgroup test on the CPU: curve.py's single-point helpers against the public byte
formats and the golden file, and csrc/g1_bytes.h -- the text the gfx950 kernels compile -- built for the host
(tests/shim/g1_bytes_shim.cpp) against those helpers and Python integers.  The shim runs plain and with -DKZG_AUDIT
(field.h's column and precondition hooks must stay silent), and once as a program of its own under the address and
undefined-behaviour sanitizers."""
import ctypes
import os
import random
import subprocess

import pytest

from g1_bytes_cases import (CURVE_IDS, build_shim, golden, golden_failures, golden_points, key_point_with_x_plus_p,
                            subgroup_matrix)
from kzg_snark_amd import curve as C
from limb_patterns import adversarial, header_layout

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "shim")
SRC = os.path.join(SHIM_DIR, "g1_bytes_shim.cpp")
U32 = ctypes.c_uint32
FP_STRUCT = {"bn254": "BnFp", "bls12_381": "BlsFp"}


# ---- the Python helpers ---------------------------------------------------------------------------------------

def test_helpers_match_the_public_encodings():
    cv = C.BLS12_381
    pins = golden()["pins"]
    g = (cv.g1[0], cv.g1[1], 1)
    assert C.compress_g1(g, cv).hex() == pins["bls12_381_generator"]
    assert pins["bls12_381_generator"].startswith("97f1d3a7") and pins["bls12_381_generator"].endswith("db22c6bb")
    assert C.compress_g1((1, 1, 0), cv).hex() == pins["bls12_381_infinity"] == "c0" + "00" * 47
    assert C.decompress_g1(bytes.fromhex(pins["bls12_381_generator"]), cv) == g
    assert C.decompress_g1(bytes.fromhex(pins["bls12_381_infinity"]), cv) == (1, 1, 0)
    bn = C.BN254
    assert C.compress_g1((1, 2, 1), bn).hex() == "80" + "00" * 30 + "01"            # y = 2 is the smaller root
    assert C.compress_g1((1, bn.p - 2, 1), bn).hex() == "c0" + "00" * 30 + "01"
    assert C.compress_g1((1, 1, 0), bn).hex() == "40" + "00" * 31


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_helpers_against_the_golden_file(name):
    cv = C.CURVES[name]
    pts = golden_points(name)
    assert {pt[1] > (cv.p - 1) // 2 for _, pt in pts if pt[2]} == {True, False}       # both signs of y
    for blob, pt in pts:
        assert len(blob) == C.g1_compressed_size(cv)
        assert C.compress_g1(pt, cv) == blob
        assert C.decompress_g1_status(blob, cv) == (pt, 0)
    fails = golden_failures(name)
    assert {st for _, st, _ in fails} == ({1, 2, 3} if name == "bls12_381" else {1, 2})
    for blob, st, case in fails:
        assert C.decompress_g1_status(blob, cv) == (None, st), case
        with pytest.raises(ValueError):
            C.decompress_g1(blob, cv)
        if st == 3:                                                        # on the curve: fine without the check
            pt, st0 = C.decompress_g1_status(blob, cv, check_subgroup=False)
            assert st0 == 0 and C.on_curve_g1(pt, cv) and C.compress_g1(pt, cv) == blob


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_helpers_round_trip(name):
    cv = C.CURVES[name]
    G = C.g1_group(cv)
    rng = random.Random(11)
    g = (cv.g1[0], cv.g1[1], 1)
    for _ in range(12):
        pt = G.multiply(g, rng.randrange(1, cv.r))
        for q in (pt, G.neg(pt)):
            assert C.decompress_g1(C.compress_g1(q, cv), cv) == q
            assert C.in_subgroup_g1(q, cv)
    assert C.decompress_g1(C.compress_g1(G.Z, cv), cv) == G.Z


# ---- g1_bytes.h on the host -------------------------------------------------------------------------------------

class Shim:
    def __init__(self, lib, audit):
        self.lib, self.audit = lib, audit
        if audit:
            lib.gb_audit_read.restype = ctypes.c_ulonglong
            lib.gb_audit_reset()

    def assert_clean(self):
        if not self.audit:
            return
        fn, what, line = ctypes.create_string_buffer(128), ctypes.create_string_buffer(160), ctypes.c_int(0)
        n = self.lib.gb_audit_read(fn, what, 128, ctypes.byref(line))
        assert n == 0, f"{n} violations, first in {fn.value.decode()} (line {line.value}): {what.value.decode()}"

    @staticmethod
    def words(x, nw):
        return (U32 * nw)(*[(x >> (32 * i)) & 0xffffffff for i in range(nw)])

    @staticmethod
    def val(w):
        return sum(int(v) << (32 * i) for i, v in enumerate(w))

    def sqrt(self, cid, a, nw):
        out = (U32 * nw)()
        ok = self.lib.gb_sqrt(cid, self.words(a, nw), out)
        assert ok in (0, 1)
        return bool(ok), self.val(out)

    def decode(self, cid, blob, check, nw):
        xy, inf = (U32 * (2 * nw))(), ctypes.c_int(0)
        st = self.lib.gb_decode(cid, bytes(blob), int(check), xy, ctypes.byref(inf))
        v = self.val(xy)
        return st, ((1, 1, 0) if inf.value else (v & ((1 << (32 * nw)) - 1), v >> (32 * nw), 1))

    def encode(self, cid, pt, nw):
        out = ctypes.create_string_buffer(4 * nw)
        inf = pt[2] == 0
        xy = self.words(0 if inf else pt[0] | (pt[1] << (32 * nw)), 2 * nw)
        assert self.lib.gb_encode(cid, xy, int(inf), out) == 0
        return out.raw

    def check(self, cid, pt, nw):
        inf = pt[2] == 0
        return self.lib.gb_check(cid, self.words(0 if inf else pt[0] | (pt[1] << (32 * nw)), 2 * nw), int(inf))


@pytest.fixture(scope="module", params=["plain", "audit"])
def shim(request):
    audit = request.param == "audit"
    return Shim(build_shim(audit), audit)


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_fp_sqrt_against_python(shim, name):
    cv, cid = C.CURVES[name], CURVE_IDS[name]
    p = cv.p
    nw = (p.bit_length() + 31) // 32
    assert shim.lib.gb_size(cid) == 4 * nw == C.g1_compressed_size(cv)
    L, N = header_layout(FP_STRUCT[name])
    rng = random.Random(cid + 7)
    ops = [0, 1, 2, 3, 4, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2] + adversarial(p, L, N, 1, count=24, seed=cid + 1)
    ops += [rng.randrange(p) for _ in range(24)]
    ops += [s * s % p for s in adversarial(p, L, N, 1)]                         # residues with adversarial roots
    seen = set()
    for a in ops:
        assert 0 <= a < p
        want = C.sqrt_fp(a, p)
        ok, root = shim.sqrt(cid, a, nw)
        assert ok == (want is not None), hex(a)
        assert root == pow(a, (p + 1) // 4, p), hex(a)                          # the candidate, square or not
        if ok:
            assert root * root % p == a
        seen.add(ok)
    assert seen == {True, False}
    assert shim.sqrt(cid, 0, nw) == (True, 0) and shim.sqrt(cid, 1, nw)[0] and not shim.sqrt(cid, p - 1, nw)[0]
    shim.assert_clean()


def test_subgroup_test_against_r_times_p(shim):
    """phi(P) = -[u^2] P agrees with [r] P = O on the whole matrix (bls12_381)."""
    nw = 12
    for pt, want, what in subgroup_matrix():
        assert shim.check(1, pt, nw) == (0 if want else 3), what
        if pt[2]:                                                              # the same through the blob
            blob = C.compress_g1(pt, C.BLS12_381)
            st, got = shim.decode(1, blob, True, nw)
            assert st == (0 if want else 3) and got == (pt if want else (0, 0, 1)), what
            assert shim.decode(1, blob, False, nw) == (0, pt), what
    # a coordinate >= p or a point off the curve: 2
    g = C.BLS12_381.g1
    assert shim.check(1, (g[0], g[1] ^ 1, 1), nw) == 2
    assert shim.check(1, (g[0] + C.BLS12_381.p, g[1], 1), nw) == 2
    shim.assert_clean()


def test_bn254_every_point_of_the_curve_is_in_the_subgroup(shim):
    cv = C.BN254
    rng = random.Random(5)
    from g1_bytes_cases import random_curve_point
    for _ in range(16):
        pt = random_curve_point(cv, rng)
        assert C.in_subgroup_g1(pt, cv)
        assert shim.check(0, pt, 8) == 0
        assert shim.decode(0, C.compress_g1(pt, cv), True, 8) == (0, pt)
    assert shim.check(0, (1, 3, 1), 8) == 2
    shim.assert_clean()


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_encode_and_decode_of_every_golden_vector(shim, name):
    cv, cid = C.CURVES[name], CURVE_IDS[name]
    nw = C.g1_compressed_size(cv) // 4
    for blob, pt in golden_points(name):
        assert shim.encode(cid, pt, nw) == blob
        assert shim.decode(cid, blob, True, nw) == (0, pt)
        assert shim.decode(cid, blob, False, nw) == (0, pt)
    for blob, st, case in golden_failures(name):
        assert shim.decode(cid, blob, True, nw) == (st, (0, 0, 1)), case          # zeros, flag 0
        want = C.decompress_g1_status(blob, cv, check_subgroup=False)
        assert shim.decode(cid, blob, False, nw) == (want[1], want[0] or (0, 0, 1)), case
    shim.assert_clean()


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_words_codec_of_g1_words_h(shim, name):
    """import_affine (the rule: both coordinates below p, on the curve), affine_to_words o affine_from_words, and the
    rule of key loading (the curve equation alone, modulo p) at the edges of the canonical range."""
    cv, cid = C.CURVES[name], CURVE_IDS[name]
    p = cv.p
    nw = (p.bit_length() + 31) // 32
    gx, gy = cv.g1

    def xy(x, y):
        return shim.words(x | (y << (32 * nw)), 2 * nw)

    def round_trip(x, y, inf=0):
        out = (U32 * (2 * nw))()
        flag = shim.lib.gb_words_round_trip(cid, xy(x, y), inf, out)
        v = shim.val(out)
        return flag, v & ((1 << (32 * nw)) - 1), v >> (32 * nw)

    ones = (1 << (32 * nw)) - 1
    assert shim.lib.gb_import(cid, xy(gx, gy)) == 1 and round_trip(gx, gy) == (0, gx, gy)
    assert shim.lib.gb_import(cid, xy(p, gy)) == 0                              # x = p
    assert shim.lib.gb_import(cid, xy(gx, p)) == 0                              # y = p
    assert ((p - 1) ** 3 + cv.b - gy * gy) % p != 0
    assert shim.lib.gb_import(cid, xy(p - 1, gy)) == 0                          # in range, off the curve
    assert shim.lib.gb_key_rule(cid, xy(p - 1, gy)) == 0
    assert shim.lib.gb_import(cid, xy(ones, ones)) == 0                         # all-ones words
    assert round_trip(ones, ones, inf=1) == (1, 0, 0)                           # the flag wins over stray words
    assert round_trip(ones, ones) == (0, ones % p, ones % p)                    # unchecked: modulo p
    # x + p fits the words; the rule refuses it, key loading takes it for x (the expectation of the GPU test
    # test_key_loading_and_compression_differ_on_a_coordinate_above_p)
    x2, y2 = key_point_with_x_plus_p(cv)
    assert x2 < 1 << (32 * nw)
    assert shim.lib.gb_import(cid, xy(x2 - p, y2)) == 1 and shim.lib.gb_import(cid, xy(x2, y2)) == 0
    assert shim.lib.gb_key_rule(cid, xy(x2, y2)) == 1
    assert round_trip(x2, y2) == (0, x2 - p, y2)
    shim.assert_clean()


def test_shim_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """g1_bytes_shim.cpp with its own main(): encode / decode / subgroup test / square roots / the canonical-words codec
    on both curves, built with
    -DKZG_AUDIT and -fsanitize=address,undefined (no recovery, static runtimes) and run as a program of its own.  Exit
    status 0 = no sanitizer report, no audit violation, every check of the program passed."""
    exe = str(tmp_path / "g1_bytes_shim_san")
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-DKZG_AUDIT", "-DG1_BYTES_SHIM_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert "no violations" in res.stdout

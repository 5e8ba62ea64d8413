"""The limb-level bounds of csrc/field.h and csrc/ec.h, pinned on the CPU.

tests/shim/bounds_shim.cpp drives the SAME headers the gfx950 kernels compile with RAW limbs, built with -DKZG_AUDIT:
every call runs the pre/postcondition hooks of field.h (128-bit check of every multiply-add column, K*p >= b and limb
dominance in the lazy differences, result ranges of the multipliers, ...).  Operands come from tests/limb_patterns.py:
all-ones limbs at the TOP of the range each function documents (weak-normal 2p, the K of sub_carry<K>, 64p for
reduce_wide, the madd_finite table for the two base fields).  Every bound below is taken from a comment in the headers,
none from what the code happens to return; every comparison is integer equality against Python integers or the
oracle's group law.  `lift` = 1 reruns a driver with every multiplier returning its representative in [p, 2p), the top
of its documented output range, so the range tables of the callers (madd_finite, the NTT levels) are walked at their
stated bounds and not at the ~1.03p a Montgomery product returns in practice."""
import ctypes
import os
import random
import subprocess

import pytest

from limb_patterns import adversarial, from_limbs, near_all_ones, to_limbs
from oracle import py_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "shim")
SRC = os.path.join(SHIM_DIR, "bounds_shim.cpp")
FIELD_IDS = {"bn254_fr": (0, O.BN254.r), "bn254_fp": (1, O.BN254.p), "bls12_381_fr": (2, O.BLS12_381.r),
             "bls12_381_fp": (3, O.BLS12_381.p)}
CURVES = {"bn254": (0, O.BN254, "bn254_fp"), "bls12_381": (1, O.BLS12_381, "bls12_381_fp")}
U32 = ctypes.c_uint32


class Shim:
    def __init__(self, lib):
        self.lib = lib
        lib.bs_audit_read.restype = ctypes.c_ulonglong
        self.fields = {name: FieldView(self, fid, p) for name, (fid, p) in FIELD_IDS.items()}

    def reset(self, lift=0):
        self.lib.bs_audit_reset(int(lift))

    def violations(self):
        fn, what, line = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128), ctypes.c_int(0)
        n = self.lib.bs_audit_read(fn, what, 128, ctypes.byref(line))
        return n, f"{n} violations, first in {fn.value.decode()} (field.h:{line.value}): {what.value.decode()}"

    def assert_clean(self):
        n, text = self.violations()
        assert n == 0, text


class FieldView:
    """layout and constants of one field AS THE HEADER HAS THEM (bs_info), and raw-limb calls"""

    def __init__(self, shim, fid, p_oracle):
        self.shim, self.fid = shim, fid
        geo = (ctypes.c_int * 6)()
        pl, r1 = (U32 * 16)(), (U32 * 16)()
        assert shim.lib.bs_info(fid, geo, pl, r1) == 0
        self.L, self.N, self.NW, self.BITS, self.FIT, self.CAP = list(geo)
        self.p = from_limbs(list(pl)[:self.N], self.L)
        self.R = 1 << (self.L * self.N)
        self.r1 = from_limbs(list(r1)[:self.N], self.L)
        self.p_oracle = p_oracle
        self.Rinv = pow(self.R, -1, self.p)

    def limbs(self, x):
        return to_limbs(x, self.L, self.N)

    def pack(self, elems):
        """elems: ints (normalised image) or explicit limb lists"""
        flat = []
        for e in elems:
            flat += self.limbs(e) if isinstance(e, int) else list(e)
        return (U32 * len(flat))(*flat)

    def call(self, op, elems, nout=1):
        out = (U32 * (max(nout, 1) * self.N))()
        rc = self.shim.lib.bs_field_op(self.fid, op, self.pack(elems), out)
        assert rc >= 0
        res = [list(out)[i * self.N:(i + 1) * self.N] for i in range(nout)]
        return rc, res

    def val(self, op, elems):
        """(value, limbs) of a one-element result"""
        _, res = self.call(op, elems)
        return from_limbs(res[0], self.L), res[0]

    def normalised(self, limbs):
        return all(v < (1 << self.L) for v in limbs[:-1])

    def pats(self, K, count=0, seed=0):
        return adversarial(self.p, self.L, self.N, K, count, seed)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(SHIM_DIR, "libbounds_shim.so")
    subprocess.run(["g++", "-O0", "-std=c++17", "-DKZG_AUDIT", "-shared", "-fPIC", SRC, "-o", so], check=True)
    return Shim(ctypes.CDLL(so))


# op codes of bs_field_op
MUL, SQR, MUL2, DOT1, DOT2, DOT3, DOT6, DOT16, ADD, SUB, DBL, NEG, NEG_WEAK, REDUCE, REDUCE_WIDE, CARRY, ADD_LAZY, \
    SUB_LAZY4, SUBC2, SUBC4, SUBC6, SUBC8, CNEG_SUB0, CNEG_SUB1, ADD_TWICE, CNEGC0, CNEGC1, IS_ZERO, IS_ZERO_WEAK, \
    FROM_WORDS, TO_WORDS, TO_MONT, FROM_MONT, INV, DOT4, DOT5, EQ = range(37)
DOTS = {1: DOT1, 2: DOT2, 3: DOT3, 4: DOT4, 5: DOT5, 6: DOT6, 16: DOT16}


# ---- layout, constants, the column capacity ---------------------------------------------------------------

@pytest.mark.parametrize("name", list(FIELD_IDS))
def test_constants_and_redistributed_multiples(shim, name):
    """The header's modulus is the oracle's; R1 = R mod p; FIT = 2^(64-2L) (the comment above Field::FIT), and the
    redistributed K*p of sub_carry<K> / sub_lazy4 have the value K*p with every lower limb >= 2^L - 1, so that they
    dominate a normalised limb (the sentence above sub_carry), and below 2^32 - 2^(L+1) so that adding a normalised limb
    and a carry cannot wrap."""
    f = shim.fields[name]
    assert f.p == f.p_oracle and f.r1 == f.R % f.p
    assert f.FIT == 1 << (64 - 2 * f.L) and f.CAP == f.FIT - 1
    assert 4 * f.p < f.R and 8 * f.p < f.R                       # "4p < R for all four fields", mul2's 8p < R
    for K in (2, 4, 6, 8):
        out = (U32 * f.N)()
        assert shim.lib.bs_pkr(f.fid, K, out) == 0
        limbs = list(out)
        assert from_limbs(limbs, f.L) == K * f.p, K
        assert all((1 << f.L) - 1 <= v <= (1 << 32) - (1 << (f.L + 1)) for v in limbs[:-1]), (K, [hex(v) for v in limbs])


@pytest.mark.parametrize("name", list(FIELD_IDS))
def test_a_column_holds_fit_products_and_no_more(shim, name):
    """"FIT products of two limbs <= 2^L - 1 plus the carry of the previous column still fit 64 bits" -- and FIT + 1
    do not, so the split rule has no slack to give away."""
    f = shim.fields[name]
    for n in range(1, f.FIT + 1):
        shim.reset()
        shim.lib.bs_column(f.fid, n)
        shim.assert_clean()
    shim.reset()
    shim.lib.bs_column(f.fid, f.FIT + 1)
    assert shim.violations()[0] == 1
    shim.reset()


# ---- the multipliers ---------------------------------------------------------------------------------

def check_product(f, got, limbs, want_mod_p, ctx):
    assert got % f.p == want_mod_p % f.p, ctx
    assert got < 2 * f.p, ctx                                  # weak-normal out
    assert f.normalised(limbs), ctx


@pytest.mark.parametrize("lift", [0, 1])
@pytest.mark.parametrize("name", list(FIELD_IDS))
def test_multipliers_at_the_top_of_the_weak_normal_range(shim, name, lift):
    """mul / sqr / mul2 / dot<K>: weak-normal (< 2p) in and out, limbs normalised.  All pairs of the fixed patterns
    (2p-1, all-ones limbs under the top limb of 2p-1, ...) and seeded mixtures; dot<K> for K = 1..6 (what poly.hip
    instantiates) and K = 16, the largest the static_assert admits -- 4*16*p <= R holds for all four fields, with
    6 p to spare for BLS12-381 Fr."""
    f = shim.fields[name]
    fixed = f.pats(2)
    mixed = f.pats(2, 60, seed=f.fid)[len(fixed):]
    shim.reset(lift)
    for a in fixed:
        got, l = f.val(SQR, [a])
        check_product(f, got, l, a * a * f.Rinv, ("sqr", hex(a)))
        for b in fixed:
            got, l = f.val(MUL, [a, b])
            check_product(f, got, l, a * b * f.Rinv, ("mul", hex(a), hex(b)))
    # nearly all-ones operands with varying low limbs: varying quotient digits over (nearly) full columns
    # (L = 30 is the layout whose mul / sqr split columns: about 1 pair in 100 of this family fills a column of an
    # UNSPLIT product past 64 bits, so it gets enough pairs for dozens of them)
    near = near_all_ones(f.p, f.L, f.N, 2, 6000 if f.L == 30 else 400, 300 + f.fid)
    for a, b in zip(near[::2], near[1::2]):
        got, l = f.val(MUL, [a, b])
        check_product(f, got, l, a * b * f.Rinv, ("mul", hex(a), hex(b)))
        got, l = f.val(SQR, [a])
        check_product(f, got, l, a * a * f.Rinv, ("sqr", hex(a)))
        got, l = f.val(MUL2, [a, b, b, a])
        check_product(f, got, l, 2 * a * b * f.Rinv, ("mul2", hex(a), hex(b)))
        got, l = f.val(DOT3, [a, b, a, b, a, b])
        check_product(f, got, l, 3 * a * b * f.Rinv, ("dot3", hex(a), hex(b)))
    ops = fixed[:6] + mixed + near[:40]
    rng = random.Random(100 + f.fid)
    for i in range(400):
        a, b, c, d = (rng.choice(ops) for _ in range(4)) if i >= 8 else [fixed[i % 2]] * 4
        got, l = f.val(MUL2, [a, b, c, d])
        check_product(f, got, l, (a * b + c * d) * f.Rinv, ("mul2", hex(a), hex(b), hex(c), hex(d)))
    assert 4 * 16 * f.p <= f.R
    for K, op in DOTS.items():
        for i in range(60):
            if i < 2:
                xs, ys = [fixed[i]] * K, [fixed[i]] * K          # every term (2p-1)^2; all-ones limbs under the top
            else:
                xs, ys = [rng.choice(ops) for _ in range(K)], [rng.choice(ops) for _ in range(K)]
            got, l = f.val(op, xs + ys)
            check_product(f, got, l, sum(x * y for x, y in zip(xs, ys)) * f.Rinv, ("dot", K, i))
    shim.assert_clean()


@pytest.mark.parametrize("lift", [0, 1])
@pytest.mark.parametrize("name", list(FIELD_IDS))
def test_products_of_the_lazy_ranges(shim, name, lift):
    """"mul / sqr / mul2 only need normalised limbs and a product of the operand VALUES below R*p": the operand ranges
    of ec.h's table above madd_finite -- Pp^2 (10p x 10p), Pp*PP (10p x 2p), X1*PP (8p x 2p) and the mul2 of
    4p x 10p + 2p x 2p.  The table is stated for the two BASE fields ("below R*p for both base fields").  Whether a
    field is covered follows from its R/p, read from the header: 100 p < R holds for BN254 Fp (R/p = 168), BLS12-381 Fp
    (630) and, as it happens, BN254 Fr (168); it does NOT hold for BLS12-381 Fr (R/p = 70), which the contract does not
    cover and which is therefore only driven with the 8p x 2p products its R/p allows (16 p < R)."""
    f = shim.fields[name]
    covered = 100 * f.p < f.R
    assert covered == (name != "bls12_381_fr")
    if name.endswith("_fp"):
        assert covered                                           # ec.h's claim
    shim.reset(lift)
    p10, p8, p4, p2 = f.pats(10, 20, 1), f.pats(8, 20, 2), f.pats(4, 10, 3), f.pats(2, 10, 4)
    rng = random.Random(7)
    if covered:
        for a in p10[:12] + p10[-20:]:
            got, l = f.val(SQR, [a])
            check_product(f, got, l, a * a * f.Rinv, ("sqr 10p", hex(a)))
            for b in p10[:4]:
                got, l = f.val(MUL, [a, b])
                check_product(f, got, l, a * b * f.Rinv, ("mul 10p x 10p", hex(a), hex(b)))
            for b in p2[:6]:
                got, l = f.val(MUL, [a, b])
                check_product(f, got, l, a * b * f.Rinv, ("mul 10p x 2p", hex(a), hex(b)))
        for i in range(300):
            a, b, c, d = (p4[i % 2], p10[i % 2], p2[i % 2], p2[i % 2]) if i < 2 else \
                (rng.choice(p4), rng.choice(p10), rng.choice(p2), rng.choice(p2))
            got, l = f.val(MUL2, [a, b, c, d])
            check_product(f, got, l, (a * b + c * d) * f.Rinv, ("mul2 4p x 10p + 2p x 2p", i))
    assert 16 * f.p < f.R
    for a in p8[:12] + p8[-20:]:
        for b in p2[:6]:
            got, l = f.val(MUL, [a, b])
            check_product(f, got, l, a * b * f.Rinv, ("mul 8p x 2p", hex(a), hex(b)))
        if 64 * f.p < f.R:
            got, l = f.val(SQR, [a])                             # dbl of an accumulator: X^2 with X < 8p
            check_product(f, got, l, a * a * f.Rinv, ("sqr 8p", hex(a)))
    shim.assert_clean()


# ---- additions, lazy differences, reductions -------------------------------------------------------------

@pytest.mark.parametrize("name", list(FIELD_IDS))
def test_additive_functions_at_the_top_of_their_ranges(shim, name):
    """add / sub / dbl / neg / neg_weak / reduce / is_zero / is_zero_weak / eq on weak-normal operands up to 2p - 1,
    sub_carry<K> with b up to and including K*p and a up to 10p, sub_carry_cneg<2>, add_twice_carry, cneg_canonical:
    the exact integer where the header promises one (a - b + K*p, a + 2b, 2p - a), the value mod p and the documented
    range elsewhere, and normalised lower limbs throughout."""
    f = shim.fields[name]
    p = f.p
    w = f.pats(2, 25, 11)                                        # weak-normal operands
    shim.reset()
    for a in w:
        for b in w[:14] + w[-8:]:
            got, l = f.val(ADD, [a, b])                          # "a + b, weak-normal in and out"
            assert got in (a + b, a + b - 2 * p) and got < 2 * p and f.normalised(l), ("add", hex(a), hex(b))
            got, l = f.val(SUB, [a, b])
            assert got in (a - b, a - b + 2 * p) and 0 <= got < 2 * p and f.normalised(l), ("sub", hex(a), hex(b))
            got, l = f.val(ADD_TWICE, [a, b])                    # "value a + 2b, limbs normalised"
            assert got == a + 2 * b and f.normalised(l)
            for op, neg in ((CNEG_SUB0, False), (CNEG_SUB1, True)):     # (neg ? 2p - a : a) - b + 2p
                got, l = f.val(op, [a, b])
                assert got == (2 * p - a if neg else a) - b + 2 * p and f.normalised(l), ("sub_carry_cneg", neg, hex(a), hex(b))
            rc, _ = f.call(EQ, [a, b])
            assert rc == int((a - b) % p == 0)
        got, l = f.val(DBL, [a])
        assert got in (2 * a, 2 * a - 2 * p) and got < 2 * p and f.normalised(l)
        got, l = f.val(NEG, [a])
        assert got % p == (-a) % p and got < 2 * p and f.normalised(l)
        got, l = f.val(NEG_WEAK, [a])                            # "2p - a ... normalised limbs, value in (0, 2p]"
        assert got == 2 * p - a and f.normalised(l)
        got, l = f.val(REDUCE, [a])                              # [0, 2p) -> [0, p)
        assert got == a % p and f.normalised(l)
        for op in (IS_ZERO, IS_ZERO_WEAK):
            rc, _ = f.call(op, [a])
            assert rc == int(a in (0, p)), (op, hex(a))
    # sub_carry_cneg with b = 2p exactly ("b <= K*p") and a at both ends
    for a in (0, 2 * p - 1, w[1]):
        for op, neg in ((CNEG_SUB0, False), (CNEG_SUB1, True)):
            got, l = f.val(op, [a, 2 * p])
            assert got == (2 * p - a if neg else a) and f.normalised(l)
    shim.assert_clean()
    # sub_carry<K>: "a - b + K*p for normalised a, b with b <= K*p"; a up to 8p (the X of an accumulator), 10p
    for K, op in ((2, SUBC2), (4, SUBC4), (6, SUBC6), (8, SUBC8)):
        bs = f.pats(K, 25, 20 + K) + [K * p]
        for a in f.pats(2)[:10] + f.pats(8)[:6] + f.pats(10)[:3]:
            for b in bs:
                got, l = f.val(op, [a, b])
                assert got == a - b + K * p and f.normalised(l), (K, hex(a), hex(b))
    shim.assert_clean()
    # add_twice_carry with a wide a (nothing in its comment confines a to 2p)
    for a in f.pats(8)[:8]:
        for b in f.pats(2)[:8]:
            got, l = f.val(ADD_TWICE, [a, b])
            assert got == a + 2 * b and f.normalised(l)
    # cneg_canonical: canonical in, [0, p] out
    for a in f.pats(1, 25, 31):
        got, l = f.val(CNEGC1, [a])
        assert got == p - a and f.normalised(l)
        got, l = f.val(CNEGC0, [a])
        assert got == a
    shim.assert_clean()


@pytest.mark.parametrize("name", list(FIELD_IDS))
def test_lazy_limbwise_forms_and_carry(shim, name):
    """add_lazy ("caller keeps limbs below 2^32"), sub_lazy4 ("a - b + 4p limb-wise, for a normalised b < 2p ... no limb
    goes negative"), carry ("limbs back below 2^L, value unchanged")."""
    f = shim.fields[name]
    p, L, N = f.p, f.L, f.N
    shim.reset()
    wide = f.pats(64, 20, 41)
    for a in wide[:10] + wide[-20:]:
        for b in f.pats(2, 10, 42):
            _, res = f.call(ADD_LAZY, [a, b])
            assert res[0] == [x + y for x, y in zip(f.limbs(a), f.limbs(b))]
            _, res2 = f.call(SUB_LAZY4, [a, b])
            assert from_limbs(res2[0], L) == a - b + 4 * p, (hex(a), hex(b))
            got, l = f.val(CARRY, [res2[0]])
            assert got == a - b + 4 * p and f.normalised(l)
            got, l = f.val(CARRY, [res[0]])
            assert got == a + b and f.normalised(l)
    # carry on limbs far above 2^L: the largest that leave room for the incoming carry (below 2^(32-L))
    big = [(1 << 32) - (1 << (32 - L))] * (N - 1) + [5]
    got, l = f.val(CARRY, [big])
    assert got == from_limbs(big, L) and f.normalised(l)
    shim.assert_clean()


@pytest.mark.parametrize("name", list(FIELD_IDS))
def test_reduce_wide_over_its_whole_range(shim, name):
    """"[0, 2^(L*N)) with normalised limbs -> [0, p)": every multiple of p up to 64p (what ntt.hip says it accepts) with
    its two neighbours -- K*p - 1 is where a quotient estimate that is one too large goes negative --, the adversarial
    patterns at 64p, and the top of the stated range: all limbs all-ones (R - 1)."""
    f = shim.fields[name]
    p = f.p
    assert 64 * p < f.R                                          # ntt.hip: "the 64p that reduce_wide accepts"
    vals = []
    for k in range(0, 65):
        vals += [k * p - 1, k * p, k * p + 1]
    vals = [v for v in vals if 0 <= v < 64 * p] + f.pats(64, 200, 51)
    for k in (3, 17, 49, 50, 53, 63):
        vals += f.pats(k)[:6]
    vals += [f.R - 1, f.R - 2, ((f.R - 1) // p) * p - 1, ((f.R - 1) // p) * p]
    shim.reset()
    for v in vals:
        got, l = f.val(REDUCE_WIDE, [v])
        assert got == v % p and f.normalised(l), hex(v)
    shim.assert_clean()


@pytest.mark.parametrize("name", list(FIELD_IDS))
def test_words_montgomery_form_and_inverse(shim, name):
    """from_words / to_words (limb image <-> saturated words, bit for bit), to_mont / from_mont, inv (a^(p-2), inv(0) = 0)
    on canonical and weak-normal operands with adversarial limbs."""
    f = shim.fields[name]
    p = f.p
    shim.reset()
    for a in f.pats(1, 30, 61):
        words = [(a >> (32 * i)) & 0xffffffff for i in range(f.NW)] + [0] * (f.N - f.NW)
        out = (U32 * f.N)()
        assert shim.lib.bs_field_op(f.fid, FROM_WORDS, (U32 * f.N)(*words), out) == 0
        assert list(out) == f.limbs(a)
        out = (U32 * f.N)()
        assert shim.lib.bs_field_op(f.fid, TO_WORDS, f.pack([a]), out) == 0
        assert list(out)[:f.NW] == words[:f.NW]
        got, l = f.val(FROM_MONT, [a])
        assert got == a * f.Rinv % p
    for a in f.pats(2, 30, 62):
        got, l = f.val(TO_MONT, [a])
        check_product(f, got, l, a * f.R, ("to_mont", hex(a)))
        got, l = f.val(FROM_MONT, [a])
        assert got == a * f.Rinv % p and f.normalised(l)        # canonical
    # any 32*NW-bit word image goes through from_words unchanged ("taken as is")
    allw = (1 << (32 * f.NW)) - 1
    out = (U32 * f.N)()
    shim.lib.bs_field_op(f.fid, FROM_WORDS, (U32 * f.N)(*([0xffffffff] * f.NW + [0] * (f.N - f.NW))), out)
    assert from_limbs(list(out), f.L) == allw
    for a in f.pats(2)[:8] + f.pats(2, 6, 63)[-6:]:
        got, l = f.val(INV, [a])                                 # Montgomery in and out; inv(0) = 0
        plain = a * f.Rinv % p
        check_product(f, got, l, (pow(plain, -1, p) * f.R) if plain else 0, ("inv", hex(a)))
    shim.assert_clean()


# ---- the audit notices what it is there to notice (positive controls) -------------------------------------

def test_the_audit_flags_broken_preconditions(shim):
    """Each hook fires on an operand just outside its function's stated precondition -- a check that cannot fail would
    make the zero-violation assertions of every other test here worthless."""
    f = shim.fields["bls12_381_fp"]
    p = f.p
    cases = [(SUBC4, [1, 4 * p + 1]),                            # b above K*p
             (SUBC8, [1, 8 * p + 1]),
             (REDUCE, [2 * p]),
             (IS_ZERO_WEAK, [2 * p]),
             (CNEGC1, [p]),
             (TO_WORDS, [p]),
             (REDUCE_WIDE, [[1 << f.L] + [0] * (f.N - 1)]),       # a limb that is not normalised
             (SUB_LAZY4, [0, [(1 << 31) + 5] + [0] * (f.N - 1)]),   # the subtrahend's limb above that of 4p
             (ADD_LAZY, [[1 << 31] * f.N, [1 << 31] * f.N]),
             (MUL, [[(1 << 32) - 1] * f.N, [(1 << 32) - 1] * f.N])]     # columns overflow, result far above 2p
    for op, elems in cases:
        shim.reset()
        f.call(op, elems)
        assert shim.violations()[0] >= 1, op
    shim.reset()


# ---- ec.h -----------------------------------------------------------------------------------------

class CurveView:
    def __init__(self, shim, name):
        self.cid, self.cv, fname = CURVES[name]
        self.shim = shim
        self.f = shim.fields[fname]
        self.p, self.b = self.cv.p, self.cv.b
        assert self.p % 4 == 3                                   # y = v^((p+1)/4)

    def lift_x(self, x):
        """(x, y) on the curve or None"""
        v = (x * x * x + self.b) % self.p
        y = pow(v, (self.p + 1) // 4, self.p)
        return (x, y) if y * y % self.p == v else None

    def affine_points(self, count, seed):
        """affine points whose Montgomery-form x has adversarial limbs: x~ from the generator (canonical, as table
        coordinates are), x = x~ / R; kept if x^3 + b is a square.  Returns [(plain (x, y), x~, y~)]"""
        f, out = self.f, []
        for xm in f.pats(1, 4 * count + 40, seed):
            pt = self.lift_x(xm * f.Rinv % self.p)
            if pt is not None and pt[1] != 0:
                out.append((pt, xm, pt[1] * f.R % self.p))
            if len(out) == count:
                break
        assert len(out) == count
        return out

    def accumulators(self, count, seed, KX):
        """XYZZ accumulators on the curve with X~ (below KX*p) and ZZ~ (weak-normal) of adversarial limbs and Y~, ZZZ~ in
        [p, 2p): (x lambda^2, y lambda^3, lambda^2, lambda^3) where a lambda exists.  Returns [(plain (x, y), limbs)]"""
        f, p, out = self.f, self.p, []
        xs, zs = f.pats(KX, 30, seed), f.pats(2, 30, seed + 1)
        rng = random.Random(seed)
        tries = 0
        while len(out) < count:
            tries += 1
            assert tries < 400 * count
            Xm, ZZm = (xs[tries % len(xs)], rng.choice(zs)) if tries % 2 else (rng.choice(xs), zs[tries % len(zs)])
            ZZ = ZZm * f.Rinv % p
            if ZZ == 0:
                continue
            lam = pow(ZZ, (p + 1) // 4, p)
            if lam * lam % p != ZZ:
                continue
            x = Xm * f.Rinv * pow(ZZ, -1, p) % p
            pt = self.lift_x(x)
            if pt is None or pt[1] == 0:
                continue
            if rng.randrange(2):
                pt = (pt[0], p - pt[1])
            lam3 = lam * ZZ % p
            Ym = pt[1] * lam3 * f.R % p + p                      # the representative in [p, 2p)
            ZZZm = lam3 * f.R % p + p
            out.append((pt, [Xm, Ym, ZZm, ZZZm]))
        return out

    def call(self, op, acc=None, aff=None, acc2=None, nout=4):
        f = self.f
        elems = list(acc or [0, 0, 0, 0]) + list(aff or [0, 0]) + list(acc2 or [0, 0, 0, 0])
        out = (U32 * (4 * f.N))()
        rc = self.shim.lib.bs_ec_op(self.cid, op, f.pack(elems), out)
        assert rc >= 0
        vals = [list(out)[i * f.N:(i + 1) * f.N] for i in range(nout)]
        return rc, vals

    def decode(self, limbs4, x_bound):
        """XYZZ raw limbs -> plain affine point or None; asserts the documented ranges and ZZ^3 = ZZZ^2"""
        f, p = self.f, self.p
        X, Y, ZZ, ZZZ = (from_limbs(l, f.L) for l in limbs4)
        assert all(f.normalised(l) for l in limbs4)
        assert X < x_bound * p and Y < 2 * p and ZZ < 2 * p and ZZZ < 2 * p
        zz, zzz = ZZ * f.Rinv % p, ZZZ * f.Rinv % p
        if zz == 0:
            return None
        assert pow(zz, 3, p) == zzz * zzz % p
        return (X * f.Rinv * pow(zz, -1, p) % p, Y * f.Rinv * pow(zzz, -1, p) % p)


def oadd(a, b, cv):
    """affine (or None) + affine (or None) by the oracle's group law"""
    pa = O.Z1() if a is None else O.from_affine(a)
    pb = O.Z1() if b is None else O.from_affine(b)
    return O.normalize(O.add(pa, pb, cv), cv)


def oneg(a, cv):
    return None if a is None else (a[0], (-a[1]) % cv.p)


MADD, MADD_FIN, MADD_FIN_NEG, EC_ADD, EC_DBL, EC_DBL_AFFINE, TO_AFFINE, ON_CURVE = range(8)


@pytest.mark.parametrize("lift", [0, 1])
@pytest.mark.parametrize("curve", list(CURVES))
def test_every_ec_formula_with_adversarial_operands(shim, curve, lift):
    """madd, madd_finite (both signs), add, dbl, dbl_affine, to_affine, on_curve against the oracle's group law, on
    affine operands whose Montgomery x has adversarial limbs and on re-scaled accumulators at the top of the ranges of
    the table above madd_finite (X1 < 8p; Y1, ZZ1, ZZZ1 < 2p), incl. P + P, P - P and y-mirrored operands.  The points
    lie on the curve but (BLS12-381) not in the r-torsion; the group law does not care."""
    c = CurveView(shim, curve)
    cv, f, p = c.cv, c.f, c.p
    affs = c.affine_points(24, 70)
    acc8 = c.accumulators(30, 71, 8)
    acc2 = c.accumulators(16, 73, 2)
    shim.reset(lift)
    for pt, xm, ym in affs:
        assert O.is_on_curve(pt, cv)
        rc, _ = c.call(ON_CURVE, aff=[xm, ym])
        assert rc == 1
        rc, _ = c.call(ON_CURVE, aff=[xm, (ym + 1) % p])
        assert rc == 0
        _, out = c.call(EC_DBL_AFFINE, aff=[xm, ym])
        assert c.decode(out, 2) == oadd(pt, pt, cv)
    for i, (a, A) in enumerate(acc8):
        assert O.is_on_curve(a, cv)
        # the consumers of a lazily reduced accumulator: X < 8p only as a mul / sqr operand
        _, out = c.call(EC_DBL, acc=A)
        assert c.decode(out, 2) == oadd(a, a, cv)
        rc, out = c.call(TO_AFFINE, acc=A, nout=2)
        assert rc == 0 and tuple(from_limbs(l, f.L) * f.Rinv % p for l in out) == a
        b2, B2 = acc2[i % len(acc2)]
        _, out = c.call(EC_ADD, acc=A, acc2=B2)
        assert c.decode(out, 2) == oadd(a, b2, cv)
        _, out = c.call(EC_ADD, acc=A, acc2=A)                   # falls through to dbl
        assert c.decode(out, 2) == oadd(a, a, cv)
        for j, (b, xm, ym) in enumerate(affs):
            for op, bb in ((MADD_FIN, b), (MADD_FIN_NEG, oneg(b, cv))):
                fin, out = c.call(op, acc=A, aff=[xm, ym])
                want = oadd(a, bb, cv)
                assert fin == int(want is not None)
                if fin:
                    assert c.decode(out, 8) == want, (i, j, op)
        # the affine operand equal to the accumulator's point: doubling (same sign), infinity (opposite sign)
        xm, ym = a[0] * f.R % p, a[1] * f.R % p
        fin, out = c.call(MADD_FIN, acc=A, aff=[xm, ym])
        assert fin == 1 and c.decode(out, 8) == oadd(a, a, cv)
        fin, out = c.call(MADD_FIN_NEG, acc=A, aff=[xm, ym])
        assert fin == 0
        fin, out = c.call(MADD_FIN, acc=A, aff=[xm, (p - ym) % p])
        assert fin == 0
        fin, out = c.call(MADD_FIN_NEG, acc=A, aff=[xm, (p - ym) % p])
        assert fin == 1 and c.decode(out, 8) == oadd(a, a, cv)
    for i, (a, A) in enumerate(acc2):                                 # madd / add take a weak-normal accumulator
        for b, xm, ym in affs[:8]:
            _, out = c.call(MADD, acc=A, aff=[xm, ym])
            assert c.decode(out, 2) == oadd(a, b, cv)
        xm, ym = a[0] * f.R % p, a[1] * f.R % p
        _, out = c.call(MADD, acc=A, aff=[xm, ym])
        assert c.decode(out, 2) == oadd(a, a, cv)
        _, out = c.call(MADD, acc=A, aff=[xm, (p - ym) % p])
        assert c.decode(out, 2) is None
        _, out = c.call(MADD, acc=[0, 0, 0, 0], aff=[xm, ym])       # O + P
        assert c.decode(out, 2) == a
        _, out = c.call(EC_ADD, acc=[0, 0, 0, 0], acc2=A)
        assert c.decode(out, 2) == a
        _, out = c.call(EC_ADD, acc=A, acc2=[0, 0, 0, 0])
        assert c.decode(out, 2) == a
    _, out = c.call(EC_DBL, acc=[0, 0, 0, 0])
    assert c.decode(out, 2) is None
    rc, _ = c.call(TO_AFFINE, acc=[0, 0, 0, 0], nout=2)
    assert rc == 1
    shim.assert_clean()


@pytest.mark.parametrize("lift", [0, 1])
@pytest.mark.parametrize("curve", list(CURVES))
def test_long_flag_tracked_chains(shim, curve, lift):
    """Thousands of steps of the MSM's inner loop (flag-tracked madd_finite) over a pool that repeats: P + P runs into
    dbl_affine, P - P into infinity and the copy-in path, both signs throughout; then add, dbl, to_affine as the MSM's
    consumers do.  X of the accumulator stays below 8p at EVERY step (bs_ec_chain returns -2 otherwise, and the next
    step's sub_carry<8> precondition is audited).  Expected value: sum of the signed counts times the points, with
    INTEGER scalars (the points are outside the r-torsion on BLS12-381)."""
    c = CurveView(shim, curve)
    cv, f, p = c.cv, c.f, c.p
    pool = c.affine_points(6, 80)
    for k in (1, 2, 3):                                          # and the generator with two multiples
        pt = O.normalize(O.multiply(O.from_affine(cv.g1), k, cv), cv)
        pool.append((pt, pt[0] * f.R % p, pt[1] * f.R % p))
    pool.append((oneg(pool[0][0], cv), pool[0][1], p - pool[0][2]))      # the mirror of pool[0] as an entry of its own
    flat = []
    for _, xm, ym in pool:
        flat += [xm, ym]
    steps = 3000
    rng = random.Random(81 + c.cid)
    idx, negs = [], []
    while len(idx) < steps:
        i, s = rng.randrange(len(pool)), rng.randrange(2)
        if rng.randrange(20):
            idx.append(i)
            negs.append(s)
        elif len(idx) % 2 == 0:                                 # +P -P (infinity), +P (copy-in), +P (doubling)
            idx += [i, i, i, i]
            negs += [s, 1 - s, s, s]
        else:                                                   # undo the last 50 steps in reverse: passes through P - P
            idx += idx[::-1][:50]
            negs += [1 - v for v in negs[::-1][:50]]
    idx, negs = idx[:steps], negs[:steps]
    out = (U32 * (2 * f.N))()
    shim.reset(lift)
    rc = shim.lib.bs_ec_chain(c.cid, f.pack(flat), len(pool), (ctypes.c_uint8 * steps)(*idx),
                              (ctypes.c_uint8 * steps)(*negs), steps, out)
    assert rc in (0, 1), rc
    shim.assert_clean()
    counts = [0] * len(pool)
    for i, s in zip(idx, negs):
        counts[i] += -1 if s else 1
    acc = O.Z1()
    for (pt, _, _), k in zip(pool, counts):
        q = O.multiply(O.from_affine(pt if k >= 0 else oneg(pt, cv)), abs(k), cv)
        acc = O.add(acc, q, cv)
    want = O.normalize(O.double(O.add(acc, O.from_affine(pool[0][0]), cv), cv), cv)
    got = None if rc == 1 else (from_limbs(list(out)[:f.N], f.L), from_limbs(list(out)[f.N:], f.L))
    assert got == want


# ---- the NTT's lazy arithmetic (ntt.hip), restated in the shim ------------------------------------------

def ntt_model(x, kind, c, r):
    """one fused step mod r on positions 0..3, as bs_ntt_run leaves them; c: the three effective twiddles (tw~ / R)"""
    if kind == 2:
        return [(x[0] + x[1]) % r, (x[0] - x[1]) % r, (x[2] + x[3]) % r, (x[2] - x[3]) % r]
    if kind == 0:
        t1, t3, c1, c2 = x[1], x[3], 1, c[0]
    else:
        t1, t3, c1, c2 = x[1] * c[0] % r, x[3] * c[0] % r, c[1], c[2]
    b0, b1 = x[0] + t1, x[0] - t1
    u2, u3 = (x[2] + t3) * c1 % r, (x[2] - t3) * c2 % r
    return [(b0 + u2) % r, (b1 + u3) % r, (b0 - u2) % r, (b1 - u3) % r]


def ntt_run(shim, f, x, kinds, tws, epi, fac, shift=0):
    n = len(kinds)
    after, fin = (U32 * (max(n, 1) * 4 * f.N))(), (U32 * (4 * f.N))()
    rc = shim.lib.bs_ntt_run(f.fid, f.pack(x), (ctypes.c_int * max(n, 1))(*kinds), f.pack(tws or [0, 0, 0]), n, shift, epi,
                             f.pack(fac), after, fin)
    assert rc == 0
    a = list(after)
    steps = [[a[(s * 4 + i) * f.N:(s * 4 + i + 1) * f.N] for i in range(4)] for s in range(n)]
    fl = list(fin)
    return steps, [fl[i * f.N:(i + 1) * f.N] for i in range(4)]


def check_epilogue(f, epi, fin, x_vals, fac):
    r = f.p
    for l, v in zip(fin, x_vals):
        got = from_limbs(l, f.L)
        assert f.normalised(l)
        if epi == 0:
            assert got == v % r                                   # reduce_wide: canonical
        elif epi == 1:
            assert got % r == v * fac[0] * fac[1] * f.Rinv * f.Rinv % r and got < 2 * r
        elif epi == 2:
            assert got % r == v * fac[0] * f.Rinv % r and got < 2 * r
        else:
            assert got == v * fac[0] * f.Rinv % r


@pytest.mark.parametrize("lift", [0, 1])
@pytest.mark.parametrize("name", ["bn254_fr", "bls12_381_fr"])
def test_ntt_lazy_levels_grow_as_the_header_says(shim, name, lift):
    """ntt.hip: "values grow by at most 4p per level (<= 49p after 12 levels ...)", "2p + 4p per level stays below the
    64p that reduce_wide accepts".  Six fused steps (first_step + five radix4_step, or the radix-2 level + five) with the
    outputs fed back, from canonical inputs (pass 1) and from weak-normal ones (what EPI_FACTOR / EPI_TABLE leave for
    pass 2); twiddles are canonical Montgomery images of adversarial limbs ("the lazy butterflies rely on twiddles < p").
    After every step: the values mod r, the integer bound (start + 4 * levels) * p, normalised limbs (incl. the top
    limb, which reduce_wide reads); then every epilogue."""
    f = shim.fields[name]
    r = f.p
    canon, weak = f.pats(1, 40, 90), f.pats(2, 40, 91)
    rng = random.Random(92 + f.fid)
    shim.reset(lift)
    for trial in range(400):
        src, start = (canon, 1) if trial % 2 == 0 else (weak, 2)
        x = [src[(trial // 2 + i) % 4] for i in range(4)] if trial < 16 else [rng.choice(src) for _ in range(4)]
        kinds = [0 if trial % 4 < 2 else 2] + [1] * 5
        tws = [canon[(trial + i) % 6] if trial < 12 else rng.choice(canon) for i in range(18)]
        fac = [rng.choice(canon), rng.choice(canon)]
        epi = (trial // 4) % 4
        steps, fin = ntt_run(shim, f, x, kinds, tws, epi, fac)
        cur, levels = [v % r for v in x], 0
        for s, kind in enumerate(kinds):
            cur = ntt_model(cur, kind, [t * f.Rinv % r for t in tws[3 * s:3 * s + 3]], r)
            levels += 1 if kind == 2 else 2
            got = [from_limbs(l, f.L) for l in steps[s]]
            assert [g % r for g in got] == cur, (trial, s)
            assert all(g < (start + 4 * levels) * r for g in got), (trial, s)
            assert all(f.normalised(l) and l[-1] < (1 << f.L) for l in steps[s])
        assert levels in (11, 12) and (start + 4 * levels) <= 50
        check_epilogue(f, epi, fin, [from_limbs(l, f.L) for l in steps[-1]], fac)
    shim.assert_clean()


@pytest.mark.parametrize("lift", [0, 1])
@pytest.mark.parametrize("name", ["bn254_fr", "bls12_381_fr"])
def test_ntt_last_step_and_epilogues_at_the_header_bound(shim, name, lift):
    """Synthetic inputs at the header's bound: below 41p before the last fused step of a 12-level pass from canonical
    inputs (49p - 8p), below 42p for pass 2; the outputs stay below 49p / 50p.  The epilogues alone take 49p and 50p,
    reduce_wide also the 64p it "accepts", the multiplying ones "any operand below R = 2^261"."""
    f = shim.fields[name]
    r = f.p
    canon = f.pats(1, 30, 95)
    rng = random.Random(96 + f.fid)
    shim.reset(lift)
    for bound in (41, 42):
        src = f.pats(bound, 60, 97 + bound)
        for trial in range(80):
            x = [src[(trial + i) % 5] for i in range(4)] if trial < 10 else [rng.choice(src) for _ in range(4)]
            tws = [rng.choice(canon[:8]) if trial % 2 else rng.choice(canon) for _ in range(3)]
            fac = [rng.choice(canon), rng.choice(canon)]
            steps, fin = ntt_run(shim, f, x, [1], tws, trial % 4, fac)
            want = ntt_model([v % r for v in x], 1, [t * f.Rinv % r for t in tws], r)
            got = [from_limbs(l, f.L) for l in steps[0]]
            assert [g % r for g in got] == want
            assert all(g < (bound + 8) * r for g in got) and all(f.normalised(l) for l in steps[0])
            check_epilogue(f, trial % 4, fin, got, fac)
    kr = (f.R - 1) // r + 1                                      # K*p - 1 >= R - 1: the patterns are cut at R below
    for epi, K in ((0, 49), (0, 50), (0, 64), (1, 50), (2, 50), (3, 50), (1, kr), (2, kr), (3, kr)):
        src = [v for v in f.pats(K, 24, 99 + K) if v < f.R]
        if K == kr:
            src += [f.R - 1, f.R - 2]
        for i in range(0, len(src) - 3, 4):
            x = src[i:i + 4]
            fac = [canon[i % len(canon)], canon[(i + 1) % len(canon)]]
            _, fin = ntt_run(shim, f, x, [], None, epi, fac)
            check_epilogue(f, epi, fin, x, fac)
    shim.assert_clean()


@pytest.mark.parametrize("name", ["bn254_fr", "bls12_381_fr"])
def test_the_audit_flags_wider_limbs_in_the_butterfly(shim, name):
    """ntt.hip hands un-carried operands (limbs below 3 * 2^29) to the plain mul<1>: 9*3 + 9 product units of the 64 that
    fit.  The same step with limbs of 2^(L+3) (9*8 + 9 = 81 units) must be flagged -- the audit's precondition for a
    multiplier is the column check itself, not "limbs < 2^L"."""
    f = shim.fields[name]
    x = f.pats(41)[:4]
    shift_top = f.L * (f.N - 1)
    tw = (((f.p - 1) >> shift_top) - 1) << shift_top | ((1 << shift_top) - 1)     # all-ones limbs under the top limb of p - 1
    assert tw < f.p
    tws = [tw] * 3
    shim.reset()
    ntt_run(shim, f, x, [1], tws, 0, [1, 1])
    shim.assert_clean()
    ntt_run(shim, f, x, [1], tws, 0, [1, 1], shift=3)
    n, text = shim.violations()
    assert n >= 1 and "mad_wide" in text, text
    shim.reset()


@pytest.mark.parametrize("lift", [0, 1])
@pytest.mark.parametrize("name", ["bn254_fr", "bls12_381_fr"])
def test_the_lazy_sites_of_poly_hip(shim, name, lift):
    """poly.hip: (a) lane8_sum_reduced / the chunk sums of tile_combine_kernel -- "8 weak-normal values -> their
    canonical sum (8 * 2p < 2^261, limbs < 2^32)": eight limb-wise 32-bit additions, carry, reduce_wide; (b) dot_upto:
    up to six canonical coefficients against weak-normal Montgomery powers, one reduction."""
    f = shim.fields[name]
    r = f.p
    weak, canon = f.pats(2, 40, 110), f.pats(1, 40, 111)
    rng = random.Random(112)
    shim.reset(lift)
    for trial in range(150):
        vs = [weak[trial % 2]] * 8 if trial < 2 else [rng.choice(weak) for _ in range(8)]
        out = (U32 * f.N)()
        assert shim.lib.bs_poly_site(f.fid, 0, 0, f.pack(vs), out) == 0
        assert from_limbs(list(out), f.L) == sum(vs) % r
        cnt = trial % 6 + 1
        cs = [canon[trial % 2]] * cnt if trial < 12 else [rng.choice(canon) for _ in range(cnt)]
        xs = [weak[trial % 2]] * cnt if trial < 12 else [rng.choice(weak) for _ in range(cnt)]
        out = (U32 * f.N)()
        assert shim.lib.bs_poly_site(f.fid, 1, cnt, f.pack(cs + xs), out) == 0
        check_product(f, from_limbs(list(out), f.L), list(out), sum(a * b for a, b in zip(cs, xs)) * f.Rinv, ("dot_upto", cnt))
    shim.assert_clean()


# ---- the same drivers as a standalone program under the sanitizers -----------------------------------------

def test_drivers_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """bounds_shim.cpp with its own main(): every Field function, the restated NTT and poly sites and a 600-step
    flag-tracked chain on both curves, built with -fsanitize=address,undefined (no recovery, static runtimes) and run as
    a program of its own.  The exit status is the verdict: 0 = no sanitizer report and no audit violation."""
    exe = str(tmp_path / "bounds_shim_san")
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-DKZG_AUDIT", "-DBOUNDS_SHIM_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert "no violations" in res.stdout

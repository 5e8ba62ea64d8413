"""Where field.h cuts the 64-bit columns of its Montgomery multipliers, checked on the CPU.

plan_columns() (csrc/field.h) decides at compile time before which group of products a column's multiply-add chain is
cut; a cut sets the chain's high 32-bit word aside (2^32 is a multiple of 2^L) and the word joins the outgoing carry as
hi * 2^(32-L).  For a field that declares TOP_LIMB_BOUND (BLS12-381 Fp: 2^26) the plan works with magnitudes -- the real
limbs of p against quotient digits below 2^L, operand limbs below 2^L with a top limb below the bound -- and not with a
count of products.

tests/shim/columns_shim.cpp prints the schedules the header chose.  Here every chain of every column is recomputed in
Python integers from the modulus (the oracle's) and the layout alone, following the printed schedule: no chain may reach
2^64, no carry 2^40, every cut must be needed (greedy placement), and BLS12-381 Fp needs 3 / 3 / at most 14 cuts for
mul / sqr / mul2.  Then the audited build (tests/shim/bounds_shim.cpp, -DKZG_AUDIT: a 128-bit check of every
multiply-add, the operand preconditions, the result range) runs the multipliers and the group law of ec.h on the
largest legal operands -- all lower limbs 2^30 - 1 under the largest top limb the ranges of ec.h allow -- and, as a
positive control, on operands whose top limb is AT the declared bound."""
import ctypes
import json
import os
import random
import subprocess

import pytest

import test_field_bounds_host as B
from limb_patterns import from_limbs, to_limbs
from oracle import py_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "shim")
MODULI = {"bn254_fr": O.BN254.r, "bn254_fp": O.BN254.p, "bls12_381_fr": O.BLS12_381.r, "bls12_381_fp": O.BLS12_381.p}
# the one field that declares a top-limb bound for the operands of its multipliers (curve_constants.h): BLS12-381 Fp,
# 2^26 -- any normalised value up to 39p has a top limb below it, and ec.h passes nothing above 10p
TOP_LIMB_BOUND = {"bls12_381_fp": 1 << 26}
LIMIT = 1 << 64
CARRY_LIMIT = 1 << 40
PRECONDITION = "operand limbs above the column bound"


@pytest.fixture(scope="module")
def schedules(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("columns") / "columns_shim")
    subprocess.run(["g++", "-O0", "-std=c++17", os.path.join(SHIM_DIR, "columns_shim.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {f["field"]: f for f in json.loads(out)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("columns_audit") / "libbounds_shim.so")
    subprocess.run(["g++", "-O0", "-std=c++17", "-DKZG_AUDIT", "-shared", "-fPIC", B.SRC, "-o", so], check=True)
    return B.Shim(ctypes.CDLL(so))


def walk(p, L, N, top_bound, plan, real_p, drop=None):
    """The worst case of every chain of one multiplier, following the printed schedule plan["cut"][k][g].
    Operand limbs 0..N-2 <= 2^L - 1, top limb <= top_bound - 1 (2^L - 1 if none is declared), quotient digits
    m_i <= 2^L - 1 against the limbs of p (real_p) or against 2^L - 1 (the count rule's assumption).  At a cut the
    chain keeps its low word, and the low word of the LARGEST value is not the largest low word (2^63 + 5 leaves 5,
    2^63 - 1 leaves 2^32 - 1): what stays in the chain is bounded by 2^32 - 1 whatever the value was, what is set aside
    by the high word of the largest value.  `drop` = (k, g) leaves that one cut out.
    Returns (largest chain value, largest carry, chain value at (k, g) of `drop`)."""
    one = (1 << L) - 1
    top = (top_bound - 1) if top_bound else one
    limb = [one] * (N - 1) + [top]
    pl = to_limbs(p, L, N) if real_p else [one] * N
    terms, square = plan["terms"], plan["square"]
    worst = worst_carry = at_drop = 0
    carry = 0
    for k in range(2 * N - 1):
        lo, hi = (0, k) if k < N else (k - N + 1, N - 1)
        chain, aside = carry, 0
        for g in range(terms + 1):
            if g < terms:
                if square:
                    group = sum((2 if i < k - i else 1) * limb[i] * limb[k - i] for i in range(lo, hi + 1) if i <= k - i)
                else:
                    group = sum(limb[i] * limb[k - i] for i in range(lo, hi + 1))
            else:
                group = sum(one * pl[k - i] for i in range(lo, hi + 1) if i < k or k >= N)
                if k < N:
                    group += one * pl[0]                       # m_k p_0
            if plan["cut"][k][g] and (k, g) != drop:
                aside += chain >> 32
                chain = (1 << 32) - 1
            chain += group
            worst = max(worst, chain)
            if (k, g) == drop:
                at_drop = chain
        carry = (chain >> L) + (aside << (32 - L))
        worst_carry = max(worst_carry, carry)
    return worst, worst_carry, at_drop


@pytest.mark.parametrize("name", list(MODULI))
def test_no_chain_reaches_2_64_and_every_cut_is_needed(schedules, name):
    f = schedules[name]
    L, N, p = f["L"], f["N"], MODULI[name]
    assert from_limbs(f["p"], L) == p
    assert f["top_limb_bound"] == TOP_LIMB_BOUND.get(name, 0)
    bound = TOP_LIMB_BOUND.get(name)
    for plan in f["plans"]:
        ctx = (name, plan["name"])
        assert plan["fits"] == 1, ctx
        assert sum(map(sum, plan["cut"])) == plan["cuts"], ctx
        # a field without a declared bound is planned by the count rule: every limb of the operands AND of p at 2^L - 1
        worst, carry, _ = walk(p, L, N, bound, plan, real_p=bound is not None)
        print(ctx, "cuts", plan["cuts"], "largest chain 2^64 -", LIMIT - worst, "largest carry", hex(carry))
        assert worst < LIMIT, ctx
        assert carry < CARRY_LIMIT, ctx
        assert carry == plan["carry_max"], ctx                  # the header's own bound is this one
        # ... and with the real modulus in any case
        worst, carry, _ = walk(p, L, N, bound, plan, real_p=True)
        assert worst < LIMIT and carry < CARRY_LIMIT, ctx
        # greedy: without any one of its cuts the chain could pass 2^64 at the group that follows
        for k, row in enumerate(plan["cut"]):
            for g, c in enumerate(row):
                if c:
                    assert g >= 1, ctx                          # the carry and the first group always fit
                    _, _, at = walk(p, L, N, bound, plan, real_p=bound is not None, drop=(k, g))
                    assert at >= LIMIT, (ctx, k, g)


def test_cut_counts(schedules):
    """BLS12-381 Fp: 3 cuts in mul and sqr (columns 10, 11, 12), at most 14 in mul2.  The three 29-bit fields: none in
    any multiplier the kernels instantiate (mul, sqr, mul2, dot<K> up to K = 6), as before."""
    plans = {pl["name"]: pl for pl in schedules["bls12_381_fp"]["plans"]}
    for name in ("mul", "sqr"):
        assert plans[name]["cuts"] == 3
        assert [k for k, row in enumerate(plans[name]["cut"]) if any(row)] == [10, 11, 12]
    assert plans["mul2"]["cuts"] <= 14
    for field in ("bn254_fr", "bn254_fp", "bls12_381_fr"):
        for pl in schedules[field]["plans"]:
            if pl["name"] != "dot<16>":
                assert pl["cuts"] == 0, (field, pl["name"])


# ---- the audited build on the largest legal operands ------------------------------------------------------

def largest(f, K):
    """all lower limbs 2^L - 1 under the top limb of K*p - 1 (the largest top limb a value below K*p can have)"""
    shift = f.L * (f.N - 1)
    return (((K * f.p - 1) >> shift) << shift) | ((1 << shift) - 1)


@pytest.mark.parametrize("lift", [0, 1])
def test_multipliers_on_the_largest_legal_operands(shim, lift):
    """The operand ranges of ec.h's table above madd_finite (Pp, Q - X3 < 10p; X1 < 8p; R < 4p; products < 2p) with every
    lower limb at 2^30 - 1: mul, sqr, mul2 report nothing and agree with Python integers.  The values are a little
    above K*p - 1 (same top limb); the products stay far below R*p (R/p = 630)."""
    f = shim.fields["bls12_381_fp"]
    ops = {K: largest(f, K) for K in (1, 2, 4, 8, 10)}
    assert all(to_limbs(v, f.L, f.N)[-1] < TOP_LIMB_BOUND["bls12_381_fp"] for v in ops.values())
    assert 4 * ops[10] ** 2 < f.R * f.p
    shim.reset(lift)
    for a in ops.values():
        got, l = f.val(B.SQR, [a])
        B.check_product(f, got, l, a * a * f.Rinv, ("sqr", hex(a)))
        for b in ops.values():
            got, l = f.val(B.MUL, [a, b])
            B.check_product(f, got, l, a * b * f.Rinv, ("mul", hex(a), hex(b)))
    for a, b, c, d in ((ops[4], ops[10], ops[2], ops[2]), (ops[10], ops[10], ops[2], ops[2]), (ops[2], ops[2], ops[2], ops[2]),
                       (ops[10], ops[4], ops[10], ops[4]), (ops[8], ops[2], ops[10], ops[2])):
        got, l = f.val(B.MUL2, [a, b, c, d])
        B.check_product(f, got, l, (a * b + c * d) * f.Rinv, ("mul2", hex(a), hex(b), hex(c), hex(d)))
    # all lower limbs all-ones but one or two: other quotient digits over the same full columns
    rng = random.Random(5)
    mask = (1 << f.L) - 1

    def vary(v):
        j = rng.randrange(f.N - 1)
        return (v & ~(mask << (f.L * j))) | (rng.randrange(mask + 1) << (f.L * j))
    for i in range(300):
        a, b = vary(ops[10]), vary(ops[(2, 8, 10)[i % 3]])
        got, l = f.val(B.MUL, [a, b])
        B.check_product(f, got, l, a * b * f.Rinv, ("mul", hex(a), hex(b)))
        got, l = f.val(B.SQR, [a])
        B.check_product(f, got, l, a * a * f.Rinv, ("sqr", hex(a)))
        got, l = f.val(B.MUL2, [a, b, ops[2], b])
        B.check_product(f, got, l, (a * b + ops[2] * b) * f.Rinv, ("mul2", hex(a), hex(b)))
    shim.assert_clean()


@pytest.mark.parametrize("lift", [0, 1])
def test_group_law_on_adversarial_operands(shim, lift):
    """madd_finite (both signs), madd, add and dbl of ec.h on BLS12-381 against the oracle's group law: accumulators with
    X below 8p and adversarial limbs (tests/limb_patterns.py), affine operands whose Montgomery x has adversarial
    limbs; with `lift` every product is returned in [p, 2p), so the lazy differences reach the tops of their ranges."""
    c = B.CurveView(shim, "bls12_381")
    cv = c.cv
    affs = c.affine_points(8, 170)
    acc8 = c.accumulators(10, 171, 8)
    acc2 = c.accumulators(6, 173, 2)
    shim.reset(lift)
    for i, (a, A) in enumerate(acc8):
        _, out = c.call(B.EC_DBL, acc=A)
        assert c.decode(out, 2) == B.oadd(a, a, cv)
        b2, B2 = acc2[i % len(acc2)]
        _, out = c.call(B.EC_ADD, acc=A, acc2=B2)
        assert c.decode(out, 2) == B.oadd(a, b2, cv)
        for b, xm, ym in affs:
            for op, bb in ((B.MADD_FIN, b), (B.MADD_FIN_NEG, B.oneg(b, cv))):
                fin, out = c.call(op, acc=A, aff=[xm, ym])
                want = B.oadd(a, bb, cv)
                assert fin == int(want is not None)
                if fin:
                    assert c.decode(out, 8) == want
        xm, ym = a[0] * c.f.R % c.p, a[1] * c.f.R % c.p           # P + P and P - P
        fin, out = c.call(B.MADD_FIN, acc=A, aff=[xm, ym])
        assert fin == 1 and c.decode(out, 8) == B.oadd(a, a, cv)
        fin, out = c.call(B.MADD_FIN_NEG, acc=A, aff=[xm, ym])
        assert fin == 0
    for a, A in acc2:
        for b, xm, ym in affs[:4]:
            _, out = c.call(B.MADD, acc=A, aff=[xm, ym])
            assert c.decode(out, 2) == B.oadd(a, b, cv)
    shim.assert_clean()


def test_a_top_limb_at_the_bound_is_reported(shim):
    """Top limb 2^26 - 1, all lower limbs 2^30 - 1: the extreme the plan is computed for -- no column overflows.  Top
    limb 2^26: the new precondition fires and nothing else, and the result is still right (the plan has slack).
    sqr of such a value is above R*p (2^772 > 630 p^2), so precondition (2), the result range, cannot hold for it:
    there the count is exactly the two of them and the operand check comes first."""
    f = shim.fields["bls12_381_fp"]
    shift = f.L * (f.N - 1)
    ones = (1 << shift) - 1
    bound = TOP_LIMB_BOUND["bls12_381_fp"]
    under, at = ((bound - 1) << shift) | ones, (bound << shift) | ones
    w = largest(f, 2)
    assert under * w * 2 < f.R * f.p and at * w * 2 < f.R * f.p
    shim.reset()
    for a in (under, at):
        for op, elems, want in ((B.MUL, [a, w], a * w), (B.MUL, [w, a], a * w), (B.MUL2, [a, w, w, w], a * w + w * w),
                                (B.MUL2, [w, w, w, a], a * w + w * w), (B.DOT3, [a, w, w, w, w, w], a * w + 2 * w * w)):
            shim.reset()
            got, l = f.val(op, elems)
            B.check_product(f, got, l, want * f.Rinv, (op, hex(a)))
            n, text = shim.violations()
            if a == under:
                assert n == 0, text
            else:
                assert n == 1 and PRECONDITION in text, text
    shim.reset()
    f.val(B.SQR, [under])
    n, text = shim.violations()
    assert n == 1 and "not weak-normal" in text, text           # range (2) only: no column carried out
    shim.reset()
    f.val(B.SQR, [at])
    n, text = shim.violations()
    assert n == 2 and PRECONDITION in text and "sqr" in text, text
    # a lower limb that is not normalised
    shim.reset()
    f.val(B.MUL, [[1 << f.L] + [0] * (f.N - 1), w])
    n, text = shim.violations()
    assert n == 1 and PRECONDITION in text, text
    shim.reset()

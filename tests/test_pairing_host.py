"""csrc/fp_tower.h -- the text the gfx950 pairing kernel compiles -- built for the host (tests/shim/pairing_shim.cpp,
the lanes of a wave replaced by a loop) against kzg_snark_amd/pairing.py's integers: Fp2 and Fp12 arithmetic operation
by operation, then whole pairings.  A tower value sum (a_k + b_k i) w^k is pairing.py's coefficient list with entry
k = a_k - shift b_k and entry k + 6 = b_k (its embed_fp2), so values are compared integer by integer.  The shim runs
plain and with -DKZG_AUDIT (field.h's column and precondition hooks must stay silent, with every multiplier returning
the representative in [p, 2p)), and once as a program of its own under the address and undefined-behaviour sanitizers.
Whole equations also run through the shim's lockstep exchange, which holds every phase to the header's contract (no lane
reads or writes what another lane of the phase writes) at the pair counts whose phases pass a wave's 64 lanes."""
import ctypes
import os
import random
import subprocess
from functools import lru_cache

import pytest

from kzg_snark_amd import curve as C
from kzg_snark_amd import pairing as PR
from limb_patterns import adversarial, from_limbs, header_layout, to_limbs

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "shim")
SRC = os.path.join(SHIM_DIR, "pairing_shim.cpp")
U32 = ctypes.c_uint32
CURVE_IDS = {"bn254": 0, "bls12_381": 1}
FP_STRUCT = {"bn254": "BnFp", "bls12_381": "BlsFp"}
OP_MUL, OP_SQR, OP_INV, OP_MUL_XI, OP_SPARSE, OP_CONJ, OP_FROB1, OP_FROB2, OP_FROB3, OP_CYC_SQR = range(10)
NAMES = ["bls12_381", "bn254"]


@lru_cache(maxsize=None)
def build_shim(audit):
    kind = "audit" if audit else "plain"
    so = os.path.join(SHIM_DIR, f"libpairing_shim_{kind}.so")
    subprocess.run(["g++", "-O1", "-std=c++17", *(["-DKZG_AUDIT"] if audit else []), "-shared", "-fPIC", SRC, "-o", so],
                   check=True)
    return ctypes.CDLL(so)


class Shim:
    def __init__(self, lib, audit):
        self.lib, self.audit = lib, audit
        if audit:
            lib.ps_audit_read.restype = ctypes.c_ulonglong
            lib.ps_audit_reset(1)                       # lift: products come back in [p, 2p)

    def assert_clean(self):
        if not self.audit:
            return
        fn, what, line = ctypes.create_string_buffer(128), ctypes.create_string_buffer(160), ctypes.c_int(0)
        n = self.lib.ps_audit_read(fn, what, 128, ctypes.byref(line))
        assert n == 0, f"{n} violations, first in {fn.value.decode()} (line {line.value}): {what.value.decode()}"


@pytest.fixture(scope="module", params=["plain", "audit"])
def shim(request):
    audit = request.param == "audit"
    return Shim(build_shim(audit), audit)


class Layout:
    """one base field: limb images <-> field values (an element travels as the limbs of its Montgomery form)"""

    def __init__(self, name):
        self.name, self.cid = name, CURVE_IDS[name]
        self.pc = PR._CURVES[name]
        self.p, self.K, self.shift = self.pc.p, self.pc.K, self.pc.shift
        self.L, self.N = header_layout(FP_STRUCT[name])
        self.rinv = pow(1 << (self.L * self.N), -1, self.p)
        self.nw = (self.p.bit_length() + 31) // 32

    def value(self, image):                      # the field element a limb image stands for
        return image * self.rinv % self.p

    def limbs(self, images):                     # limb images (ints below 2p) -> the shim's array
        flat = [v for im in images for v in to_limbs(im, self.L, self.N)]
        return (U32 * len(flat))(*flat)

    def images(self, arr, count):
        return [from_limbs(arr[i * self.N:(i + 1) * self.N], self.L) for i in range(count)]

    def fp12(self, images):                      # 12 limb images (c[0].c0, c[0].c1, c[1].c0, ...) -> pairing.py's list
        v = [self.value(im) for im in images]
        out = [0] * 12
        for k in range(6):
            a, b = v[2 * k], v[2 * k + 1]
            out[k], out[k + 6] = (a - self.shift * b) % self.p, b
        return out

    def operands(self, count, seed, per=2):
        """`count` operands of `per` limb images each: seeded random ones, then adversarial limb images at the top of
        the documented range of every operand here, [0, 2p)"""
        rng = random.Random(seed)
        adv = adversarial(self.p, self.L, self.N, 2, count=12, seed=seed)
        rng.shuffle(adv)
        out = [[rng.randrange(self.p) for _ in range(per)] for _ in range(count)]
        for i in range(count):
            out.append([adv[(i * per + j) % len(adv)] for j in range(per)])
        out.append([2 * self.p - 1] * per)
        return out


@lru_cache(maxsize=None)
def layout(name):
    return Layout(name)


# ---- constants ------------------------------------------------------------------------------------------------------

def test_committed_constants_are_the_generators_output():
    """curve_constants.h (the twist coefficient, the Frobenius coefficients, the loop parameters, both curves' u, all in
    Montgomery limbs) is what gen_constants.py prints; the generator asserts the identities behind them as it runs."""
    import sys
    csrc = os.path.join(HERE, "..", "kzg_snark_amd", "csrc")
    out = subprocess.run([sys.executable, os.path.join(csrc, "gen_constants.py")], capture_output=True, text=True,
                         check=True).stdout
    with open(os.path.join(csrc, "curve_constants.h")) as f:
        assert f.read() == out


# ---- Fp2 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_fp2_against_python(shim, name):
    lay = layout(name)
    p, N = lay.p, lay.N
    F2 = C._Fp2(p)
    xi = (lay.shift, 1)
    ops = lay.operands(6, seed=lay.cid + 3)
    for i, a in enumerate(ops):
        b = ops[(i + 1) % len(ops)]
        av, bv = tuple(lay.value(v) for v in a), tuple(lay.value(v) for v in b)
        want = {OP_MUL: F2.mul(av, bv), OP_SQR: F2.mul(av, av), OP_MUL_XI: F2.mul(av, xi),
                OP_INV: F2.inv(av) if any(av) else (0, 0)}
        for op, w in want.items():
            out = (U32 * (2 * N))()
            assert shim.lib.ps_fp2(lay.cid, op, lay.limbs(a), lay.limbs(b), out) == 0
            got = tuple(lay.value(v) for v in lay.images(out, 2))
            assert got == w, (op, i)
    out = (U32 * (2 * N))()
    zero = lay.limbs([0, 0])
    assert shim.lib.ps_fp2(lay.cid, OP_INV, zero, zero, out) == 0
    assert [lay.value(v) for v in lay.images(out, 2)] == [0, 0]                               # inv(0) = 0
    shim.assert_clean()


# ---- Fp12 -----------------------------------------------------------------------------------------------------------

def fp12_call(shim, lay, op, a, b=None):
    out = (U32 * (12 * lay.N))()
    assert shim.lib.ps_fp12(lay.cid, op, lay.limbs(a), lay.limbs(b if b is not None else a), out) == 0
    return lay.images(out, 12)


@pytest.mark.parametrize("name", NAMES)
def test_fp12_mul_sqr_inv_sparse_against_python(shim, name):
    lay = layout(name)
    K = lay.K
    mask = shim.lib.ps_line_mask(lay.cid)
    assert mask == (0b001011 if name == "bn254" else 0b001101)
    ops = lay.operands(3, seed=lay.cid + 11, per=12)
    for i, a in enumerate(ops):
        b = ops[(i + 1) % len(ops)]
        A, B = lay.fp12(a), lay.fp12(b)
        assert lay.fp12(fp12_call(shim, lay, OP_MUL, a, b)) == K.mul(A, B), i
        assert lay.fp12(fp12_call(shim, lay, OP_SQR, a)) == K.mul(A, A), i
        assert lay.fp12(fp12_call(shim, lay, OP_CONJ, a)) == K.conj(A), i
        inv = lay.fp12(fp12_call(shim, lay, OP_INV, a))
        assert K.mul(inv, A) == K.one and inv == K.inv(A), i
        line = [v if (mask >> (j // 2)) & 1 else 0 for j, v in enumerate(b)]             # a line's coefficients only
        assert lay.fp12(fp12_call(shim, lay, OP_SPARSE, a, b)) == K.mul(A, lay.fp12(line)), i
    assert lay.fp12(fp12_call(shim, lay, OP_INV, [0] * 12)) == K.zero                       # inv(0) = 0
    shim.assert_clean()


@pytest.mark.parametrize("name", NAMES)
def test_frobenius_and_cyclotomic_squaring_against_python(shim, name):
    lay = layout(name)
    K, p = lay.K, lay.p
    ops = lay.operands(1, seed=lay.cid + 23, per=12)
    for i, a in enumerate(ops):
        A = lay.fp12(a)
        for j, op in ((1, OP_FROB1), (2, OP_FROB2), (3, OP_FROB3)):
            assert lay.fp12(fp12_call(shim, lay, op, a)) == K.pow(A, p ** j), (i, j)
        # the easy part of the final exponentiation lands in the cyclotomic subgroup, where the squaring is defined
        e = fp12_call(shim, lay, OP_MUL, fp12_call(shim, lay, OP_CONJ, a), fp12_call(shim, lay, OP_INV, a))
        e = fp12_call(shim, lay, OP_MUL, fp12_call(shim, lay, OP_FROB2, e), e)
        Ev = K.mul(K.conj(A), K.inv(A))
        Ev = K.mul(K.pow(Ev, p * p), Ev)
        assert lay.fp12(e) == Ev
        assert lay.fp12(fp12_call(shim, lay, OP_CYC_SQR, e)) == K.mul(Ev, Ev), i
    shim.assert_clean()


# ---- whole pairings through the shim's lane loop --------------------------------------------------------------------

def words(ints, nw):
    flat = [(x >> (32 * i)) & 0xffffffff for x in ints for i in range(nw)]
    return (U32 * len(flat))(*flat)


def equation(shim, lay, pairs, entry="ps_equation"):
    """pairs: [(G1 tuple, G2 tuple)] -> (status, pairing.py-shaped value); a point at infinity (z = 0) travels as its
    flag beside zero coordinates, and the flag arrays are NULL when no point of their side is one.  entry: ps_equation
    (HostLanes), or ps_equation_lockstep / ps_equation_lockstep_reverse, which add (conflicts, phases, widest phase)."""
    nw = lay.nw
    inf1 = [P[2] == 0 for P, _ in pairs]
    inf2 = [Q[2] in (0, (0, 0)) for _, Q in pairs]
    g1 = words([0 if f else c for (P, _), f in zip(pairs, inf1) for c in (P[0], P[1])], nw)
    g2 = words([0 if f else c for (_, Q), f in zip(pairs, inf2) for c in (Q[0][0], Q[0][1], Q[1][0], Q[1][1])], nw)
    flags = [(ctypes.c_uint8 * len(pairs))(*f) if any(f) else None for f in (inf1, inf2)]
    out = (U32 * (12 * nw))()
    info = (ctypes.c_ulonglong * 3)(99, 0, 0)
    extra = () if entry == "ps_equation" else (info,)
    st = getattr(shim.lib, entry)(lay.cid, g1, flags[0], g2, flags[1], len(pairs), out, *extra)
    v = [sum(int(out[i * nw + j]) << (32 * j) for j in range(nw)) for i in range(12)]
    val = [0] * 12
    for k in range(6):
        val[k], val[k + 6] = (v[2 * k] - lay.shift * v[2 * k + 1]) % lay.p, v[2 * k + 1]
    return (st, tuple(val), *([tuple(info)] if extra else []))


@pytest.mark.parametrize("name", NAMES)
def test_pairing_values_and_bilinearity(shim, name):
    lay = layout(name)
    cv = C.CURVES[name]
    G1, G2 = C.g1_group(cv), C.g2_group(cv)
    g1, g2 = (cv.g1[0], cv.g1[1], 1), (cv.g2[0], cv.g2[1], (1, 0))
    c = shim.lib.ps_gt_multiple(lay.cid)
    assert c == (1 if name == "bn254" else 3)
    rng = random.Random(lay.cid + 41)
    for _ in range(2):
        a, b = rng.randrange(1, cv.r), rng.randrange(1, cv.r)
        P, Q = G1.multiply(g1, a), G2.multiply(g2, b)
        st, val = equation(shim, lay, [(P, Q)])
        assert st == 1 and val == tuple(lay.K.pow(list(PR.pairing(Q, P, cv)), c))
        st, val = equation(shim, lay, [(P, Q), (G1.neg(G1.multiply(g1, a * b % cv.r)), g2)])
        assert st == 0 and val == tuple(lay.K.one)
    shim.assert_clean()


# ---- the phase contract: whole equations through the shim's lockstep exchange -----------------------------------------
# fp_tower.h: "a body never reads a slot that another lane writes in the same phase".  HostLanes cannot see a violation
# (the later lane reads the new value and the result is whatever the author saw); on the wave it is a race.  Under
# LockstepLanes every lane of a phase starts from the state the phase began with, so a body that reads a neighbour's
# write computes with the old value and the equation's value leaves pairing.py's; two lanes that write one word are
# counted.  The per-pair product phases are k * jobs lanes wide, jobs up to 6: past the 64 lanes of a wave from k = 11
# (66, the 6-job phases) and, for the 5-job phase, from k = 13 (65) -- the widest phase reported back shows the run was
# that wide.  Equations close by the trapdoor: (a_i G1, b_i G2) and one closing pair -(sum a_i b_i - S) G1, G2 give
# e(G1, G2)^S.
HOST_POOL = 8


class HostPool:
    def __init__(self, name):
        self.cv = cv = C.CURVES[name]
        self.G1, self.G2 = C.g1_group(cv), C.g2_group(cv)
        self.g1, self.g2 = (cv.g1[0], cv.g1[1], 1), (cv.g2[0], cv.g2[1], (1, 0))
        rng = random.Random(97 + CURVE_IDS[name])
        self.a = [rng.randrange(1, cv.r) for _ in range(HOST_POOL)]
        self.b = [rng.randrange(1, cv.r) for _ in range(HOST_POOL)]
        self.A = [self.G1.multiply(self.g1, a) for a in self.a]
        self.B = [self.G2.multiply(self.g2, b) for b in self.b]
        self.S = rng.randrange(1, cv.r)
        self._host = {}

    def picks(self, k):                          # the indices (i, j) of the k - 1 pairs before the closing one
        return [(t % HOST_POOL, (3 * t + 1) % HOST_POOL) for t in range(k - 1)]

    def closed(self, k, delta=0, skip1=(), skip2=()):
        """k pairs with the product e(G1, G2)^delta: pair t is (a_i G1, b_j G2), with G1 at infinity for t in skip1 and
        G2 for t in skip2, and the last pair closes the ones that are left"""
        idx = self.picks(k)
        total = sum(self.a[i] * self.b[j] for t, (i, j) in enumerate(idx) if t not in skip1 and t not in skip2)
        pairs = [(self.G1.Z if t in skip1 else self.A[i], self.G2.Z if t in skip2 else self.B[j])
                 for t, (i, j) in enumerate(idx)]
        return pairs + [(self.G1.neg(self.G1.multiply(self.g1, (total - delta) % self.cv.r)), self.g2)]

    def host(self, P, Q):                        # pairing.py's value, computed once per pair of points
        if (P, Q) not in self._host:
            self._host[P, Q] = list(PR.pairing(Q, P, self.cv))
        return self._host[P, Q]


@lru_cache(maxsize=None)
def host_pool(name):
    return HostPool(name)


def run_lockstep(shim, lay, pairs, status, value, widest=None):
    """the equation under LockstepLanes, lanes in both orders: no word written by two lanes of a phase, and the status
    and value that pairing.py's algebra gives -- which HostLanes' loop gives too"""
    k = len(pairs)
    widest = (36 if k <= 6 else 6 * k) if widest is None else widest
    value = tuple(value)
    st, val, (conflicts, phases, wide) = equation(shim, lay, pairs, "ps_equation_lockstep")
    assert conflicts == 0 and st == status and val == value, (k, conflicts, st)
    assert wide == widest and phases > 1000, (k, wide, phases)
    rst, rval, (rconflicts, rphases, rwide) = equation(shim, lay, pairs, "ps_equation_lockstep_reverse")
    assert (rconflicts, rst, rval, rphases, rwide) == (0, st, val, phases, wide), (k, rconflicts, rst)
    assert equation(shim, lay, pairs) == (st, val), k
    shim.assert_clean()


@pytest.mark.parametrize("k", [1, 2, 11, 13, 16])
@pytest.mark.parametrize("name", NAMES)
def test_phase_contract_under_lockstep_lanes(shim, name, k):
    lay, pool = layout(name), host_pool(name)
    K = lay.K
    c = shim.lib.ps_gt_multiple(lay.cid)
    if k == 1:
        P, Q = pool.A[0], pool.B[1]
        run_lockstep(shim, lay, [(P, Q)], 1, K.pow(pool.host(P, Q), c))
    else:
        run_lockstep(shim, lay, pool.closed(k), 0, K.one)


@pytest.mark.parametrize("name", NAMES)
def test_phase_contract_with_skipped_pairs(shim, name):
    lay, pool = layout(name), host_pool(name)
    K = lay.K
    c = shim.lib.ps_gt_multiple(lay.cid)
    k = 11
    # pair 0 skipped by its G1 flag, pair 5 by its G2 flag, the closing pair sums the live ones: idle lanes inside the
    # 66-lane phases, among them lane 0 and lanes of the wrapped range's pair
    run_lockstep(shim, lay, pool.closed(k, skip1=(0,), skip2=(5,)), 0, K.one)
    # only the last pair live (lanes 60 .. 65 of a 6-job phase): its pairing, as at k = 1
    P, Q = pool.A[0], pool.B[1]
    alone = [(pool.G1.Z, pool.B[t % HOST_POOL]) if t % 2 else (pool.A[t % HOST_POOL], pool.G2.Z) for t in range(k - 1)]
    run_lockstep(shim, lay, alone + [(P, Q)], 1, K.pow(pool.host(P, Q), c))


@pytest.mark.parametrize("name", NAMES)
def test_a_value_that_is_not_one_at_eleven_pairs(shim, name):
    """the product of k = 11 pairs is E^(c S), E = pairing.py's e(G1, G2), S != 0: a value past k = 2 that one wrong
    line or one pair's lost lane would change"""
    lay, pool = layout(name), host_pool(name)
    c = shim.lib.ps_gt_multiple(lay.cid)
    E = pool.host(pool.g1, pool.g2)
    want = lay.K.pow(E, c * pool.S % pool.cv.r)
    assert want != lay.K.one
    run_lockstep(shim, lay, pool.closed(11, delta=pool.S), 1, want)


def test_shim_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """pairing_shim.cpp with its own main(): pairings of the generators (e(G1, G2) e(-G1, G2) = 1 -- under HostLanes and
    under the lockstep exchange, whose snapshot code so runs under the sanitizers --, infinity flags,
    malformed points) and the tower operations on both curves, built with -DKZG_AUDIT and
    -fsanitize=address,undefined (no recovery, static runtimes) and run as a program of its own.  Exit status 0 = no
    sanitizer report, no audit violation, every check of the program passed."""
    exe = str(tmp_path / "pairing_shim_san")
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-DKZG_AUDIT", "-DPAIRING_SHIM_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert "no violations" in res.stdout

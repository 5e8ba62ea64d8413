"""The G1 transform (g1_level_kernel, csrc/domain.hip) and the FK20 code around it on inputs that make butterflies add an
infinite operand, a point to itself and a point to its negative (tests/g1_fft_profiles.py builds them;
tests/test_g1_fft_profiles_host.py counts which butterfly does what).  Every key point is a known multiple of G, loaded
with kzg_srs_load_g1, so every output is [k] G for a scalar k from the definition -- the long-division quotient
against the key's scalars, the scalar inverse DFT -- and one oracle scalar multiple per distinct k.  Every comparison
is exact: canonical affine words and the infinity flag."""
import numpy as np
import pytest

import g1_fft_profiles as P
from oracle import c_oracle
from oracle import py_oracle as O

pytestmark = pytest.mark.gpu


class Rig:
    """one curve: the context and [k] G by scalar, from the C oracle, cached for the module"""

    def __init__(self, native, curve):
        self.native, self.curve, self.cv = native, curve, O.curve(curve)
        self.ctx = native.get_context(curve)
        self.L = self.ctx.fp_limbs
        self.g = native.ints_to_limbs(list(self.cv.g1), self.L).reshape(-1)
        self.cache = {0: None}

    def points(self, scalars):
        """(xy uint64[n, 2L], inf uint8[n]) of [k] G for every k; an infinite point's words are zero"""
        xy = np.zeros((len(scalars), 2 * self.L), dtype=np.uint64)
        inf = np.zeros(len(scalars), dtype=np.uint8)
        for i, k in enumerate(scalars):
            k %= self.cv.r
            if k not in self.cache:
                out, oinf = c_oracle.g1_mul(self.curve, self.g, k)
                assert not oinf
                self.cache[k] = out
            if self.cache[k] is None:
                inf[i] = 1
            else:
                xy[i] = self.cache[k]
        return xy, inf

    def load(self, scalars):
        return self.ctx.srs_load_g1(*self.points(scalars))

    def check(self, got_xy, got_inf, scalars, what):
        """got == [k] G for every k, on the flag and, where finite, on every word"""
        want_xy, want_inf = self.points(scalars)
        got_xy, got_inf = np.asarray(got_xy).reshape(want_xy.shape), np.asarray(got_inf).reshape(-1)
        finite = want_inf == 0
        bad = np.flatnonzero((got_inf != want_inf) | (finite & (got_xy != want_xy).any(axis=1)))
        assert bad.size == 0, (what, "first mismatches at", bad[:8].tolist(), "of", len(scalars),
                               "flags", got_inf[bad[:8]].tolist(), "want", want_inf[bad[:8]].tolist())

    def pack(self, polys, stride):
        arr = np.zeros((len(polys), stride, 4), dtype=np.uint64)
        for j, p in enumerate(polys):
            if p:
                arr[j, :len(p)] = self.native.ints_to_limbs([int(c) for c in p])
        return arr


@pytest.fixture(scope="module")
def rigs(native):
    return {c: Rig(native, c) for c in P.CURVES}


def same_points(a, b):
    """two device outputs (xy, inf, ...) agree on every flag and on the words of every finite point"""
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0][a[1] == 0], b[0][b[1] == 0])


# ---- 1. kzg_srs_lagrange on loaded keys ------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("log_n", [4, 6])
@pytest.mark.parametrize("part", ["profile", "geometric", "spike", "level"])
def test_lagrange_key_of_every_key_profile(rigs, curve, log_n, part):
    """part: the key profiles; a_t = w^(et) for every e; one finite point at every position; the vectors with a
    chosen class at every butterfly of one level"""
    rig = rigs[curve]
    r, n = rig.cv.r, 1 << log_n
    w = rig.cv.root_of_unity(n)
    ran = 0
    for name, key in P.lagrange_cases(log_n, rig.cv).items():
        head = name.split("_")[0]
        if (head if head in ("geometric", "spike", "level") else "profile") != part:
            continue
        srs = rig.load(key)
        lk = rig.ctx.srs_lagrange(srs, log_n, w)
        rig.check(*lk.export(), P.lagrange_key_scalars(key, w, r), (name, "lagrange key"))
        lk.close()
        srs.close()
        ran += 1
    assert ran == {"profile": len(P.BASE_KEYS), "geometric": n, "spike": n, "level": 2 * log_n}[part]


# ---- 2. kzg_domain_table_create + kzg_open_domain --------------------------------------------------------------------
CROSS_CHECKED = ("all_equal", "all_minus_one", "single_1", "single_mid", "single_last", "geometric_0", "geometric_1",
                 "h_constant", "h_alternating", "h_spike_0", "h_geometric_1")


def open_domain(rig, table, polys, n, w):
    stride = max(max((len(p) for p in polys), default=1), 1)
    return rig.ctx.open_domain(table, rig.pack(polys, stride), [len(p) for p in polys], stride, w, evals=False)


@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("log_n,full", [(4, True), (6, False)])
@pytest.mark.parametrize("kname", P.BASE_KEYS)
def test_open_domain_over_key_and_polynomial_profiles(rigs, curve, log_n, full, kname):
    """All n proofs of every polynomial profile in ONE batch per key; the tau key's batch also holds the polynomials
    built from a target h.  The all-infinity key gives O everywhere, the zero and empty polynomials too.  For keys
    that are powers of a tau, a sample of the structured polynomials is opened with kzg_open at the same points."""
    rig = rigs[curve]
    r, n = rig.cv.r, 1 << log_n
    w = rig.cv.root_of_unity(n)
    (key, tau), = [v for k, v in P.key_profiles(log_n, 0, rig.cv).items() if k == kname]
    (polys,) = [ps for k, _, ps in P.domain_cases(log_n, rig.cv, full) if k == kname]
    names = sorted(polys)
    srs = rig.load(key)
    table = rig.ctx.domain_table(srs, log_n)
    xy, inf, _ = open_domain(rig, table, [polys[p] for p in names], n, w)
    for j, pname in enumerate(names):
        want = P.coset_proof_scalars(key, polys[pname], 1, n, w, r)
        rig.check(xy[j], inf[j], want, (kname, pname))
        if kname == "all_inf" or pname in ("zero", "empty"):
            assert inf[j].all()
    if tau is not None:
        one = rig.native.int_to_words(1)
        sample = [p for p in CROSS_CHECKED + ("h_level_%d_0" % (log_n - 1),) if p in polys]
        assert len(sample) >= (8 if kname == "tau" else 2), sample
        for pname in sample:
            p = polys[pname]
            j = names.index(pname)
            arr = rig.pack([p], n)
            for i in (0, 1, n // 2, n - 1):
                oxy, oinf, _ = rig.ctx.open(srs, arr, [len(p)], n, rig.native.int_to_words(pow(w, i, r)), one)
                assert oinf[0] == inf[j, i] and (oinf[0] or np.array_equal(np.asarray(oxy).reshape(-1), xy[j, i])), \
                    (kname, pname, i)
    table.close()
    srs.close()


# ---- 3. kzg_coset_table_create + kzg_open_cosets, every Straus group ---------------------------------------------------
COSET_PARAMS = [(log_n, log_l, kname) for log_n in (6, 4) for log_l in range(min(log_n, 6))
                for kname in P.BASE_KEYS + (P.PAIR_KEYS if log_l else ())]


@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("log_n,log_l,kname", COSET_PARAMS)
def test_open_cosets_at_every_group_size(rigs, curve, log_n, log_l, kname):
    """N = n and 2n; "open_cosets_group" 0 (the library's rule) and 1..5 (G = 1 .. 16, clipped to l): the proofs equal
    the definition and do not depend on the group.  At log_n = 6 this is G = 16 in a single group (l = 16), G = 16 in
    two groups through dom_group_sum_kernel (l = 32) and G = 1 in 32 groups (l = 32, value 1); the keys whose
    sub-tables coincide or are opposite, with c_(sl) = c_(sl+1), make the chain itself double and cancel."""
    rig = rigs[curve]
    r, n, l = rig.cv.r, 1 << log_n, 1 << log_l
    (polys,) = [ps for k, _, ps in P.coset_cases(log_n, log_l, rig.cv) if k == kname]
    key = P.key_profiles(log_n, log_l, rig.cv)[kname][0]
    names = sorted(polys)
    stride = max(len(polys[p]) for p in names)
    arr, lens = rig.pack([polys[p] for p in names], stride), [len(polys[p]) for p in names]
    srs = rig.load(key)
    table = rig.ctx.coset_table(srs, log_n, log_l)
    try:
        for log_N in (log_n + 1, log_n):
            N = 1 << log_N
            w = rig.cv.root_of_unity(N)
            rig.ctx.set_tuning("open_cosets_group", 0)
            ref = rig.ctx.open_cosets(table, arr, lens, stride, log_N, w, evals=False)
            for j, pname in enumerate(names):
                rig.check(ref[0][j], ref[1][j], P.coset_proof_scalars(key, polys[pname], l, N, w, r),
                          (kname, pname, "N", N))
            for value in range(1, 6):
                rig.ctx.set_tuning("open_cosets_group", value)
                got = rig.ctx.open_cosets(table, arr, lens, stride, log_N, w, evals=False)
                assert same_points(got, ref), (kname, "N", N, "open_cosets_group", value)
    finally:
        rig.ctx.set_tuning("open_cosets_group", 0)
    table.close()
    srs.close()

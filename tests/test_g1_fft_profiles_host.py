"""What tests/test_g1_transforms_gpu.py covers, pinned on the CPU: the inputs of tests/g1_fft_profiles.py reach the
exceptional branches of Ec::add inside every G1 transform (counted by the census, a replay of g1_level_kernel's
schedule on scalars), and the definition the GPU results are compared with agrees with the oracle's opening.  A later
edit of the profiles that drops a case fails here."""
import random
from collections import Counter

import pytest

import g1_fft_profiles as P
from oracle import py_oracle as O


def union(censuses):
    tot = Counter()
    for c in censuses:
        tot.update(c)
    return tot


def pairs(census):
    return {(cls, unit) for (_, cls, unit) in census}


EVERY_EXCEPTION = {(cls, unit) for cls in P.EXCEPTIONAL for unit in (True, False)}


def test_the_census_on_cases_worked_by_hand():
    r = O.BN254.r
    root = O.BN254.root_of_unity(4)                           # a 4-th root: i
    # bit-reversed load of (a0 a1 a2 a3) is (a0 a2 a1 a3); level 0 pairs (a0, a2) and (a1, a3)
    seen, out = P.dit_census([5, 7, 5, 0], root, r)
    assert seen[(0, "A==B", True)] == 1 and seen[(0, "B_inf", True)] == 1
    # level 1: (10, 7) with twiddle 1 and (0, 7 i) with twiddle i
    assert seen[(1, "generic", True)] == 1 and seen[(1, "A_inf", False)] == 1 and sum(seen.values()) == 4
    assert out == P.dft([5, 7, 5, 0], root, r)
    seen, _ = P.dit_census([3, 4, 3, 4], root, r)
    assert seen[(1, "both_inf", False)] == 1                  # (3 - 3, 4 - 4) after level 0
    seen, _ = P.dit_census([1, 0, r - 1, 0], root, r)
    assert seen[(0, "A==-B", True)] == 1 and seen[(0, "both_inf", True)] == 1
    assert P.cells(2) == {(0, c, True) for c in P.CLASSES} | {(1, c, u) for c in P.CLASSES for u in (True, False)}


@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("log_n", [4, 6])
def test_lagrange_keys_reach_every_cell(curve, log_n):
    """kzg_srs_lagrange on loaded keys: any vector is an input, so every (level, class, twiddle kind) is reached."""
    cv = O.curve(curve)
    r, n = cv.r, 1 << log_n
    w = cv.root_of_unity(n)
    winv = pow(w, -1, r)
    seen = []
    for name, key in P.lagrange_cases(log_n, cv).items():
        census, out = P.dit_census(key, winv, r)
        assert [x * pow(n, -1, r) % r for x in out] == P.lagrange_key_scalars(key, w, r), name   # the replay transforms
        seen.append(census)
    assert set(union(seen)) == P.cells(log_n)


@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("log_n", [4, 6])
def test_built_vectors_put_the_asked_class_at_the_asked_level(curve, log_n):
    cv = O.curve(curve)
    r, n = cv.r, 1 << log_n
    w = cv.root_of_unity(n)
    for s in range(log_n):
        for last_zero in (False, True):
            x = P.build_level_vector(log_n, w, s, r, 9, shift=1, last_zero=last_zero)
            assert not last_zero or x[n - 1] == 0
            census, _ = P.dit_census(x, w, r)
            at_s = Counter()
            for (lv, cls, _), k in census.items():
                if lv == s:
                    at_s[cls] += k
            want = Counter(P.CLASSES[(b + k + 1) % 6] for b in range(n >> (s + 1)) for k in range(1 << s))
            if last_zero:                 # the last block's B operands are not free: allow its 2^s butterflies to move
                assert sum((want - at_s).values()) <= 1 << s
            else:
                assert at_s == want


# cells no input of the final transform can reach, by name.  N = n: h is free but for h_(n-1) = O, which only fixes
# one operand of one butterfly per level.  N = 2n: h_u = O for every u >= n - 1, the odd half of the bit-reversed
# load, so at level 0 every B is infinite.
FINAL_UNREACHABLE = {
    0: set(),
    1: {(0, cls, True) for cls in ("A_inf", "A==B", "A==-B", "generic")},
}


@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("log_n", [4, 6])
def test_final_transform_inputs_reach_every_reachable_cell(curve, log_n):
    """The final FK20 transform (l = 1): its input h ends in O.  Every cell is reached with N = n; with N = 2n every
    cell but level 0's with a finite B, and those never occur."""
    cv = O.curve(curve)
    r, n = cv.r, 1 << log_n
    w = cv.root_of_unity(n)
    hs = P.h_profiles(log_n, w, r)
    assert all(len(h) == n and h[n - 1] == 0 for h in hs.values())
    seen = union(P.dit_census(h, w, r)[0] for h in hs.values())
    assert set(seen) == P.cells(log_n) - FINAL_UNREACHABLE[0]
    # the polynomial built from h has h as its FK20 vector under the tau key
    key = P.key_profiles(log_n, 0, cv)["tau"][0]
    w2 = cv.root_of_unity(2 * n)
    padded = []
    for name in ("h_level_%d_0" % (log_n - 1), "h_geometric_3", "h_spike_2", "h_constant"):
        p = P.poly_from_h(hs[name], P.TAU, 1, r)
        assert P.fk20_stages(key, p, log_n, 0, log_n, w, cv)["final"][0] == hs[name], name
        padded.append(P.fk20_stages(key, p, log_n, 0, log_n + 1, w2, cv)["final"])
        assert padded[-1][0] == hs[name] + [0] * n
    seen2 = union(P.dit_census(h + [0] * n, w2, r)[0] for h in hs.values())
    assert set(seen2) & FINAL_UNREACHABLE[1] == set()
    assert {c for c in seen2 if c[0] == 0} == {(0, "B_inf", True), (0, "both_inf", True)}
    assert pairs(seen2) >= EVERY_EXCEPTION


@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("log_n,full", [(4, True), (6, False)])
def test_table_and_inverse_transforms_meet_every_exception_at_both_twiddle_kinds(curve, log_n, full):
    """Their inputs are constrained (the key's zero-padding; c^ . S), so the claim is per class: each exceptional
    class occurs with a unit and with a non-unit twiddle, in the product of profiles the GPU test opens."""
    cv = O.curve(curve)
    r, n = cv.r, 1 << log_n
    w = cv.root_of_unity(n)
    table, inverse = [], []
    for kname, key, polys in P.domain_cases(log_n, cv, full):
        for pname, p in polys.items():
            if kname == "tau" and pname.startswith("h_"):
                continue                                                  # those aim at the final transform
            st = P.fk20_stages(key, p, log_n, 0, log_n, w, cv)
            assert st["proofs"] == P.coset_proof_scalars(key, p, 1, n, w, r), (kname, pname)
            inverse.append(P.dit_census(*st["inverse"], r)[0])
        table.append(P.dit_census(*st["table"][0], r)[0])
    assert pairs(union(table)) >= EVERY_EXCEPTION
    assert pairs(union(inverse)) >= EVERY_EXCEPTION
    # an infinite operand under a non-unit twiddle: the all-infinity key alone gives it at every level above 0
    all_inf = [k for k in P.domain_cases(log_n, cv, full) if k[0] == "all_inf"][0]
    st = P.fk20_stages(all_inf[1], all_inf[2]["all_equal"], log_n, 0, log_n, w, cv)
    assert set(P.dit_census(*st["inverse"], r)[0]) == {(s, "both_inf", u) for (s, _, u) in P.cells(log_n + 1)}
    assert st["proofs"] == [0] * n


@pytest.mark.parametrize("curve", P.CURVES)
def test_fk20_in_scalars_equals_the_definition_for_every_coset_case(curve):
    """The staged replay the census reads is the computation the definition describes: every l, N = n and 2n."""
    cv = O.curve(curve)
    r, log_n = cv.r, 4
    for log_l in range(log_n):
        for kname, key, polys in P.coset_cases(log_n, log_l, cv):
            for log_N in (log_n, log_n + 1):
                w = cv.root_of_unity(1 << log_N)
                for pname, p in polys.items():
                    st = P.fk20_stages(key, p, log_n, log_l, log_N, w, cv)
                    assert st["proofs"] == P.coset_proof_scalars(key, p, 1 << log_l, 1 << log_N, w, r), \
                        (log_l, kname, log_N, pname)


@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("log_n", [4, 6])
def test_coinciding_and_opposite_sub_tables_double_and_cancel_in_the_straus_chain(curve, log_n):
    """c_(sl) = c_(sl+1) gives sub-tables 0 and 1 the same scalar, and "pair_only" leaves the other sub-tables without
    coefficients, so nothing precedes them in the chain: with equal points its second addition at the top set bit is
    P + P, with opposite points P + (-P), after which the accumulator is infinite again."""
    cv = O.curve(curve)
    r = cv.r
    assert set(P.key_profiles(log_n, 0, cv)) == set(P.BASE_KEYS)
    assert set(P.key_profiles(log_n, 1, cv)) == set(P.BASE_KEYS + P.PAIR_KEYS)
    w = cv.root_of_unity(1 << log_n)
    for log_l in range(1, log_n):
        cases = {k: (key, polys) for k, key, polys in P.coset_cases(log_n, log_l, cv)}
        for kname, cls in (("const_along_j", "A==B"), ("opposite_pairs", "A==-B")):
            key, polys = cases[kname]
            st = P.fk20_stages(key, polys["pair_only"], log_n, log_l, log_n, w, cv)
            hit = 0
            for e, pts in zip(st["scalars"], st["points"]):
                assert e[0] == e[1]
                if e[0] and pts[0]:
                    assert pts[1] == (pts[0] if cls == "A==B" else r - pts[0])
                    seen = P.straus_census(e[:2], pts[:2], r)
                    assert seen[cls] >= 1 and seen["A_inf"] >= 1
                    hit += 1
            assert hit >= (1 << log_n >> log_l)                          # at least half of the 2m outputs


@pytest.mark.parametrize("curve", P.CURVES)
@pytest.mark.parametrize("n", [4, 8])
def test_the_definition_equals_the_oracle_opening_on_a_tau_key(curve, n):
    """Pins the reference itself: [sum_t q_t tau^t] G is O.open_'s proof, at every point of the domain and one off it;
    for cosets, l = 2, the commitment of the long-division quotient."""
    cv = O.curve(curve)
    r = cv.r
    rng = random.Random(n)
    log_n = n.bit_length() - 1
    key = P.key_profiles(log_n, 0, cv)["tau"][0]
    assert key == [pow(P.TAU, t, r) for t in range(n)]
    ck = O.setup(n - 1, P.TAU, cv)
    G = O.from_affine(cv.g1)
    w = cv.root_of_unity(n)
    polys = P.poly_profiles(log_n, cv)
    for pname in ("random", "all_equal", "single_1", "geometric_1", "zero"):
        p = polys[pname]
        ks = P.coset_proof_scalars(key, p, 1, n, w, r)
        for i, z in enumerate([pow(w, i, r) for i in range(n)] + [rng.randrange(r)]):
            k = ks[i] if i < n else P.proof_scalar(key, p, 1, z, r)
            assert O.normalize(O.multiply(G, k, cv), cv) == O.normalize(O.open_(ck, [p], z, 1, cv)[0], cv), (pname, i)
        a = pow(w, 2, r)
        q = P.coset_quotient(p, 2, a, r)
        prod = [0] * (len(q) + 2)                                                   # q (X^2 - a)
        for t, x in enumerate(q):
            prod[t] = (prod[t] - a * x) % r
            prod[t + 2] = (prod[t + 2] + x) % r
        assert all((c - d) % r == 0 for c, d in zip(p[2:], prod[2:]))               # the remainder has degree < l
        assert O.normalize(O.multiply(G, P.proof_scalar(key, p, 2, w, r), cv), cv) == \
            O.normalize(O.commit(ck, [q], cv)[0], cv)

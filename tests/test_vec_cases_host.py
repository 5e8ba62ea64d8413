"""What tests/test_vec_edges_gpu.py covers, pinned on the CPU: the constants of tests/vec_cases.py are those of
csrc/poly.hip, the sizes bracket every change of the three launch plans, every labelled input hits the regime its label
names, and the expected lists are the plain definitions.  An edit of the kernels' constants or of the case tables that
makes a case test nothing fails here."""
import os
import re

import pytest

import vec_cases as V
from oracle import py_oracle as O

FIELDS = {"bls12_381": O.BLS12_381.r, "bn254": O.BN254.r}


def test_the_constants_are_the_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "kzg_snark_amd", "csrc", "poly.hip")) as f:
        src = f.read()
    for name in ("LC", "DOT_G", "MAXK"):
        found = re.findall(r"^constexpr uint32_t %s = (\d+);" % name, src, flags=re.M)
        assert [int(x) for x in found] == [getattr(V, name)], name
    # the two numbers of the plans that are not named constants
    assert re.search(r"vec_inverse_kernel<F>, dim3\(\(uint32_t\)\(\(chunks \+ 63\) / 64\)\), dim3\(%d\)" % V.INVERSE_BLOCK,
                     src)
    assert re.search(r"uint32_t lt = %d;\s*\n\s*while \(\(\(size_t\)LC << lt\) < n && lt < 24\) \+\+lt;" % V.POWERS_LT0,
                     src)
    assert max(V.PREFIX_NS + V.INVERSE_NS + V.POWERS_NS + V.ALIAS_NS) <= V.MAX_N == 40000


def test_the_prefix_sizes_reach_every_level_count_full_and_one_past():
    LC = V.LC
    assert V.prefix_levels(1) == [1] and V.prefix_levels(33) == [33, 2]
    assert V.prefix_levels(32769) == [32769, 1025, 33, 2]
    by_n = {n: V.prefix_levels(n) for n in V.PREFIX_NS}
    assert {len(m) for m in by_n.values()} == {1, 2, 3, 4}
    for depth in (1, 2, 3):                                    # LC^depth fills `depth` levels; one more adds a level of 2
        full, past = by_n[LC ** depth], by_n[LC ** depth + 1]
        assert len(full) == depth and full[-1] == LC
        assert len(past) == depth + 1 and past[-2:] == [LC + 1, 2]
        assert len(by_n[max(LC ** depth - 1, 1)]) == depth
    for n, m in by_n.items():
        assert m[0] == n and m[-1] <= LC and all(x > LC for x in m[:-1])
        assert all(m[i + 1] == -(-m[i] // LC) for i in range(len(m) - 1))


def test_the_inverse_sizes_bracket_the_change_of_the_thread_count():
    assert V.inverse_threads(2048) == 64 and V.inverse_threads(2049) == 128
    assert {2047, 2048, 2049} <= set(V.INVERSE_NS)
    assert [V.inverse_threads(n) for n in V.INVERSE_NS] == [64, 64, 64, 64, 64, 64, 128, 192, 1280]
    for n in V.INVERSE_NS:
        T = V.inverse_threads(n)
        batches = [V.inverse_batch(n, t) for t in range(T)]
        assert sorted(i for b in batches for i in b) == list(range(n))       # a partition of the vector
        assert max(len(b) for b in batches) <= V.LC                         # what the kernel's comment promises
    assert max(len(V.inverse_batch(40000, t)) for t in range(1280)) == V.LC  # and a full batch is among them


def test_the_powers_sizes_bracket_both_changes_of_the_width():
    T = {n: V.powers_threads(n) for n in V.POWERS_NS}
    assert (T[4096], T[4097], T[8192], T[8193]) == (128, 256, 256, 512)
    assert T[1] == T[127] == T[128] == T[129] == T[4095] == 128
    assert any(n < T[n] for n in V.POWERS_NS) and 127 < T[127]              # idle threads
    assert any(n > T[n] and n % T[n] for n in V.POWERS_NS)                  # a strided loop with a ragged last step
    for n in V.POWERS_NS:
        assert -(-n // T[n]) <= V.LC                                        # LC elements per thread at the most


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_the_inverse_cases_hit_the_batches_they_name(field):
    r = FIELDS[field]
    seen = set()
    for n in V.INVERSE_NS:
        T = V.inverse_threads(n)
        cases = V.inverse_cases(n, r)
        assert len({c.label for c in cases}) == len(cases)
        chosen = V.inverse_chosen_threads(n)
        assert (n > T) == bool(chosen)
        if chosen:
            assert chosen[0] == 0 and len(chosen) == 3 and chosen[0] < chosen[1] < chosen[2] < T
            assert len(V.inverse_batch(n, chosen[-1])) >= 2
            assert chosen[-1] == T - 1 or len(V.inverse_batch(n, chosen[-1] + 1)) < 2
        for c in cases:
            assert len(c.a) == len(c.want) == n
            m = re.fullmatch(r"thread(\d+):(.*)", c.label)
            if not m:
                continue
            t, kind = int(m.group(1)), m.group(2)
            seen.add(kind)
            batch = V.inverse_batch(n, t)
            zeros = {i for i, x in enumerate(c.a) if x == 0}
            if kind == "whole-batch-zero":
                assert len(batch) >= 2 and zeros == set(batch)
                others = [V.inverse_batch(n, u) for u in range(T) if u != t]
                assert not any(b and set(b) <= zeros for b in others)
            elif kind == "first-zero":
                assert len(batch) >= 2 and zeros == {min(batch)} == {t}
            elif kind == "last-zero":
                assert len(batch) >= 2 and zeros == {max(batch)} and max(batch) + T >= n
            else:
                assert kind == "tail-single-zero" and zeros == set(batch) and len(batch) == 1
                assert t + 1 == T or not V.inverse_batch(n, t + 1)         # the last thread with work
    assert seen == {"whole-batch-zero", "first-zero", "last-zero", "tail-single-zero"}
    # batches of more than one element are zeroed at both thread counts of the change and in the last block of several
    for n in (2048, 2049, 4097, 40000):
        assert sum(c.label.endswith("whole-batch-zero") for c in V.inverse_cases(n, r)) == 3


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_the_expected_lists_are_the_definitions(field):
    r = FIELDS[field]
    a = V.base_vector(r, V.MAX_N)
    assert len(a) == V.MAX_N and all(1 < x < r - 1 for x in a)
    # the definitions themselves
    inv = V.ref_inverse(a[:3000] + [0, 1, r - 1], r)
    assert all(x * y % r == 1 for x, y in zip(a[:3000] + [0, 1, r - 1], inv) if x) and inv[3000:] == [0, 1, r - 1]
    pre = V.ref_prefix(a[:3000], r)
    assert pre[0] == 1 and all(pre[i + 1] == pre[i] * a[i] % r for i in range(2999))
    s, c0 = a[7], a[8]
    pw = V.ref_mul_powers(a[:8193], s, c0, r)
    for i in (0, 1, 2, 127, 128, 129, 4095, 4096, 4097, 8191, 8192):
        assert pw[i] == a[i] * c0 * pow(s, i, r) % r
    assert V.ref_mul_powers([5, 6, 7], 0, 3, r) == [15, 0, 0]               # 0^0 = 1
    w = V.fourth_root_of_unity(r)
    assert w * w % r == r - 1 and pow(w, 4, r) == 1 and w not in (1, r - 1)
    assert V.ref_op("add", [r - 1], [2], r) == [1] and V.ref_op("sub", [1], [2], r) == [r - 1]
    assert V.ref_op("mul", [r - 1], [r - 1], r) == [1]
    assert V.ref_lincomb(3, [[1, 2, 3], [10, 20, 30]], [3, 1], [2, r - 1], r) == [(2 - 10) % r, 4, 6]
    # the closed forms of the case tables
    for n in V.PREFIX_NS:
        marks = V.prefix_marks(n)
        assert set(marks) == {p for p in (0, 31, 32, 1023, 1024, 32767, 32768, n - 2, n - 1) if 0 <= p < n}
        cases = V.prefix_cases(n, r)
        assert [c.label for c in cases] == ["random", "ones", "minus-ones"] + \
            [f"{kind}@{p}" for p in marks for kind in ("non-one", "zero")]
        for c in cases:
            assert len(c.a) == n and c.want == V.ref_prefix(c.a, r), (n, c.label)
            if c.label.startswith("non-one@"):
                p = int(c.label[8:])
                assert [i for i, x in enumerate(c.a) if x != 1] == [p] and c.a[p] not in (0, 1, r - 1)
                assert set(c.want[:p + 1]) == {1} and set(c.want[p + 1:]) <= {c.a[p]}
            if c.label.startswith("zero@"):
                p = int(c.label[5:])
                assert [i for i, x in enumerate(c.a) if x == 0] == [p] and 0 not in c.want[:p + 1]
                assert not any(c.want[p + 1:])
    for n in V.POWERS_NS:
        cases = V.powers_cases(n, r)
        assert len(cases) == 9
        for c, (label, s, c0) in zip(cases, V.powers_scalars(r)):
            assert c.label == label and c.want == V.ref_mul_powers(c.a, s, c0, r), (n, label)
    pairs = {(s, c0) for _, s, c0 in V.powers_scalars(r)}
    rs = [s for _, s, _ in V.powers_scalars(r) if s not in (0, 1, r - 1, w)]
    rc = [c for _, _, c in V.powers_scalars(r) if c not in (0, 1, r - 1)]
    assert len(set(rs)) == len(set(rc)) == 1 and len(pairs) == 9
    assert {(s, rc[0]) for s in (0, 1, r - 1, w, rs[0])} | {(rs[0], c) for c in (0, 1, r - 1)} | {(0, 0)} == pairs
    # the x^n vector of the prover: s of order 4 gives a cycle of four values times a[i] c0
    cyc = [c for c in V.powers_cases(8193, r) if c.label.startswith("s=i,")][0]
    assert all(cyc.want[i] * cyc.a[i + 4] % r == cyc.want[i + 4] * cyc.a[i] % r for i in range(0, 8189, 97))


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_the_inverse_expectations_are_the_definition(field):
    """every case of every size but the largest against pow(x, -1, r) afresh; the largest on the rows that differ from
    the shared random vector, whose inverses the test above proves by x * inv(x) == 1 on a sample and this one in full"""
    r = FIELDS[field]
    a = V.base_vector(r, V.MAX_N)
    base = V.inverse_cases(V.MAX_N, r)[0]
    assert base.label == "random" and base.a == a and all(x * y % r == 1 for x, y in zip(a, base.want))
    for n in V.INVERSE_NS:
        for c in V.inverse_cases(n, r):
            if c.label in ("random", "zeros", "minus-ones") or c.label.startswith("one-non-zero"):
                assert all((x * y % r == 1) if x else y == 0 for x, y in zip(c.a, c.want)), (n, c.label)
                if c.label.startswith("one-non-zero"):
                    assert sum(1 for x in c.a if x) == 1
            else:                                               # the random vector with zeros put in
                assert all((x == a[i] and y == base.want[i]) if x else y == 0
                           for i, (x, y) in enumerate(zip(c.a, c.want))), (n, c.label)

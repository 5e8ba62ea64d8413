"""The case table of the degree rule (tests/degree_cases.py) against the oracle, and the table against itself: no GPU.

At m <= 8 the oracle runs every case on a real key: O.open_ raises ValueError exactly where the table says `refuse`,
and returns the point the trapdoor expectation gives everywhere else.  The shapes the GPU tests run are then checked for
what makes them worth running: both verdicts in every family, and a range beyond the key (R >= 1) in every accepting
case that is meant to reach the library's check."""
import pytest

import degree_cases as D
from oracle import py_oracle as O

CURVES = D.CURVES


@pytest.mark.parametrize("curve", CURVES)
def test_the_table_says_what_the_oracle_does(curve):
    cv = O.curve(curve)
    tau = D.tau_of(curve)
    keys = {}
    seen = set()
    for case in D.table(curve, small=True):
        assert 0 < case.m <= 8
        ck = keys.setdefault(case.m, O.setup(case.m - 1, tau, cv))
        assert len(ck) == case.m
        want = D.expect(curve, case)
        seen.add((D.family(case), want.verdict))
        if want.verdict == "refuse":
            with pytest.raises(ValueError, match=f"exceeds maximum allowed degree {case.m - 1}$"):
                O.open_(ck, case.polys, case.z, case.xi, cv)
        else:
            point, value = O.open_(ck, case.polys, case.z, case.xi, cv)
            assert value == want.value == O.poly_eval(O.combine(case.polys, case.xi, cv.r), case.z, cv.r), case.label
            assert O.eq(point, O.from_affine(want.point) if want.point else O.Z1(), cv), case.label
    assert seen == {(f, v) for f in D.FAMILIES for v in ("accept", "refuse")}


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_the_table_is_worth_running(curve, small):
    r = O.curve(curve).r
    cases = D.table(curve, small)
    verdicts = {c.label: D.verdict(c, r) for c in cases}
    for f in D.FAMILIES:
        assert {verdicts[c.label] for c in cases if D.family(c) == f} == {"accept", "refuse"}, f
    for c in cases:
        n = D.length(c)
        assert 0 < c.m and n <= D.MAX_N and all(0 <= x < r for p in c.polys for x in p), c.label
        assert 0 <= c.z < r and 0 < c.xi < r
        if verdicts[c.label] == "accept" and D.family(c) in "BDE":
            assert D.beyond(c) >= 1, c.label                  # otherwise it would not reach the kernel
        if D.family(c) == "D":
            assert len(D.stale_poly(curve, c)) == n + D.STALE_EXTRA <= D.MAX_N
    # what the families are for, in the table's own terms
    by = {c.label: c for c in cases}
    for c in cases:
        f, R = D.family(c), D.beyond(c)
        if f == "A":
            assert R in (-1, 0, 1) and verdicts[c.label] == ("refuse" if R == 1 else "accept")
        if f in "BD":
            assert c.polys[0][c.m + 2:] == [0] * (R - 1) and bool(c.polys[0][c.m + 1]) == (verdicts[c.label] == "refuse")
        if f == "C":
            above = [i for i, x in enumerate(c.polys[0]) if x and i > c.m]
            assert len(above) == (0 if c.label.endswith("mirror") else 1) and (c.z, c.xi) == (0, 1)
            assert c.polys[0][c.m] and verdicts[c.label] == ("refuse" if above else "accept")
        if f == "E":
            assert all(len(p) == c.m + 1 + R and p[-1] for p in c.polys[1:]) and len(c.polys) in (2, 17)
            assert verdicts[c.label] == ("accept" if ":cancel:" in c.label else "refuse")
    if not small:
        ranges = {f: {D.beyond(c) for c in cases if D.family(c) == f} for f in "BCE"}
        assert ranges["B"] == {1, 255, 256, 257, 513, 2049} and ranges["C"] == {257, 513} and ranges["E"] == {1, 300}
        assert {c.m for c in cases if D.family(c) == "B"} == {255, 300, 2048}
        words = [by[f"C:R513:word{w}"].polys[0][-1] for w in range(8)]
        assert words == [1 << (32 * w) for w in range(8)]


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_the_open_points_cases(curve, small):
    """family F: both verdicts; the cancelling combination cancels as a whole only (no single point's combination fits
    the key); t = 1 with the weights xi^(i+1) restates the plain opening"""
    cv = O.curve(curve)
    r = cv.r
    seen = set()
    for pc in D.points_table(curve, small):
        want = D.expect_points(curve, pc)
        n = max(len(p) for p in pc.polys)
        assert len(want.quotient) == n - 1 and n - 1 - pc.m >= 1 and n <= D.MAX_N
        seen.add(want.verdict)
        if pc.label.endswith("t4:cancel"):
            assert want.verdict == "accept" and len(pc.points) == 4
            for j, z in enumerate(pc.points):
                one = D.quotient_points(pc.polys, [z], [[row[j]] for row in pc.weights], r)
                assert len(O.poly_normalize(one)) == n - 1 > pc.m
        elif pc.label.endswith("t4:high"):
            assert want.verdict == "refuse"
        else:
            assert want.verdict == "accept"
            assert (want.point is None) == pc.label.endswith("zero-weights")
    assert seen == {"accept", "refuse"}
    for case in D.table(curve, small=True) if small else []:
        if D.family(case) in "BE":
            pc, want = D.as_points(case, r), D.expect(curve, case)
            q = D.quotient_points(pc.polys, pc.points, pc.weights, r)
            assert ("refuse" if len(O.poly_normalize(q)) > pc.m else "accept") == want.verdict
            if want.verdict == "accept":
                assert O.normalize(O.commit_trapdoor(q, D.tau_of(curve), cv), cv) == want.point, case.label

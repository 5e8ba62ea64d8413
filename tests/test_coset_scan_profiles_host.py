"""What tests/test_open_coset_scan_gpu.py covers, pinned on the CPU: the blocked scan of tests/coset_scan_profiles.py
(a restatement of coset_scan_level and its two kernels, csrc/poly.hip) equals the plain suffix recursion the GPU results
are compared with, and the case table reaches every depth, ragged tile, carry edge and launch-grid edge the scan has.
A later edit of the table that drops one of them fails here."""
import os
import random
import re

import pytest

import coset_scan_profiles as P
from oracle import py_oracle as O

FIELDS = {"small": 97, "bls12_381": O.BLS12_381.r, "bn254": O.BN254.r}


def test_the_constants_are_the_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "kzg_snark_amd", "csrc", "poly.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr uint32_t CS_R = (\d+);", src).group(1)) == P.CS_R
    assert int(re.search(r"constexpr uint32_t CS_MAX_LOG_L = (\d+);", src).group(1)) == P.CS_MAX_LOG_L
    for kernel in ("coset_tile_kernel", "coset_fill_kernel"):
        assert re.search(r"__launch_bounds__\(%d\) void %s\(" % (P.BLOCK, kernel), src), kernel


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_the_blocked_scan_is_the_plain_one(field):
    """rows 1 .. 600 (three levels, every raggedness of the two lower ones), l in {1, 2, 4}, the last row holding
    1 .. l coefficients; a in turn random, 0, 1 and r - 1"""
    r = FIELDS[field]
    rng = random.Random(600)
    for rows in range(1, 601):
        for l in (1, 2, 4):
            n = (rows - 1) * l + 1 + rows % l
            assert (n + l - 1) // l == rows
            coeffs = [rng.randrange(r) for _ in range(n)]
            a = (rng.randrange(r), 0, 1, r - 1)[(rows + l) % 4]
            assert P.blocked_divide(coeffs, l, a, r) == P.coset_divide(coeffs, l, a, r), (rows, l)
    assert P.blocked_divide([], 4, 5, r) == P.coset_divide([], 4, 5, r) == ([], [0] * 4)


def test_which_shapes_can_tell_a_wrong_scan():
    """Two wrong scans, to say which shapes a test can catch them at.  a^R enters a consumed value only as
    upper[b + 1] = A[b + 1] + a^R A[b + 2] + ..: with two tiles the one carry read is the last aggregate itself and
    upper[0], where a^R is spent, is read by nobody -- a wrong a^R shows from three tiles on (rows > 2 CS_R), at any
    depth.  A carry dropped where the level above has more than CS_R rows shows exactly from depth 3 on."""
    r = FIELDS["bn254"]
    rng = random.Random(33)
    for rows in list(range(1, 70)) + [255, 256, 257, 272, 273, 511, 512, 513]:
        for l in (1, 2):
            n = (rows - 1) * l + 1
            coeffs = [rng.randrange(1, r) for _ in range(n)]
            a = rng.randrange(2, r - 1)
            good = P.coset_divide(coeffs, l, a, r)
            p = P.plan(n, l.bit_length() - 1)
            assert (P.blocked_divide(coeffs, l, a, r, fault="power") != good) == any(v.tiles >= 3 for v in p.levels)
            assert (P.blocked_divide(coeffs, l, a, r, fault="carry") != good) == (p.depth >= 3), (rows, l)
            assert (rows > 2 * P.CS_R) == any(v.tiles >= 3 for v in p.levels)
    # the table: every case of depth 3 or more has three tiles at some level; of depth 2, those above 2 CS_R rows
    for c in P.cases():
        p = P.plan(c.n, c.log_l)
        assert any(v.tiles >= 3 for v in p.levels) == (p.rows > 2 * P.CS_R)
        assert p.depth < 3 or p.rows > 2 * P.CS_R
    assert sum(P.plan(c.n, c.log_l).depth == 2 and P.plan(c.n, c.log_l).rows > 2 * P.CS_R for c in P.cases()) >= 2


def test_the_definition_is_the_division():
    """q (X^l - a) + rho = p, coefficient by coefficient"""
    r = FIELDS["bn254"]
    rng = random.Random(9)
    for n, l in ((1, 4), (4, 4), (5, 4), (37, 1), (37, 8)):
        p = [rng.randrange(r) for _ in range(n)]
        a = rng.randrange(r)
        q, rho = P.coset_divide(p, l, a, r)
        back = list(rho) + [0] * max(n - l, 0)
        for t, c in enumerate(q):
            back[t + l] = (back[t + l] + c) % r
            back[t] = (back[t] - a * c) % r
        assert back[:n] == p and not any(back[n:]) and len(q) == max(n - l, 0) and len(rho) == l


def test_the_plan_on_cases_worked_by_hand():
    p = P.plan(40, 3)                                         # 5 rows of 8: one tile, one launch of 8 threads
    assert (p.rows, p.depth, p.agg_used, p.quotient_len, p.copied) == (5, 1, 0, 32, 8)
    assert p.agg == 8                                         # reserved by the sum although a single tile writes none
    assert p.launches == (P.Launch("fill", 0, 8, False),)
    assert p.levels[0].ragged and not p.levels[0].carry_absent_last
    p = P.plan(273, 0)                                        # 273 -> 18 -> 2 rows
    assert [(v.rows, v.tiles, v.ragged, v.carry_absent_last) for v in p.levels] == \
        [(273, 18, True, True), (18, 2, True, True), (2, 1, True, False)]
    assert (p.agg, p.agg_used) == (18 + 2 + 1, 18 + 2)
    assert [(x.kernel, x.level, x.threads) for x in p.launches] == \
        [("tile", 0, 18), ("tile", 1, 2), ("fill", 2, 1), ("fill", 1, 2), ("fill", 0, 18)]
    p = P.plan(4096 * 17, 12)                                 # 17 rows of 4096: two tiles
    assert (p.depth, p.agg, p.agg_used) == (2, 3 * 4096, 2 * 4096)
    assert all(x.whole_blocks for x in p.launches)
    p = P.plan(3, 12)                                         # n < l: no quotient, three remainder elements come back
    assert (p.rows, p.depth, p.quotient_len, p.copied) == (1, 1, 0, 3)
    for n, log_l in ((1, 0), (65537, 0), (1 << 17, 12), (1 << 17, 5)):
        p = P.plan(n, log_l)
        assert p.agg_used <= p.agg and len(p.launches) == 2 * p.depth - 1


def test_the_case_table_reaches_every_edge_of_the_scan():
    table = P.cases()
    assert len(table) <= 120                                  # per curve: the GPU test stays at seconds
    assert len({c.label for c in table}) == len(table) == len({(c.log_l, c.n) for c in table})
    assert all(1 <= c.n <= P.MAX_N and 0 <= c.log_l <= P.CS_MAX_LOG_L for c in table)
    plans = {c.label: P.plan(c.n, c.log_l) for c in table}
    # every shape the table is required to hold
    have = {(c.log_l, c.n) for c in table}
    assert {(0, rows) for rows in P.ROWS_L1} <= have
    for log_l, row_counts in P.ROWS_BY_LOG_L.items():
        l = 1 << log_l
        for rows in row_counts:
            assert {(log_l, n) for n in (rows * l, rows * l - 1, (rows - 1) * l + 1) if n} <= have
    assert {(l.bit_length() - 1, n) for l in P.AROUND_L for n in (l - 1, l, l + 1)} <= have
    assert set(P.ROWS_BY_LOG_L) == {1, 3, 8, 12}
    # every depth 1 .. 5, and each of them exact and ragged by one row at the bottom
    assert {p.depth for p in plans.values()} == {1, 2, 3, 4, 5}
    for depth in (1, 2, 3):
        at = [p for p in plans.values() if p.depth == depth and p.l == 1]
        assert any(p.rows == P.CS_R ** depth for p in at) and any(p.rows == P.CS_R ** depth - 1 for p in at), depth
        assert any(q.rows == P.CS_R ** depth + 1 and q.depth == depth + 1 for q in plans.values() if q.l == 1), depth
    assert any(p.rows == P.CS_R ** 4 + 1 and p.depth == 5 and p.levels[-1].rows == 2 for p in plans.values())
    # a ragged tile at every level of a depth-3 and of a depth-4 case
    for depth in (3, 4):
        assert any(p.depth == depth and all(v.ragged for v in p.levels) for p in plans.values()), depth
    # a last tile without a carry beside tiles with one, at the bottom level and at a level that is itself filled from
    # a level above (the carry-absent tile of level i lies below carry-present tiles of level i + 1)
    assert any(p.levels[0].carry_absent_last for p in plans.values())
    assert any(p.depth >= 3 and p.levels[0].carry_absent_last and p.levels[1].carry_absent_last and p.levels[1].tiles > 2
               for p in plans.values())
    # the level above with exactly b + 1 rows for the last tile, and with two tiles only (one carry in the whole level)
    assert any(v.tiles == 2 for p in plans.values() for v in p.levels)
    # launches that are and are not whole blocks of 256 threads, below and above one block
    launches = [x for p in plans.values() for x in p.launches]
    assert any(x.whole_blocks and x.threads == P.BLOCK for x in launches)
    assert any(x.whole_blocks and x.threads > P.BLOCK for x in launches)
    assert any(not x.whole_blocks and x.threads < P.BLOCK for x in launches)
    assert any(not x.whole_blocks and x.threads > P.BLOCK and x.threads % P.BLOCK in (1, 2) for x in launches)
    # both sides of n > l, at every l above one, and the largest l in more than one tile
    for log_l in (1, 3, 8, 12):
        mine = [p for p in plans.values() if p.l == 1 << log_l]
        assert any(p.n < p.l for p in mine) and any(p.n == p.l for p in mine) and any(p.n == p.l + 1 for p in mine)
        assert any(p.copied < p.l for p in mine) and any(p.quotient_len == 1 for p in mine)
    assert any(p.l == 4096 and p.depth == 2 for p in plans.values())
    # the last row full, one short and holding a single coefficient, at a depth-3 shape of every l in {2, 8, 256}
    for log_l in (1, 3, 8):
        l = 1 << log_l
        fill = {p.n - (p.rows - 1) * l for p in plans.values() if p.l == l and p.depth == 3}
        assert {1, l - 1, l} <= fill, log_l

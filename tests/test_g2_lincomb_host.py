"""G2 linear combinations on the CPU: csrc/g2_lincomb.h -- the text the gfx950 kernels of g2_lincomb.hip compile -- built
for the host (tests/shim/g2_lincomb_shim.cpp).  The full addition against curve.Group.add in every exceptional case,
the plan of a call (launches, partial sums, fold levels, 32-bit indices) against its restatement in Python integers, and
the wave sum and the fold restated over the shim's addition against the oracle's sums.  Every comparison is exact."""
import os
import random
import re

import pytest

import g2_lincomb_cases as gl
import g_mul_cases as gm
from g2_bytes_cases import INF2
from kzg_snark_amd import curve as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["kzg_g2_lincomb", "kzg_g2_lincomb_powers"]
# multiples of the point of small prime order q that meet every branch of the addition: 0, +-1, the middle, q - 1, q
SMALL_MULTIPLES = {"bls12_381": list(range(0, 15)), "bn254": [0, 1, 2, 3, 5034, 5035, 10067, 10068, 10069, 10070]}


def test_symbols_are_declared_defined_built_and_listed():
    from kzg_snark_amd import _native, build
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    api = open(os.path.join(ROOT, "kzg_snark_amd", "csrc", "api.hip")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(kzg_ctx\* ctx" % name, header, re.M), name
        assert re.search(r"^int %s\(kzg_ctx\* ctx" % name, api, re.M), name
        assert name in _native.SIGNATURES, name
    assert "g2_lincomb.hip" in build.SOURCES
    from kzg_snark_amd.kzg import KZG
    for method in ("lincomb_g2", "commit_g2"):
        assert callable(getattr(KZG, method)), method
    for method in ("g2_lincomb", "g2_lincomb_powers"):
        assert callable(getattr(_native.Context, method)), method


def test_the_shim_states_the_constants_of_the_python_layer():
    from kzg_snark_amd import _native
    tb, cap, fold_tb, span, limit, _ = gl.consts(gl.build_shim())
    ctx = _native.Context
    assert (tb, cap, fold_tb, span) == (ctx.G2_LINCOMB_LANES, ctx.G2_LINCOMB_LAUNCH_LANES, ctx.G2_LINCOMB_FOLD_LANES,
                                        ctx.G2_LINCOMB_FOLD_SPAN)
    assert tb == gl.WAVE == fold_tb and limit == 1 << 21 and cap % tb == 0 and span % fold_tb == 0


# ---- the full addition ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=gm.CURVES)
def jac(request):
    return gl.Jac(request.param)


def named_points(name):
    pts = {w: pt for pt, w in gm.points(name, 2)}
    small = next(w for w in pts if w.startswith("order "))
    return pts, pts[small], int(small.split()[1])


def check_add(jac, a, b):
    """lift(a) + lift(b) through the shim equals the oracle's a + b"""
    want = jac.G.normalize(jac.G.add(a, b))
    assert jac.affine(jac.add(jac.lift(a), jac.lift(b))) == want
    return want


def test_infinite_operands_equal_points_and_opposite_points(jac):
    G = jac.G
    pts, small, _ = named_points(jac.name)
    Q, R, out = pts["G"], pts["random subgroup point 1"], pts["outside the subgroup"]
    assert check_add(jac, INF2, INF2) == INF2
    for P in (Q, R, out, small):
        assert check_add(jac, INF2, P) == G.normalize(P)
        assert check_add(jac, P, INF2) == G.normalize(P)
        assert check_add(jac, P, P) == G.normalize(G.multiply(P, 2))
        assert check_add(jac, P, G.neg(P)) == INF2
        assert check_add(jac, G.neg(P), P) == INF2
    for a, b in ((Q, R), (R, Q), (Q, out), (out, small), (small, Q)):
        check_add(jac, a, b)


def test_a_point_of_small_order_added_to_its_multiples(jac):
    G = jac.G
    _, t, q = named_points(jac.name)
    assert G.is_inf(G.multiply(t, q)) and not G.is_inf(t)
    seen = set()
    for j in SMALL_MULTIPLES[jac.name]:
        m = G.normalize(G.multiply(t, j))
        seen.add(check_add(jac, t, m))
        check_add(jac, m, t)
        check_add(jac, m, m)
    assert INF2 in seen and G.normalize(G.multiply(t, 2)) in seen


def test_the_same_point_at_another_z_is_still_the_same_point(jac):
    G = jac.G
    pts, small, _ = named_points(jac.name)
    rng = random.Random(0x7a)
    for P in (pts["G"], pts["outside the subgroup"], small):
        a = jac.lift(P)
        b, c = jac.rescale(a, rng.randrange(2, jac.cv.p)), jac.rescale(a, rng.randrange(2, jac.cv.p))
        assert a != b != c and jac.affine(b) == G.normalize(P) == jac.affine(c)
        twice = G.normalize(G.multiply(P, 2))
        for x, y in ((a, b), (b, a), (b, c)):
            assert jac.affine(jac.add(x, y)) == twice                     # recognised as equal: the doubling
        minus = jac.rescale(jac.lift(G.neg(P)), rng.randrange(2, jac.cv.p))
        for x, y in ((a, minus), (minus, b), (c, minus)):
            assert jac.affine(jac.add(x, y)) == INF2                      # recognised as opposite
        R = pts["random subgroup point 2"]
        r2 = jac.rescale(jac.lift(R), rng.randrange(2, jac.cv.p))
        assert jac.affine(jac.add(b, r2)) == G.normalize(G.add(P, R))
        inf_z = jac.lift(INF2)
        assert jac.affine(jac.add(inf_z, b)) == G.normalize(P) == jac.affine(jac.add(b, inf_z))


def test_a_point_that_is_no_point_is_refused_by_the_lift(jac):
    gen = gm.points(jac.name, 2)[1][0]
    off = (gen[0], (gen[1][0] ^ 1, gen[1][1]), (1, 0))
    nw = jac.nw
    out = (gl.U32 * jac.limbs)()
    xy = (gl.U32 * (4 * nw))(*gm.words(gm.to_value(off, 2, nw), 4 * nw))
    assert jac.lib.gl_from_affine(jac.id, xy, 0, out) == 1


# ---- the wave sum and the fold, restated ----------------------------------------------------------------------------------

def test_the_wave_sum_of_64_lanes(jac):
    G = jac.G
    pts, small, q = named_points(jac.name)
    Q = pts["random subgroup point 0"]
    k = 0x1234567
    kQ = G.multiply(Q, k)
    inf = jac.lift(INF2)
    # all equal: a doubling in every round
    assert jac.affine(jac.wave_sum([jac.lift(kQ)] * 64)) == G.normalize(G.multiply(Q, 64 * k))
    # Q, -Q alternating: lanes t and t + s are equal until the last round, which adds 32 Q and -32 Q
    assert jac.affine(jac.wave_sum([jac.lift(Q if t % 2 == 0 else G.neg(Q)) for t in range(64)])) == INF2
    assert jac.affine(jac.wave_sum([inf] * 64)) == INF2
    for lane in (0, 1, 37, 63):
        assert jac.affine(jac.wave_sum([jac.lift(Q) if t == lane else inf for t in range(64)])) == G.normalize(Q)
    # 64 copies of the point of small order, and 64 different points
    assert jac.affine(jac.wave_sum([jac.lift(small)] * 64)) == G.normalize(G.multiply(small, 64 % q))
    lanes = [G.multiply(Q, t + 1) for t in range(64)]
    assert jac.affine(jac.wave_sum([jac.lift(p) for p in lanes])) == G.normalize(G.multiply(Q, 64 * 65 // 2))


def test_the_fold_of_equal_and_of_mixed_partial_sums(jac):
    G = jac.G
    span = gl.consts(jac.lib)[3]
    pts, small, q = named_points(jac.name)
    Q = pts["random subgroup point 0"]
    one = jac.lift(Q)
    for count, levels in ((1, 1), (2, 1), (65, 1), (span, 1), (span + 1, 2), (2 * span + 3, 2)):
        got, depth = jac.fold([one] * count, span)                        # equal partials: doublings in lanes and waves
        assert depth == levels and jac.affine(got) == G.normalize(G.multiply(Q, count))
    mixed = [jac.lift(p) for p in (Q, G.neg(Q), INF2, small, G.multiply(Q, 5))] * 53
    want = G.normalize(G.add(G.multiply(Q, 5 * 53), G.multiply(small, 53 % q)))
    got, depth = jac.fold(mixed, span)
    assert depth == 2 and jac.affine(got) == want


# ---- the plan -------------------------------------------------------------------------------------------------------------

def plan_sizes(tb, cap, span, limit):
    ns = {0, 1, 2, tb - 1, tb, tb + 1, limit - 1, limit}
    ns |= {c * cap + d for c in range(1, limit // cap + 1) for d in (-tb - 1, -tb, -1, 0, 1, tb, tb + 1)}
    ns |= {tb * w + d for w in (tb, span, span + 1, 2 * span, span * tb) for d in (-tb, -1, 0, 1, tb)}
    return sorted(n for n in ns if 0 <= n <= limit)


@pytest.mark.parametrize("name", gm.CURVES)
def test_the_plan_of_every_size_around_the_wave_the_launch_cap_and_the_fold(name):
    lib = gl.build_shim()
    tb, cap, fold_tb, span, limit, max_levels = gl.consts(lib)
    cap_blocks = cap // tb
    limbs = lib.gl_point_limbs(gl.CURVE_IDS[name])
    sizes = plan_sizes(tb, cap, span, limit)
    assert {0, 1, cap, cap + 1, 2 * cap + 1, tb * span + 1, limit} <= set(sizes)
    depths = set()
    for n in sizes:
        p = gl.shim_plan(lib, name, n)
        assert p["ok"], n
        blocks = -(-n // tb)
        assert p["blocks"] == blocks == p["partials"], n
        # the launches cover [0, blocks) once, in order, in whole workgroups, none above the cap, as few as possible
        grids, b0 = [], 0
        while b0 < blocks:
            assert p["launch_blocks"] > 0
            grids.append((b0, min(p["launch_blocks"], blocks - b0)))
            b0 += p["launch_blocks"]
        at = 0
        for b0, grid in grids:
            assert b0 == at and 1 <= grid <= cap_blocks, (n, grids)
            at += grid
        assert at == blocks and len(grids) == -(-blocks // cap_blocks) == p["launches"], (n, grids)
        assert (blocks - 1) * tb < n <= blocks * tb or n == 0
        # the fold
        widths = gl.widths_of(blocks, span)
        assert p["levels"] == max(len(widths) - 1, 0) <= max_levels, n
        assert p["width"][:len(widths)] == widths and not any(p["width"][len(widths):]), (n, p["width"])
        if n:
            assert widths[-1] == 1 and p["levels"] >= 1
        depths.add(p["levels"])
        # indices: the table of the largest launch, every smaller grid of the call, the partial sums, the ping-pong
        if n:
            top = 8 * p["pieces"] * p["launch_blocks"] * tb - 1
            assert p["table_top"] == top < p["vectors"] and top < 1 << 25, n
            for _, grid in grids:
                assert gl.shim_table_top(lib, name, grid) == 8 * p["pieces"] * grid * tb - 1 <= top
            assert blocks * limbs - 1 < p["partial_limbs"] and blocks * limbs < 1 << 32
            for level in range(1, p["levels"]):
                # level `level` reads buffer level & 1 and writes buffer (level + 1) & 1: buffer 0 holds width[0] points,
                # buffer 1 width[1]
                assert widths[level] <= widths[level & 1] and widths[level + 1] <= widths[(level + 1) & 1]
    assert depths == {0, 1, 2}
    assert not gl.shim_plan(lib, name, limit + 1)["ok"]

"""The Shplonk opening on the GPU: kzg_open_points_device and kzg_fr_poly_eval_batch at the edges of
the tile scan, and KZG.open_multi / check_multi, against the plain-Python restatement (tests/multi_restated.py, pinned to
the check equation by tests/test_open_multi_host.py).  Integer work: every comparison is exact.

The code's constants the shapes are chosen from: chunks of 8 coefficients, tiles of T = 2048 (the library's choice when
nothing else runs) or 1024 (`open_tile_threads` = 128), 16 polynomials per combine launch (17 takes two), six products
per Field::dot group, 3 points per launch (5 take two launches), groups of 64 tiles beyond 1024 tiles."""
import random

import numpy as np
import pytest

from oracle import py_oracle as O
from multi_restated import quotient_points, restate_open_multi
from restated import g1_mul

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
KZG_ERR_ARG = -1
TAU = 0x1d0c5eed0badc0ffee1234567
MAX_N = 3 * 2048 + 5


class Env:
    def __init__(self, native, curve):
        self.native, self.curve, self.cv = native, curve, O.curve(curve)
        self.r = self.cv.r
        self.ctx = native.get_context(curve)
        self.tau = TAU % self.r
        self.G1 = O.from_affine(self.cv.g1)
        self.key = self.ctx.srs_generate(native.int_to_words(self.tau), MAX_N)

    def commitment(self, coeffs):
        """[p(tau)] G1 as the library returns a point: affine coordinates, or None for infinity"""
        return O.normalize(g1_mul(self.G1, O.poly_eval(coeffs, self.tau, self.r), self.cv), self.cv)

    def point(self, xy, inf):
        return None if inf[0] else tuple(self.native.limbs_to_ints(xy.reshape(2, self.ctx.fp_limbs)))


@pytest.fixture(scope="module")
def envs(native):
    out = {c: Env(native, c) for c in CURVES}
    yield out
    for e in out.values():
        e.key.close()


def upload(native, polys, extra_rows=0, pad=0):
    """the polynomials as rows of one device array (with `extra_rows` zero rows above them) -> (tensor, lens, stride)"""
    import torch
    stride = max(max((len(p) for p in polys), default=0), 1) + pad
    arr = np.zeros((len(polys) + extra_rows, stride, 4), dtype=np.uint64)
    for i, p in enumerate(polys):
        if p:
            arr[i, :len(p)] = native.ints_to_limbs(p)
    return torch.from_numpy(arr.view(np.int64)).to("cuda:0"), [len(p) for p in polys], stride


def row_ints(native, tensor, row, count):
    import torch
    torch.cuda.synchronize()
    flat = tensor[row, :count].cpu().numpy().view(np.uint64).reshape(count, 4)
    return native.limbs_to_ints(flat) if count else []


def shapes(T):
    """(lens, t, zero point?, zero column?): every length of the issue's list as the longest, k = 1, 3 and 17, t = 1, 2
    and 5, unequal lengths (an empty polynomial and one of a single coefficient among them)"""
    return [
        ([1], 1, False, False),
        ([2, 1, 0], 2, True, False),
        ([8], 5, True, True),
        ([9, 9, 4], 1, False, False),
        ([T - 1, T - 9, 1], 2, False, True),
        ([T], 5, True, False),
        ([T + 1] + [T + 1 - 7 * i for i in range(1, 17)], 2, True, False),
        ([3 * T + 5, 2 * T, 17], 5, False, False),
        ([3 * T + 5 - i for i in range(17)], 1, False, False),
    ]


def make_case(rng, r, lens, t, zero_point, zero_column):
    polys = [[r - 1] * m if i % 3 == 2 else [rng.randrange(r) for _ in range(m)] for i, m in enumerate(lens)]
    points = [rng.randrange(1, r) for _ in range(t)]
    if zero_point:
        points[-1] = 0
    if t >= 3:
        points[1] = points[0]                                    # points may repeat at this level
    weights = [[rng.randrange(r) for _ in range(t)] for _ in lens]
    if len(lens) >= 3:
        weights[1][0] = 0                                        # a zero weight beside non-zero ones
    if zero_column:
        for row in weights:
            row[0] = 0
    return polys, points, weights


@pytest.mark.parametrize("tb", [0, 128])
@pytest.mark.parametrize("curve", CURVES)
def test_open_points_and_eval_batch_at_the_scan_edges(envs, curve, tb):
    """the quotient left in d_quot coefficient by coefficient, the point [q(tau)] G1, and every p_i(z_j) by Horner"""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    T = 1024 if tb == 128 else 2048
    rng = random.Random(77 + tb)
    try:
        ctx.set_tuning("open_tile_threads", tb)
        for lens, t, zero_point, zero_column in shapes(T):
            polys, points, weights = make_case(rng, r, lens, t, zero_point, zero_column)
            k, n = len(polys), max(lens)
            d, dl, stride = upload(native, polys, extra_rows=1, pad=3)
            want = quotient_points(polys, points, weights, r)
            xy, inf = ctx.open_points(env.key, d.data_ptr(), dl, stride, points, weights,
                                      d_quot=d.data_ptr() + k * stride * 32, device=True)
            assert row_ints(native, d, k, n - 1) == want, ("quotient", lens[:3], t)
            assert row_ints(native, d, k, stride)[n - 1:] == [0] * (stride - n + 1), ("beyond the quotient", lens[:3], t)
            assert env.point(xy, inf) == env.commitment(want), ("point", lens[:3], t)
            got = ctx.poly_eval_batch(d.data_ptr(), dl, stride, points)
            assert got == [[O.poly_eval(p, z, r) for z in points] for p in polys], ("values", lens[:3], t)
    finally:
        ctx.set_tuning("open_tile_threads", 0)


@pytest.mark.parametrize("tb", [0, 128])
@pytest.mark.parametrize("curve", CURVES)
def test_open_points_with_a_zero_point_first(envs, curve, tb):
    """z = 0 where shapes() never puts it, in the kernel the plain opening runs too: the call's only point (the fill
    copies the combination and writes), and the first point both of the call and of its second launch of 3 points (there
    the fill copies and adds to what the first launch left).  k = 2, every weight non-zero, so that no point drops out;
    n = 9 ends inside a chunk, n = T + 1 has a second tile of one coefficient.  The quotient coefficient by
    coefficient against the exact restatement."""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    T = 1024 if tb == 128 else 2048
    rng = random.Random(123 + tb)
    try:
        ctx.set_tuning("open_tile_threads", tb)
        for n in (9, T + 1):
            polys = [[rng.randrange(r) for _ in range(n)], [r - 1] * (n - 2)]
            d, dl, stride = upload(native, polys, extra_rows=1, pad=3)
            for t in (1, 4):
                points = [rng.randrange(1, r) for _ in range(t)]
                points[0] = points[-1] = 0
                weights = [[rng.randrange(1, r) for _ in range(t)] for _ in polys]
                want = quotient_points(polys, points, weights, r)
                xy, inf = ctx.open_points(env.key, d.data_ptr(), dl, stride, points, weights,
                                          d_quot=d.data_ptr() + 2 * stride * 32, device=True)
                assert row_ints(native, d, 2, n - 1) == want, ("quotient", n, t)
                assert row_ints(native, d, 2, stride)[n - 1:] == [0] * (stride - n + 1), ("beyond the quotient", n, t)
                assert env.point(xy, inf) == env.commitment(want), ("point", n, t)
    finally:
        ctx.set_tuning("open_tile_threads", 0)


@pytest.mark.parametrize("curve", CURVES)
def test_open_points_host_twin_and_empty_inputs(envs, curve):
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    rng = random.Random(5)
    polys, points, weights = make_case(rng, r, [40, 33, 1], 2, True, False)
    arr = np.zeros((3, 40, 4), dtype=np.uint64)
    for i, p in enumerate(polys):
        arr[i, :len(p)] = native.ints_to_limbs(p)
    xy, inf = ctx.open_points(env.key, arr, [40, 33, 1], 40, points, weights)
    assert env.point(xy, inf) == env.commitment(quotient_points(polys, points, weights, r))
    # every polynomial empty; no polynomials; no points; nothing but zero weights: the point at infinity, values zero
    d, dl, stride = upload(native, [[], [], []], extra_rows=1)
    assert ctx.open_points(env.key, d.data_ptr(), dl, stride, points, weights, device=True)[1][0] == 1
    assert ctx.poly_eval_batch(d.data_ptr(), dl, stride, points) == [[0, 0]] * 3
    d, dl, stride = upload(native, polys, extra_rows=1)
    assert ctx.open_points(env.key, d.data_ptr(), dl, stride, [], [[], [], []], device=True)[1][0] == 1
    xy, inf = ctx.open_points(env.key, d.data_ptr(), dl, stride, points, [[0, 0]] * 3,
                              d_quot=d.data_ptr() + 3 * stride * 32, device=True)
    assert inf[0] == 1 and row_ints(native, d, 3, stride) == [0] * stride
    with pytest.raises(native.NativeError) as e:
        ctx.open_points(env.key, d.data_ptr(), dl, stride, [1] * 65, [[1] * 65] * 3, device=True)
    assert e.value.code == KZG_ERR_ARG
    with pytest.raises(native.NativeError) as e:
        ctx.poly_eval_batch(d.data_ptr(), dl, stride, [1] * 65)
    assert e.value.code == KZG_ERR_ARG


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


def multi_case(rng, r, n):
    """5 polynomials of lengths n, 1, 700 (at most n), 5, n over 4 points, 0 among them: sets of 1 to 4 points, the
    polynomial of one coefficient shorter than its set of two"""
    polys = [[rng.randrange(r) for _ in range(m)] for m in (n, 1, min(700, n), min(5, n), n)]
    z = [rng.randrange(1, r), 0, rng.randrange(1, r), r - 1]
    sets = [[z[0]], [z[1], z[0]], [z[0], z[2], z[3]], [z[3], z[2], z[1], z[0]], [z[2]]]
    return polys, sets


@pytest.mark.parametrize("tb", [0, 128])
@pytest.mark.parametrize("curve", CURVES)
def test_open_multi_against_the_restatement_and_both_pairings(kzgs, curve, tb):
    kzg = kzgs[curve]
    cv, r = O.curve(curve), kzg.curve_order
    T = 1024 if tb == 128 else 2048
    n = T + 1
    rng = random.Random(31 + tb)
    tau = TAU % r
    ck, rk = kzg.setup(n - 1, tau=tau)
    polys, sets = multi_case(rng, r, n)
    gamma, zeta = rng.randrange(1, r), rng.randrange(1, r)
    want = restate_open_multi(polys, sets, gamma, zeta, tau, cv)
    ctx = kzg._context()
    try:
        ctx.set_tuning("open_tile_threads", tb)
        seen = []
        proof = kzg.open_multi(ck, polys, sets, gamma, lambda W: seen.append(W) or zeta)
        assert kzg.evaluate_each(polys[:3], want.T) == [[O.poly_eval(p, z, r) for z in want.T] for p in polys[:3]]
    finally:
        ctx.set_tuning("open_tile_threads", 0)
    assert seen == [proof.W] and proof.zeta == zeta                     # the challenge was asked for with W in hand
    assert proof.evaluations == want.evaluations
    assert kzg.eq(proof.W, want.W) and kzg.eq(proof.W2, want.W2)
    assert kzg.open_multi(ck, polys, sets, gamma, zeta) == proof        # a fixed challenge: the same proof
    comms = kzg.commit(ck, polys)

    def verdict(evals=proof.evaluations, pr=proof, pairing="device", **over):
        return kzg.check_multi(rk, comms, sets, evals, pr, over.get("gamma", gamma), over.get("zeta", zeta),
                               pairing=pairing)

    assert verdict() is True
    if tb == 0:
        assert verdict(pairing="host") is True
    bad = [list(v) for v in proof.evaluations]
    bad[2][1] = (bad[2][1] + 1) % r
    assert verdict(evals=bad) is False
    assert verdict(pr=(proof.W2, proof.W)) is False
    assert verdict(gamma=(gamma + 1) % r) is False
    assert verdict(zeta=(zeta + 1) % r) is False
    off_curve = (proof.W[0], (proof.W[1] + 1) % cv.p, 1)
    assert verdict(pr=(off_curve, proof.W2)) is False
    if tb == 0:
        assert verdict(evals=bad, pairing="host") is False
    # every set [z]: the first proof point is open's
    z = sets[0][0]
    single = kzg.open_multi(ck, polys, [[z]] * len(polys), gamma, zeta)
    assert single.W == kzg.open(ck, polys, z, gamma)
    assert kzg.check_multi(rk, comms, [[z]] * len(polys), single.evaluations, single, gamma, zeta) is True


@pytest.mark.parametrize("curve", CURVES)
def test_open_points_beyond_the_direct_tile_sum(envs, curve):
    """1026 tiles of 1024 (groups of 64 tiles: tile_group_kernel per point), k = 1, t = 2, weights (a, b): the point is
    a open(p, z_1, xi = 1) + b open(p, z_2, xi = 1), formed on the host from the two points the existing opening
    returns"""
    env = envs[curve]
    native, ctx, cv, r = env.native, env.ctx, env.cv, env.r
    n = (1 << 20) + 1025
    rs = np.random.RandomState(11)
    raw = rs.randint(0, 1 << 62, size=(1, n, 4)).astype(np.uint64)
    raw[:, :, 3] >>= np.uint64(3)
    rng = random.Random(12)
    z1, z2, a, b = (rng.randrange(1, r) for _ in range(4))
    import torch
    d = torch.from_numpy(raw.view(np.int64)).to("cuda:0")
    key = ctx.srs_generate(native.int_to_words(env.tau), n - 1)
    try:
        ctx.set_tuning("open_tile_threads", 128)
        parts = []
        for z in (z1, z2):
            xy, inf, _ = ctx.open(key, d.data_ptr(), [n], n, native.int_to_words(z), native.int_to_words(1), device=True)
            parts.append(O.from_affine(env.point(xy, inf)))
        xy, inf = ctx.open_points(key, d.data_ptr(), [n], n, [z1, z2], [[a, b]], device=True)
    finally:
        ctx.set_tuning("open_tile_threads", 0)
        key.close()
    want = O.add(g1_mul(parts[0], a, cv), g1_mul(parts[1], b, cv), cv)
    assert env.point(xy, inf) == O.normalize(want, cv)


@pytest.mark.parametrize("curve", CURVES)
def test_a_held_sharded_slice(envs, curve):
    """kzg_fr_poly_eval_batch works in buffers of its own: finish still works after it.  kzg_open_points_device works
    in the opening's buffers: finish then refuses, as it does after a plain opening."""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    rng = random.Random(3)
    polys = [[rng.randrange(r) for _ in range(m)] for m in (3000, 2500)]
    d, dl, stride = upload(native, polys)
    z, xi = rng.randrange(1, r), rng.randrange(1, r)
    zw, xw, none = native.int_to_words(z), native.int_to_words(xi), native.int_to_words(0)
    ctx.open_shard_begin(d.data_ptr(), dl, stride, zw, xw)
    first = ctx.open_shard_finish(env.key, zw, none, True)
    points = [rng.randrange(1, r), z, 0]
    assert ctx.poly_eval_batch(d.data_ptr(), dl, stride, points) == [[O.poly_eval(p, y, r) for y in points] for p in polys]
    again = ctx.open_shard_finish(env.key, zw, none, True)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    want, _ = O.poly_divide_linear(O.combine(polys, xi, r), z, r)
    assert env.point(again[0], again[1]) == env.commitment(want)
    ctx.open_points(env.key, d.data_ptr(), dl, stride, points, [[1, 2, 3], [4, 5, 6]], device=True)
    with pytest.raises(native.NativeError) as e:
        ctx.open_shard_finish(env.key, zw, none, True)
    assert e.value.code == KZG_ERR_ARG and "another opening" in str(e.value)

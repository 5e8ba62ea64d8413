"""Device vector / polynomial primitives (kzg_fr_*) against Python integers.  Bit-exact."""
import random

import numpy as np
import pytest

from oracle import py_oracle as O

pytestmark = pytest.mark.gpu


def dev(native, vals):
    import torch
    return torch.from_numpy(native.ints_to_limbs(vals).view(np.int64)).to("cuda:0")


def host(native, t):
    return native.limbs_to_ints(t.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 1000, 1025, 40000])
def test_vector_primitives(native, curve, n):
    import torch
    cv = O.curve(curve)
    r = cv.r
    ctx = native.get_context(curve)
    rng = random.Random(n)
    a = [rng.randrange(r) for _ in range(n)]
    b = [rng.randrange(r) for _ in range(n)]
    if n > 2:
        a[1], b[2] = 0, r - 1
    da, db = dev(native, a), dev(native, b)
    out = torch.empty_like(da)
    for op, f in (("add", lambda x, y: (x + y) % r), ("sub", lambda x, y: (x - y) % r), ("mul", lambda x, y: x * y % r)):
        ctx.vec_op(op, n, da.data_ptr(), db.data_ptr(), out.data_ptr())
        ctx.synchronize()
        assert host(native, out) == [f(x, y) for x, y in zip(a, b)], op
    s, c0 = rng.randrange(r), rng.randrange(r)
    ctx.vec_mul_powers(n, da.data_ptr(), s, c0, out.data_ptr())
    ctx.synchronize()
    assert host(native, out) == [x * c0 * pow(s, i, r) % r for i, x in enumerate(a)]
    ctx.vec_inverse(n, da.data_ptr(), out.data_ptr())
    ctx.synchronize()
    assert host(native, out) == [pow(x, -1, r) if x else 0 for x in a]
    inpl = dev(native, a)                                  # in place (out aliases the input); a blocking upload:
                                                           # a clone() would run on torch's stream, not the library's
    ctx.vec_inverse(n, inpl.data_ptr(), inpl.data_ptr())
    ctx.synchronize()
    assert host(native, inpl) == [pow(x, -1, r) if x else 0 for x in a]
    if n >= 33:                                            # zeros in many batches: the batch kernel strides, so the
                                                           # elements 0 .. 32 are the FIRST elements of 33 different
                                                           # threads, never a whole batch of several.  Whole batches
                                                           # of zeros: tests/test_vec_edges_gpu.py, test_inverse_batches
        az = list(a)
        for i in list(range(0, 32)) + [32, n - 1]:
            az[i] = 0
        dz = dev(native, az)
        ctx.vec_inverse(n, dz.data_ptr(), out.data_ptr())
        ctx.synchronize()
        assert host(native, out) == [pow(x, -1, r) if x else 0 for x in az]
    ctx.vec_prefix_product(n, db.data_ptr(), out.data_ptr())
    ctx.synchronize()
    want, acc = [], 1
    for y in b:
        want.append(acc)
        acc = acc * y % r
    assert host(native, out) == want
    z = rng.randrange(r)
    assert ctx.poly_eval(n, da.data_ptr(), z) == O.poly_eval(a, z, r)
    assert ctx.poly_eval(n, da.data_ptr(), 0) == a[0]
    # lincomb of three vectors of different lengths
    c = [rng.randrange(r) for _ in range(max(1, n // 2))]
    dc = dev(native, c)
    sc = [rng.randrange(r), 1, r - 1]
    ctx.vec_lincomb(n, [da.data_ptr(), db.data_ptr(), dc.data_ptr()], [n, n, len(c)], sc, out.data_ptr())
    ctx.synchronize()
    assert host(native, out) == [(sc[0] * a[i] + sc[1] * b[i] + sc[2] * (c[i] if i < len(c) else 0)) % r for i in range(n)]


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_poly_eval_at_the_tile_boundaries(native, curve):
    """kzg_fr_poly_eval = the first tile pass of the opening's scan without its stores + the sum of the tile
    aggregates: lengths around the chunk (8) and tile (2048) sizes and far beyond, z = 0 / 1 / r-1 / random,
    coefficients r-1 / random, also with the aggregates of 64 tiles folded first (`open_direct_tiles` = 1: the path
    polynomials beyond 2^21 coefficients take)."""
    r = O.curve(curve).r
    ctx = native.get_context(curve)
    rng = random.Random(8)
    try:
        for n in (1, 2, 7, 8, 9, 2047, 2048, 2049, 4096, 100001, 300000):
            a = [r - 1] * n if n % 2 == 0 and n < 5000 else [rng.randrange(r) for _ in range(n)]
            da = dev(native, a)
            for z in (0, 1, r - 1, rng.randrange(r)):
                want = O.poly_eval(a, z, r)
                for direct in ((0, 1) if n > 4096 else (0,)):
                    ctx.set_tuning("open_direct_tiles", direct)
                    assert ctx.poly_eval(n, da.data_ptr(), z) == want, (n, z, direct)
    finally:
        ctx.set_tuning("open_direct_tiles", 0)


KZG_ERR_ARG = -1


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("n", [33, 1025])
def test_lincomb_at_the_group_boundaries(native, curve, n):
    """kzg_fr_vec_lincomb sums its terms in groups of DOT_G = 6 that share one Montgomery reduction (dot_upto in
    csrc/poly.hip), up to MAXK = 64 terms: k = 1, 5, 6, 7, 12, 13, 63, 64 -- one short group, one and two full ones,
    full ones followed by a single term, the limit and the limit less one.  Per k two calls against Python integers:
      * mixed: scalars 0, 1, r-1 among random ones; lengths n, n - 1, n / 2, 1 and (from k = 5 on) one 0, so that
        terms drop out of a group at different elements;
      * extremes: every scalar r-1 and every vector r-1 at elements 0, 31, 32 and n-1, all lengths n -- each group,
        the full ones of six included, then reduces the largest sum of products it can meet.
    One term more than MAXK is refused with KZG_ERR_ARG."""
    import torch
    r = O.curve(curve).r
    ctx = native.get_context(curve)
    rng = random.Random(6400 + n)
    kmax = 64
    vecs = [[rng.randrange(r) for _ in range(n)] for _ in range(kmax)]
    for v in vecs[1::3]:
        v[0], v[1], v[n - 1] = r - 1, 0, 1
    top = [list(v) for v in vecs]
    for v in top:
        for i in (0, 31, 32, n - 1):
            v[i] = r - 1
    d_vecs = [dev(native, v) for v in vecs]
    d_top = [dev(native, v) for v in top]
    out = torch.empty_like(d_vecs[0])
    torch.cuda.synchronize()                 # torch's stream wrote them; the context runs on a stream of its own
    len_cycle = [n, n // 2, n - 1, 0, n, 1, n]
    for k in (1, 5, 6, 7, 12, 13, 63, 64):
        lens = [len_cycle[j % len(len_cycle)] for j in range(k)]
        sc = [(0, 1, r - 1, rng.randrange(r), rng.randrange(r))[(j + k) % 5] for j in range(k)]
        ctx.vec_lincomb(n, [d.data_ptr() for d in d_vecs[:k]], lens, sc, out.data_ptr())
        ctx.synchronize()
        want = [sum(sc[j] * vecs[j][i] for j in range(k) if i < lens[j]) % r for i in range(n)]
        assert host(native, out) == want, ("mixed", k)
        ctx.vec_lincomb(n, [d.data_ptr() for d in d_top[:k]], [n] * k, [r - 1] * k, out.data_ptr())
        ctx.synchronize()
        want = [(r - 1) * sum(top[j][i] for j in range(k)) % r for i in range(n)]
        assert host(native, out) == want, ("extremes", k)
    before = host(native, out)
    with pytest.raises(native.NativeError) as e:
        ctx.vec_lincomb(n, [d_vecs[j % kmax].data_ptr() for j in range(kmax + 1)], [n] * (kmax + 1), [1] * (kmax + 1),
                        out.data_ptr())
    assert e.value.code == KZG_ERR_ARG
    ctx.synchronize()
    assert host(native, out) == before

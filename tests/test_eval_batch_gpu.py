"""GPU tests of the batched barycentric evaluation (kzg_fr_eval_lagrange_batch*, csrc/lagrange.hip): b ragged value
vectors over one domain, each at its own point -- in the domain or not -- give the value of the interpolant computed in
Python and what kzg_fr_eval_lagrange gives for that vector alone; a chunk boundary forced by the tuning key and the
device form on the context's stream give the same; argument errors are refused.  Equality of integers."""
import random

import numpy as np
import pytest

from oracle import py_oracle as O

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
KZG_ERR_ARG, KZG_ERR_DEGREE = -1, -4


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


def batch(native, cv, log_n, b, seed):
    """(w, vectors, lens, stride, points, vals uint64[b, stride, 4], z uint64[b, 4]): ragged lengths that include 0 and
    n, stride > n, points drawn from {0, 1 = w^0, w^(n-1), w^(n/2), random} -- several of a batch in the domain"""
    r = cv.r
    n = 1 << log_n
    rng = random.Random(seed)
    w = cv.root_of_unity(n)
    lens = ([n, 0, n // 2 + 1, 1, n - 1] * 2)[:b] if b > 1 else [n]
    special = [pow(w, n - 1, r), 0, pow(w, n // 2, r), 1, rng.randrange(r)]
    zs = [rng.randrange(r)] if b == 1 else (special * 2)[:b]
    vecs = [[rng.randrange(r) for _ in range(m)] for m in lens]
    stride = n + 3
    vals = np.zeros((b, stride, 4), dtype=np.uint64)
    for j, v in enumerate(vecs):
        if v:
            vals[j, :len(v)] = native.ints_to_limbs(v)
        vals[j, len(v):] = np.uint64(0xdead)                               # beyond lens[j]: never read as values
    return w, vecs, lens, stride, zs, vals, native.ints_to_limbs(zs)


def interpolant_at(cv, w, n, vec, z):
    coeffs = O.ifft_ff(list(vec) + [0] * (n - len(vec)), w, cv.r)
    return O.poly_eval(coeffs, z, cv.r)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [1, 3, 8, 12])
def test_every_vector_at_its_own_point(kzgs, native, curve, log_n):
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    n = 1 << log_n
    for b in (1, 2, 5):
        w, vecs, lens, stride, zs, vals, zl = batch(native, cv, log_n, b, 10 * log_n + b)
        out = native.limbs_to_ints(ctx.eval_lagrange_batch(log_n, w, vals, lens, stride, zl))
        d = kzg._upload(ctx, vals)
        for j in range(b):
            assert out[j] == interpolant_at(cv, w, n, vecs[j], zs[j]), (b, j)
            alone = ctx.eval_lagrange(log_n, w, lens[j], d.data_ptr() + j * stride * 32, zs[j])
            assert out[j] == alone, (b, j)
        if b == 5:
            assert out[1] == 0 and out[3] == vecs[3][0]                    # no values; z = w^0 reads value 0


@pytest.mark.parametrize("curve", CURVES)
def test_chunk_boundaries_and_the_device_form(kzgs, native, curve):
    import torch
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    log_n, b = 5, 5
    w, vecs, lens, stride, zs, vals, zl = batch(native, cv, log_n, b, 77)
    want = [interpolant_at(cv, w, 1 << log_n, v, z) for v, z in zip(vecs, zs)]
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        ctx.set_tuning("eval_batch_chunk", 2)                              # chunks of 2, 2 and 1 vectors
        assert native.limbs_to_ints(ctx.eval_lagrange_batch(log_n, w, vals, lens, stride, zl)) == want
        ctx.set_tuning("eval_batch_chunk", 1)
        assert native.limbs_to_ints(ctx.eval_lagrange_batch(log_n, w, vals, lens, stride, zl)) == want
        ms, count = ctx.prof_read("eval_lagrange_batch")
        assert count == 2 and ms > 0                                       # one span per call, whatever the chunks
    finally:
        ctx.set_tuning("eval_batch_chunk", 0)
        ctx.prof_enable(False)
    # the device form: enqueued on the context's stream (here torch's current stream); the caller synchronises once
    # at the end (the second call may itself wait for the first call's copy of its lengths)
    ctx.bind_torch_stream()
    try:
        dev = f"cuda:{ctx.device}"
        d_vals = torch.from_numpy(vals.view(np.int64)).to(dev)
        d_z = torch.from_numpy(zl.view(np.int64)).to(dev)
        d_out = torch.zeros((b, 4), dtype=torch.int64, device=dev)
        for _ in range(2):                                                 # back to back, no synchronise between
            assert ctx.eval_lagrange_batch(log_n, w, d_vals.data_ptr(), lens, stride, d_z.data_ptr(),
                                           d_out=d_out.data_ptr()) is None
        ctx.synchronize()
        got = native.limbs_to_ints(d_out.cpu().numpy().view(np.uint64))
    finally:
        ctx.set_stream(0)
    assert got == want


@pytest.mark.parametrize("curve", CURVES)
def test_argument_errors(kzgs, native, curve):
    kzg, cv = kzgs[curve], O.curve(curve)
    ctx = kzg._context()
    log_n = 3
    w, vecs, lens, stride, zs, vals, zl = batch(native, cv, log_n, 2, 5)

    def code(fn, *a, **k):
        try:
            fn(*a, **k)
        except native.NativeError as e:
            return e.code
        return 0

    assert code(ctx.eval_lagrange_batch, log_n, w, vals, [9, 1], stride, zl) == KZG_ERR_DEGREE
    wide = np.zeros((2, 4, 4), dtype=np.uint64)
    assert code(ctx.eval_lagrange_batch, log_n, w, wide, [5, 1], 4, zl) == KZG_ERR_ARG       # lens[j] > stride
    assert code(ctx.eval_lagrange_batch, log_n, w * w % cv.r, vals, lens, stride, zl) == KZG_ERR_ARG
    assert code(ctx.eval_lagrange_batch, 0, w, vals, lens, stride, zl) == KZG_ERR_ARG
    assert ctx.eval_lagrange_batch(log_n, w, vals[:0], [], stride, zl[:0]).shape == (0, 4)    # b = 0: no work
    out = native.limbs_to_ints(ctx.eval_lagrange_batch(log_n, w, vals, lens, stride, zl))
    assert out == [interpolant_at(cv, w, 8, v, z) for v, z in zip(vecs, zs)]

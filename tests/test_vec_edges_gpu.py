"""The Fr vector primitives (kzg_fr_vec_op, _vec_lincomb, _vec_mul_powers, _vec_inverse, _vec_prefix_product,
kzg_fr_poly_eval) at every level, width, alias and edge of their launch plans: the cases of tests/vec_cases.py (pinned
on the CPU by tests/test_vec_cases_host.py) against Python integers, bit-exact.

Every output is the rows [2, 2 + n) of a tensor of n + 4 rows filled with a pattern that is no field element; the four
rows around it must come back untouched, and so must the input of a call that does not alias."""
import random

import numpy as np
import pytest

import vec_cases as V
from oracle import py_oracle as O

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
GUARD = 2                                                     # rows before and after every output
ROW = 32                                                      # bytes per element: views of whole rows stay 32-byte aligned
SENTINEL = np.array([0xA5C396E15A3C0F1E, 0x5A3C0F1EA5C396E1, 0xC396E15A3C0F1EA5, 0xF0E1D2C3B4A59687], dtype=np.uint64)
assert int.from_bytes(SENTINEL.tobytes(), "little") > 1 << 255          # above both moduli: the image of no element


def dev(native, vals):
    import torch
    return torch.from_numpy(native.ints_to_limbs(vals).view(np.int64)).to("cuda:0")


def host(native, t):
    return native.limbs_to_ints(t.cpu().numpy().view(np.uint64))


class Guarded:
    """n rows on the device between two guard rows on either side; the rows hold `vals` or the sentinel.  Uploaded by
    a blocking copy, so the library's own stream may use it at once."""

    def __init__(self, native, n, vals=None, before=GUARD, after=GUARD):
        import torch
        self.native, self.n, self.before = native, n, before
        rows = np.tile(SENTINEL, (before + n + after, 1))
        if vals is not None and n:
            assert len(vals) == n
            rows[before:before + n] = native.ints_to_limbs(vals)
        self.t = torch.from_numpy(rows.view(np.int64)).to("cuda:0")
        self.ptr = self.t.data_ptr() + ROW * before
        assert self.ptr % ROW == 0

    def read(self):
        """the n rows as integers, after checking every guard row; call after a synchronise"""
        rows = self.t.cpu().numpy().view(np.uint64)
        outside = np.concatenate([rows[:self.before], rows[self.before + self.n:]])
        assert (outside == SENTINEL).all(), "a row outside [0, n) was written"
        return self.native.limbs_to_ints(rows[self.before:self.before + self.n])

    def untouched(self):
        return bool((self.t.cpu().numpy().view(np.uint64) == SENTINEL).all())


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", V.PREFIX_NS)
def test_prefix_product_levels(native, curve, n):
    """one to four levels, each full and one past full; ones around a single other value show exclusivity and which
    chunk every carry comes from, a single zero where the product must die and where it must not yet have"""
    r = O.curve(curve).r
    ctx = native.get_context(curve)
    for c in V.prefix_cases(n, r):
        a, out = Guarded(native, n, c.a), Guarded(native, n)
        ctx.vec_prefix_product(n, a.ptr, out.ptr)
        ctx.synchronize()
        assert out.read() == c.want, c.label
        assert a.read() == c.a, c.label


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", V.INVERSE_NS)
def test_inverse_batches(native, curve, n):
    """the batch kernel (out != a) and the Fermat kernel (in place) on the same inputs: whole batches of zeros, a zero
    first and a zero last in a batch of several, on both sides of the change of the thread count"""
    r = O.curve(curve).r
    ctx = native.get_context(curve)
    for c in V.inverse_cases(n, r):
        a, out = Guarded(native, n, c.a), Guarded(native, n)
        ctx.vec_inverse(n, a.ptr, out.ptr)
        ctx.synchronize()
        assert out.read() == c.want, c.label
        assert a.read() == c.a, c.label
        ctx.vec_inverse(n, a.ptr, a.ptr)
        ctx.synchronize()
        assert a.read() == c.want, ("in place", c.label)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", V.POWERS_NS)
def test_mul_powers_widths(native, curve, n):
    """128, 256 and 512 threads, fewer elements than threads, s and c0 in {0, 1, r - 1}, s of order four"""
    r = O.curve(curve).r
    ctx = native.get_context(curve)
    scalars = V.powers_scalars(r)
    for c, (label, s, c0) in zip(V.powers_cases(n, r), scalars):
        assert c.label == label
        a, out = Guarded(native, n, c.a), Guarded(native, n)
        ctx.vec_mul_powers(n, a.ptr, s, c0, out.ptr)
        ctx.synchronize()
        assert out.read() == c.want, label
        assert a.read() == c.a, label
        ctx.vec_mul_powers(n, a.ptr, s, c0, a.ptr)
        ctx.synchronize()
        assert a.read() == c.want, ("in place", label)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", V.ALIAS_NS)
def test_elementwise_aliasing(native, curve, n):
    """`out` equal to an input of every element-wise call (include/kzg_mi355x.h allows it)"""
    r = O.curve(curve).r
    ctx = native.get_context(curve)
    rng = random.Random(7100 + n)

    def vec():
        return [rng.randrange(r) for _ in range(n)]

    a, b = vec(), vec()
    a[0], b[n - 1] = r - 1, r - 1
    for op in ("add", "sub", "mul"):
        want = V.ref_op(op, a, b, r)
        da, db = Guarded(native, n, a), Guarded(native, n, b)
        ctx.vec_op(op, n, da.ptr, db.ptr, da.ptr)                           # out = a
        ctx.synchronize()
        assert da.read() == want and db.read() == b, (op, "out = a")
        da = Guarded(native, n, a)
        ctx.vec_op(op, n, da.ptr, db.ptr, db.ptr)                           # out = b
        ctx.synchronize()
        assert db.read() == want and da.read() == a, (op, "out = b")
        ctx.vec_op(op, n, da.ptr, da.ptr, da.ptr)                           # a = b = out: 2a, 0, a^2
        ctx.synchronize()
        assert da.read() == V.ref_op(op, a, a, r), (op, "a = b = out")
    assert V.ref_op("sub", a, a, r) == [0] * n

    # one element in the middle of a larger tensor, as DeviceAlgebra.set_entries adds its blinding terms
    p, q = vec(), rng.randrange(r)
    big = [rng.randrange(r) for _ in range(64)]
    big[17] = p[0]
    dbig, dq = Guarded(native, 64, big), Guarded(native, 1, [q])
    ctx.vec_op("add", 1, dbig.ptr + 17 * ROW, dq.ptr, dbig.ptr + 17 * ROW)
    ctx.synchronize()
    got = dbig.read()
    assert got[17] == (big[17] + q) % r and (got[16], got[18]) == (big[16], big[18])
    assert got[:17] == big[:17] and got[18:] == big[18:] and dq.read() == [q]

    # lincomb: out is term 0
    c = vec()
    sc = [rng.randrange(r), r - 1, 1]
    da, db, dc = Guarded(native, n, a), Guarded(native, n, b), Guarded(native, n, c)
    ctx.vec_lincomb(n, [da.ptr, db.ptr, dc.ptr], [n, n, n], sc, da.ptr)
    ctx.synchronize()
    assert da.read() == V.ref_lincomb(n, [a, b, c], [n, n, n], sc, r)
    assert db.read() == b and dc.read() == c

    # lincomb: seven terms, out is the last -- the lone member of the second group of DOT_G
    k = V.DOT_G + 1
    vecs = [vec() for _ in range(k)]
    sc = [rng.randrange(r) for _ in range(k)]
    d = [Guarded(native, n, v) for v in vecs]
    ctx.vec_lincomb(n, [x.ptr for x in d], [n] * k, sc, d[k - 1].ptr)
    ctx.synchronize()
    assert d[k - 1].read() == V.ref_lincomb(n, vecs, [n] * k, sc, r)
    assert [x.read() for x in d[:k - 1]] == vecs[:k - 1]

    # lincomb: one pointer as two terms, out of place and in place
    sc = [rng.randrange(r), rng.randrange(r), r - 1]
    want = V.ref_lincomb(n, [a, b, a], [n, n, n], sc, r)
    da, db, out = Guarded(native, n, a), Guarded(native, n, b), Guarded(native, n)
    ctx.vec_lincomb(n, [da.ptr, db.ptr, da.ptr], [n, n, n], sc, out.ptr)
    ctx.synchronize()
    assert out.read() == want and da.read() == a and db.read() == b
    ctx.vec_lincomb(n, [da.ptr, db.ptr, da.ptr], [n, n, n], sc, da.ptr)
    ctx.synchronize()
    assert da.read() == want and db.read() == b

    # lincomb: out is a term that is shorter than n -- its rows from n / 2 on are read as zero and written by the call
    half = n // 2
    sc = [rng.randrange(r), rng.randrange(r)]
    da, dc = Guarded(native, n, a), Guarded(native, n, c)
    ctx.vec_lincomb(n, [da.ptr, dc.ptr], [n, half], sc, dc.ptr)
    ctx.synchronize()
    want = [(sc[0] * a[i] + (sc[1] * c[i] if i < half else 0)) % r for i in range(n)]
    assert want == V.ref_lincomb(n, [a, c], [n, half], sc, r)
    assert dc.read() == want and da.read() == a

    # mul_powers in place
    s, c0 = rng.randrange(r), rng.randrange(r)
    da = Guarded(native, n, a)
    ctx.vec_mul_powers(n, da.ptr, s, c0, da.ptr)
    ctx.synchronize()
    assert da.read() == V.ref_mul_powers(a, s, c0, r)


def fresh_context(native, curve):
    """a context of its own: its scratch buffers start empty, whatever the shared one has grown to"""
    return native.Context(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_chains_without_a_wait(native, curve):
    """Calls enqueued back to back as the prover enqueues them, one synchronise at the end of each chain.  The prefix
    product and poly_eval share two scratch buffers of the context that either may have to regrow while the other's
    kernels are still queued."""
    r = O.curve(curve).r
    rng = random.Random(7200)

    # the accumulator's shape: ratios by a product, a shift, an inversion, the running product, a combination
    n = 1025
    a = [rng.randrange(1, r) for _ in range(n)]
    b = [rng.randrange(1, r) for _ in range(n)]
    a[1000] = 0                                                # 0 -> 0 in the inversion; the product is zero from 1001 on
    s, c0 = rng.randrange(2, r), rng.randrange(1, r)
    sc = [rng.randrange(r), r - 1, rng.randrange(r)]
    w1 = V.ref_op("mul", a, b, r)
    w2 = V.ref_mul_powers(w1, s, c0, r)
    w3 = V.ref_inverse(w2, r)
    w4 = V.ref_prefix(w3, r)
    w5 = V.ref_lincomb(n, [w4, w3, a], [n, n, n // 2], sc, r)
    assert w3[1000] == 0 and w4[1000] != 0 and not any(w4[1001:]) and any(w5[1001:])
    ctx = fresh_context(native, curve)
    try:
        da, db = Guarded(native, n, a), Guarded(native, n, b)
        t = [Guarded(native, n) for _ in range(5)]
        ctx.vec_op("mul", n, da.ptr, db.ptr, t[0].ptr)
        ctx.vec_mul_powers(n, t[0].ptr, s, c0, t[1].ptr)
        ctx.vec_inverse(n, t[1].ptr, t[2].ptr)
        ctx.vec_prefix_product(n, t[2].ptr, t[3].ptr)
        ctx.vec_lincomb(n, [t[3].ptr, t[2].ptr, da.ptr], [n, n, n // 2], sc, t[4].ptr)
        ctx.synchronize()
        assert [x.read() for x in t] == [w1, w2, w3, w4, w5]
        assert da.read() == a and db.read() == b
    finally:
        ctx.close()

    # a small prefix product, at once a larger one that regrows the scratch, at once one that fits again
    big = V.base_vector(r, 32769)
    ins = [big[100:133], big, big[5000:6024]]
    ctx = fresh_context(native, curve)
    try:
        d_in = [Guarded(native, len(v), v) for v in ins]
        d_out = [Guarded(native, len(v)) for v in ins]
        for x, y in zip(d_in, d_out):
            ctx.vec_prefix_product(x.n, x.ptr, y.ptr)
        ctx.synchronize()
        for v, x, y in zip(ins, d_in, d_out):
            assert y.read() == V.ref_prefix(v, r), len(v)
            assert x.read() == v
    finally:
        ctx.close()

    # a prefix product, at once a poly_eval that needs both scratch buffers at another size
    coeffs = [rng.randrange(r) for _ in range(100001)]
    z = rng.randrange(2, r)
    v = big[7:1032]
    ctx = fresh_context(native, curve)
    try:
        d_c = dev(native, coeffs)
        x, y = Guarded(native, 1025, v), Guarded(native, 1025)
        ctx.vec_prefix_product(1025, x.ptr, y.ptr)
        value = ctx.poly_eval(100001, d_c.data_ptr(), z)       # synchronises
        assert value == O.poly_eval(coeffs, z, r)
        assert y.read() == V.ref_prefix(v, r) and x.read() == v
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_empty_vectors(native, curve):
    """n = 0: every call returns at once and writes nothing"""
    ctx = native.get_context(curve)
    a, b, out = Guarded(native, 0), Guarded(native, 0), Guarded(native, 0)
    for op in ("add", "sub", "mul"):
        ctx.vec_op(op, 0, a.ptr, b.ptr, out.ptr)
    ctx.vec_lincomb(0, [a.ptr, b.ptr], [0, 0], [3, 5], out.ptr)
    ctx.vec_lincomb(0, [], [], [], out.ptr)
    ctx.vec_mul_powers(0, a.ptr, 3, 5, out.ptr)
    ctx.vec_inverse(0, a.ptr, out.ptr)
    ctx.vec_inverse(0, a.ptr, a.ptr)
    ctx.vec_prefix_product(0, a.ptr, out.ptr)
    assert ctx.poly_eval(0, a.ptr, 3) == 0
    assert ctx.poly_eval(0, a.ptr, 0) == 0
    ctx.synchronize()
    assert out.read() == [] and a.read() == [] and b.read() == []
    assert out.untouched() and a.untouched() and b.untouched()

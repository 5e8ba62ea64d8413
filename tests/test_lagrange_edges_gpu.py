"""Evaluation-form KZG (csrc/lagrange.hip) past one pass of its kernels: the cases of tests/lagrange_cases.py (pinned on
the CPU by tests/test_lagrange_cases_host.py) against Python integers and the oracle's group law.  The batched
evaluation at two and four passes of its strided loop and across the grid's y limit, in-domain points past a vector's
end, scratch growth while earlier calls are queued, the single vector at two passes of the 2048-workgroup pass, and the
opening and the key from tau against the definition q_i = (P_i - y)/(w^i - z).  Equality of integers everywhere."""
import functools
import random

import numpy as np
import pytest

import lagrange_cases as L
from oracle import py_oracle as O
from test_vec_edges_gpu import SENTINEL, Guarded

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
KZG_ERR_ARG = -1


def upload(arr):
    """a host array on the device, by a blocking copy: the library's own stream may read it at once"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def pack(native, vecs, stride):
    """uint64[b, stride, 4]: vector j in its first len(vecs[j]) rows, every other row a pattern that is no element"""
    vals = np.tile(SENTINEL, (len(vecs), stride, 1))
    for j, v in enumerate(vecs):
        if v:
            vals[j, :len(v)] = native.ints_to_limbs(v)
    return vals


@functools.lru_cache(maxsize=None)
def batch(curve, name):
    """(log_n, w, vecs, lens, zs, want) of a table of tests/lagrange_cases.py, computed once"""
    cv = O.curve(curve)
    log_n, table, seed = {"13": (L.BATCH13_LOG_N, L.BATCH13_TABLE, 1300), "14": (L.BATCH14_LOG_N, L.BATCH14_TABLE, 1400),
                          "small": (L.SMALL_LOG_N, L.SMALL_TABLE, 300)}[name]
    w = cv.root_of_unity(1 << log_n)
    rows = [(ln, z) for _, ln, z in table]
    vecs, zs, want = L.batch_vectors(rows, log_n, w, cv.r, seed)
    return log_n, w, vecs, [ln for ln, _ in rows], zs, want


class DeviceBatch:
    """the arguments of the device form: values at stride n + 3 with the rows beyond lens[j] poisoned, the points"""

    def __init__(self, native, log_n, vecs, zs):
        self.stride = (1 << log_n) + 3
        self.vals = pack(native, vecs, self.stride)
        self.z = native.ints_to_limbs(zs)
        self.d_vals, self.d_z = upload(self.vals), upload(self.z)

    def run(self, ctx, log_n, w, lens, out):
        assert ctx.eval_lagrange_batch(log_n, w, self.d_vals.data_ptr(), lens, self.stride, self.d_z.data_ptr(),
                                       d_out=out.ptr) is None


# ---- a. the batched pass at two and four passes ----------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("name", ["13", "14"])
def test_batched_evaluation_past_one_pass(native, curve, name):
    """every thread of lagr_batch_sums_kernel adds several terms; the in-domain index in the last lane of the first
    pass, the first and the last of the second, a second pass of one thread and of one workgroup.  In one launch, in
    chunks of 5 and as the device form between guard rows"""
    log_n, w, vecs, lens, zs, want = batch(curve, name)
    table = L.BATCH13_TABLE if name == "13" else L.BATCH14_TABLE
    for j, (_, ln, spec) in enumerate(table):                  # what the in-domain rows are, whatever computed `want`
        if spec[0] == "w":
            assert want[j] == (vecs[j][spec[1]] if spec[1] < ln else 0)
    ctx = native.get_context(curve)
    d = DeviceBatch(native, log_n, vecs, zs)
    assert d.stride > 1 << log_n
    for chunk in (0, L.BATCH_TUNED_CHUNK):
        ctx.set_tuning("eval_batch_chunk", chunk)
        try:
            got = native.limbs_to_ints(ctx.eval_lagrange_batch(log_n, w, d.vals, lens, d.stride, d.z))
            out = Guarded(native, len(lens))
            d.run(ctx, log_n, w, lens, out)
            ctx.synchronize()
        finally:
            ctx.set_tuning("eval_batch_chunk", 0)
        for j, row in enumerate(table):
            assert got[j] == want[j], (chunk, row[0])
        assert out.read() == want, chunk


# ---- b. the grid's y limit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_batch_beyond_the_grids_y_limit(native, curve):
    """b = 65537 vectors over two points: launches of 65535 and 2 vectors, every offset of the chunk loop non-zero"""
    r = O.curve(curve).r
    ctx = native.get_context(curve)
    lens, v0, v1, zs, want = L.ylimit_batch(r, 65537)
    b, stride = L.YLIMIT_B, L.YLIMIT_STRIDE
    for j in list(range(0, b, 4099)) + [65533, 65534, 65535, 65536]:
        assert want[j] == L.ref_barycentric([v0[j], v1[j]][:lens[j]], 2, r - 1, zs[j], r), j
    ln = np.array(lens)
    vals = np.tile(SENTINEL, (b, stride, 1))
    vals[ln >= 1, 0] = native.ints_to_limbs(v0)[ln >= 1]
    vals[ln >= 2, 1] = native.ints_to_limbs(v1)[ln >= 2]
    z = native.ints_to_limbs(zs)
    got = native.limbs_to_ints(ctx.eval_lagrange_batch(L.YLIMIT_LOG_N, r - 1, vals, lens, stride, z))
    wrong = [j for j in range(b) if got[j] != want[j]]
    assert not wrong, (len(wrong), wrong[:8])
    d_vals, d_z, out = upload(vals), upload(z), Guarded(native, b)
    ctx.eval_lagrange_batch(L.YLIMIT_LOG_N, r - 1, d_vals.data_ptr(), lens, stride, d_z.data_ptr(), d_out=out.ptr)
    ctx.synchronize()
    assert out.read() == want


# ---- c. in-domain index past the end, across chunk edges -------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_in_domain_points_past_the_end_of_their_vectors(native, curve):
    """z_j = w^m with m >= lens[j] > 0 is a value read as zero, found by no thread; m = lens[j] - 1 is the last value"""
    cv = O.curve(curve)
    r, log_n = cv.r, L.PAST_LOG_N
    n = 1 << log_n
    w = cv.root_of_unity(n)
    rng = random.Random(500)
    vecs = [[rng.randrange(1, r) for _ in range(ln)] for ln, _ in L.PAST_TABLE]
    lens = [ln for ln, _ in L.PAST_TABLE]
    zs = [pow(w, m, r) for _, m in L.PAST_TABLE]
    want = [v[m] if m < ln else 0 for v, (ln, m) in zip(vecs, L.PAST_TABLE)]
    assert want == [L.ref_barycentric(v, n, w, z, r) for v, z in zip(vecs, zs)]
    ctx = native.get_context(curve)
    d = DeviceBatch(native, log_n, vecs, zs)
    for chunk in (L.PAST_CHUNK, 0):
        ctx.set_tuning("eval_batch_chunk", chunk)
        try:
            got = native.limbs_to_ints(ctx.eval_lagrange_batch(log_n, w, d.vals, lens, d.stride, d.z))
            out = Guarded(native, len(lens))
            d.run(ctx, log_n, w, lens, out)
            ctx.synchronize()
        finally:
            ctx.set_tuning("eval_batch_chunk", 0)
        assert got == want and out.read() == want, chunk


# ---- d. scratch growth with work queued ------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_scratch_growth_while_earlier_calls_are_queued(native, curve):
    """a context of its own (its scratch starts empty): a small call, at once the log_n = 13 call that has to regrow
    the scratch the small call's kernels use, at once the small call again; one synchronise at the end"""
    s_log, s_w, s_vecs, s_lens, s_zs, s_want = batch(curve, "small")
    log_n, w, vecs, lens, zs, want = batch(curve, "13")
    small, big = DeviceBatch(native, s_log, s_vecs, s_zs), DeviceBatch(native, log_n, vecs, zs)
    out1, out2, out3 = Guarded(native, len(s_lens)), Guarded(native, len(lens)), Guarded(native, len(s_lens))
    ctx = native.Context(curve)
    try:
        small.run(ctx, s_log, s_w, s_lens, out1)
        big.run(ctx, log_n, w, lens, out2)
        small.run(ctx, s_log, s_w, s_lens, out3)
        ctx.synchronize()
        assert out1.read() == s_want
        assert out2.read() == want
        assert out3.read() == s_want
    finally:
        ctx.close()


# ---- e. the single vector at 2^19 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_single_vector_at_two_passes(native, curve):
    """kzg_fr_eval_lagrange at n = 2^19: 2048 workgroups, every thread takes two indices; the in-domain value is found
    in the second pass, and a vector of 2^18 + 1 values leaves the second pass one thread with a value"""
    cv = O.curve(curve)
    r, log_n = cv.r, L.SINGLE_LOG_N
    n = 1 << log_n
    w = cv.root_of_unity(n)
    g = np.random.default_rng(19)
    limbs = np.frombuffer(g.bytes(n * 32), dtype=np.uint64).reshape(n, 4).copy()
    limbs[:, 3] >>= np.uint64(4)                               # below 2^252, below both moduli
    for i in (0, (1 << 18) - 1, 1 << 18, n - 1):
        limbs[i] = native.ints_to_limbs([r - 1])[0]
    vals = native.limbs_to_ints(limbs)
    assert len(vals) == n and max(vals) == r - 1
    d = upload(limbs)
    ctx = native.get_context(curve)
    rng = random.Random(19)
    for label, ln, spec in L.SINGLE_TABLE:
        z = L.point(spec, w, r, rng)
        if spec[0] == "random":
            want = L.ref_barycentric(vals[:ln], n, w, z, r)
        else:
            want = vals[spec[1]] if spec[1] < ln else 0
        assert ctx.eval_lagrange(log_n, w, ln, d.data_ptr(), z) == want, label


# ---- f. the opening and the key against the definition ---------------------------------------------------------------
def g1_times(cv, s):
    """[s] G1 as affine (x, y), None for infinity: the oracle's group law"""
    return O.normalize(O.multiply(O.from_affine(cv.g1), s, cv), cv)


def opened(native, ctx, srs, vecs, n, z, xi):
    """(y, proof as (x, y) or None) of kzg_open_evals on host arrays; the rows beyond a vector's length are poisoned"""
    arr = pack(native, vecs, n) if vecs else np.tile(SENTINEL, (1, n, 1))
    xy, inf, ev = ctx.open_evals(srs, arr, [len(v) for v in vecs], n, native.int_to_words(z), native.int_to_words(xi))
    assert inf[0] in (0, 1)
    pt = None if inf[0] else tuple(native.limbs_to_ints(xy.reshape(2, ctx.fp_limbs)))
    return native.limbs_to_ints(ev.reshape(1, 4))[0], pt


def defined(cv, vecs, n, w, z, xi):
    P = L.combine(vecs, [len(v) for v in vecs], xi, n, cv.r)
    y, s = L.proof_scalar(P, n, w, z, TAU % cv.r, cv.r)
    return y, g1_times(cv, s)


@pytest.mark.parametrize("curve", CURVES)
def test_opening_from_values_is_the_definition(native, curve):
    """n = 1024, two ragged vectors, xi != 0: y and [sum_i q_i L_i(tau)] G1 from the quotient's definition on the
    domain, at a random point, at 0 and at w^m in the last lane of a workgroup and the first of the next"""
    cv = O.curve(curve)
    r, n = cv.r, 1 << L.OPEN_LOG_N
    w = cv.root_of_unity(n)
    ctx = native.get_context(curve)
    srs = ctx.srs_generate_lagrange(native.int_to_words(TAU), L.OPEN_LOG_N, w)
    rng = random.Random(1024)
    vecs = [L.random_values(rng, ln, r, [(126, 130), (254, 258)]) for ln in L.OPEN_LENS]
    xi = rng.randrange(1, r)
    for spec in L.OPEN_POINTS:
        z = L.point(spec, w, r, rng)
        y, proof = defined(cv, vecs, n, w, z, xi)
        assert proof is not None
        if spec[0] == "w":                                      # the claimed value is the combination of the values
            m = spec[1]
            assert y == (xi * vecs[0][m] + (xi * xi * vecs[1][m] if m < L.OPEN_LENS[1] else 0)) % r
        assert opened(native, ctx, srs, vecs, n, z, xi) == (y, proof), spec
    srs.close()


@pytest.mark.parametrize("curve", CURVES)
def test_opening_edges_at_n_16(native, curve):
    """constant and zero vectors (quotient zero, proof at infinity), a unit vector at its own point, no vectors, the
    most vectors one call takes and one more"""
    cv = O.curve(curve)
    r, n = cv.r, 16
    w = cv.root_of_unity(n)
    ctx = native.get_context(curve)
    srs = ctx.srs_generate_lagrange(native.int_to_words(TAU), 4, w)
    rng = random.Random(16)
    c, xi, m = rng.randrange(1, r), rng.randrange(1, r), 11
    inside, outside = pow(w, m, r), rng.randrange(r)
    for z in (inside, outside, 0):
        assert opened(native, ctx, srs, [[c] * n], n, z, 1) == (c, None), z
        assert opened(native, ctx, srs, [[c] * n], n, z, xi) == (c * xi % r, None), z
        assert opened(native, ctx, srs, [[0] * n], n, z, xi) == (0, None), z
        assert opened(native, ctx, srs, [], n, z, xi) == (0, None), z          # k = 0
    e_m = [0] * m + [1] + [0] * (n - m - 1)
    for vecs in ([e_m], [e_m[:m + 1]]):
        y, proof = defined(cv, vecs, n, w, inside, 1)
        assert y == 1 and proof is not None
        assert opened(native, ctx, srs, vecs, n, inside, 1) == (1, proof)
    assert opened(native, ctx, srs, [e_m[:m]], n, inside, 1) == (0, None)      # the point past the vector's end
    many = [L.random_values(rng, rng.randrange(0, n + 1), r) for _ in range(L.MAXK)]
    many[0], many[L.MAXK - 1] = L.random_values(rng, n, r), L.random_values(rng, n, r)
    for z in (inside, outside):
        want = defined(cv, many, n, w, z, xi)
        assert want[1] is not None
        assert opened(native, ctx, srs, many, n, z, xi) == want, z              # k = 64
    with pytest.raises(native.NativeError) as e:                                # k = 65
        opened(native, ctx, srs, many + [many[0]], n, outside, xi)
    assert e.value.code == KZG_ERR_ARG
    assert opened(native, ctx, srs, many[:1], n, outside, xi) == defined(cv, many[:1], n, w, outside, xi)
    srs.close()


@pytest.mark.parametrize("curve", CURVES)
def test_key_from_tau_in_the_domain_at_n_1024(native, curve):
    """tau = w^m in the last lane of a workgroup and the first of the next: G1 at m, infinity everywhere else"""
    cv = O.curve(curve)
    r, n = cv.r, 1 << L.OPEN_LOG_N
    w = cv.root_of_unity(n)
    ctx = native.get_context(curve)
    for m in L.KEY_TAU_EXPONENTS:
        assert L.ref_lagrange_scalars(n, w, pow(w, m, r), r) == [0] * m + [1] + [0] * (n - m - 1)
        srs = ctx.srs_generate_lagrange(native.int_to_words(pow(w, m, r)), L.OPEN_LOG_N, w)
        xy, inf = srs.export()
        assert list(np.flatnonzero(inf == 0)) == [m] and set(inf.tolist()) == {0, 1}, m
        assert tuple(native.limbs_to_ints(xy[m].reshape(2, ctx.fp_limbs))) == tuple(cv.g1), m
        srs.close()

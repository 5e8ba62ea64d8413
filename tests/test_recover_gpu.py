"""GPU parity of coset recovery (csrc/recover.hip through the C ABI and the facade): the coefficients recovered from
any K >= n/l cosets equal, bit for bit on canonical limbs, the polynomial the test started with; its evaluations come
from the oracle's transform (oracle.py_oracle at small sizes, c_oracle's at 2^16), and the algebra itself is pinned
against Lagrange interpolation in tests/test_recover_host.py.  The arithmetic is exact: no tolerance anywhere."""
import random

import numpy as np
import pytest

from oracle import c_oracle
from oracle import py_oracle as O
from recover_restated import coset_points, index_set, rng_for

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
SMALL_SHAPES = [(8, 16, 1), (8, 16, 2), (8, 32, 4), (16, 16, 4), (4, 16, 4), (8, 16, 8)]      # (n, N, l)
KZG_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctxs(native):
    made = {c: native.Context(c) for c in CURVES}
    yield made
    for c in made.values():
        c.close()


def log2(v):
    return v.bit_length() - 1


def limbs(native, ints):
    return np.ascontiguousarray(native.ints_to_limbs([int(v) for v in ints])).reshape(-1, 4)


def evaluations(native, curve, coeffs, N, w, big=False):
    """uint64[N, 4]: the polynomial on {w^t}, by the oracle's transform"""
    r = O.curve(curve).r
    if big:
        data = np.zeros((N, 4), dtype=np.uint64)
        data[:len(coeffs)] = coeffs if isinstance(coeffs, np.ndarray) else limbs(native, coeffs)
        return c_oracle.fft(curve, data, w)
    return limbs(native, O.fft_ff(list(coeffs) + [0] * (N - len(coeffs)), w, r))


def cells(ev, idx, l):
    """uint64[K, l, 4]: cell k = the values on coset idx[k], value j at w^(idx[k] + j C)"""
    C = ev.shape[0] // l
    return np.ascontiguousarray(ev.reshape(l, C, 4)[:, np.asarray(idx, dtype=np.int64)].transpose(1, 0, 2))


def recover(ctx, n, N, l, w, idx, vals, b=1):
    return ctx.recover_cosets(log2(n), log2(N), log2(l), w, np.asarray(idx, dtype=np.uint32), vals, b)


def leaf_width(ctx):
    width, have = ctx.prof_read("recover_leaf")
    assert have == 1 and width == int(width) and width >= 1
    return int(width)


# ---- 1. every K at small shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "n%d-N%d-l%d" % s)
def test_every_cell_count_at_small_shapes(native, ctxs, curve, shape):
    n, N, l = shape
    cv, ctx = O.curve(curve), ctxs[curve]
    r, w, C = cv.r, cv.root_of_unity(N), N // l
    rng = rng_for("small", curve, shape)
    p = [rng.randrange(r) for _ in range(n)]
    want, ev = limbs(native, p), evaluations(native, curve, p, N, w)
    for K in range(-(-n // l), C + 1):
        idx = index_set(rng, C, K)
        got, ok = recover(ctx, n, N, l, w, idx, cells(ev, idx, l))
        assert ok.tolist() == [1], (K, idx)
        assert np.array_equal(got[0], want), (K, idx)


# ---- 2. around the leaf width and the tree's levels ---------------------------------------------------------------------
_TREE = {}


def tree_case(native, curve):
    if curve not in _TREE:
        n, N = 1 << 9, 1 << 11
        cv = O.curve(curve)
        rng = rng_for("tree", curve)
        p = [rng.randrange(cv.r) for _ in range(n)]
        w = cv.root_of_unity(N)
        _TREE[curve] = (n, N, w, limbs(native, p), evaluations(native, curve, p, N, w))
    return _TREE[curve]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("arrangement", ["bottom", "top", "random"])
def test_missing_counts_around_the_leaf_and_the_levels(native, ctxs, curve, arrangement):
    ctx = ctxs[curve]
    n, N, w, want, ev = tree_case(native, curve)
    C, leaf = N, leaf_width(ctx)                       # l = 1: up to C - n = 1536 cosets may be missing
    counts = {0, 1, 2, 3, 1535, 1536, leaf - 1, leaf, leaf + 1, 2 * leaf + 1}
    for j in range(5, 11):
        counts |= {(1 << j) - 1, 1 << j, (1 << j) + 1}
    assert max(counts) <= C - n
    rng = rng_for("tree", curve, arrangement)
    for m in sorted(counts):
        if arrangement == "bottom":
            missing = set(range(m))
        elif arrangement == "top":
            missing = set(range(C - m, C))
        else:
            missing = set(rng.sample(range(C), m))
        idx = [i for i in range(C) if i not in missing]
        rng.shuffle(idx)
        got, ok = recover(ctx, n, N, 1, w, idx, cells(ev, idx, 1))
        assert ok.tolist() == [1], m
        assert np.array_equal(got[0], want), m


# ---- 3. value edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_value_edges(native, ctxs, curve):
    n, N, l = 1 << 6, 1 << 7, 4
    cv, ctx = O.curve(curve), ctxs[curve]
    r, w, C = cv.r, cv.root_of_unity(N), N // l
    rng = rng_for("edges", curve)
    polys = [[r - 1] * n, [0] * n, [0] * 17 + [rng.randrange(1, r)] + [0] * (n - 18), [0] * (n - 1) + [rng.randrange(1, r)]]
    idx = index_set(rng, C, C // 2)
    vals = np.stack([cells(evaluations(native, curve, p, N, w), idx, l) for p in polys])
    got, ok = recover(ctx, n, N, l, w, idx, vals, b=len(polys))
    assert ok.tolist() == [1] * len(polys)
    for j, p in enumerate(polys):
        assert np.array_equal(got[j], limbs(native, p)), j


# ---- 4. inconsistency, both directions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_a_changed_value_is_flagged_when_the_cells_overdetermine(native, ctxs, curve):
    n, N, l = 1 << 6, 1 << 7, 4
    cv, ctx = O.curve(curve), ctxs[curve]
    r, w, C = cv.r, cv.root_of_unity(N), N // l
    rng = rng_for("flag", curve)
    polys = [[rng.randrange(r) for _ in range(n)] for _ in range(3)]
    idx = index_set(rng, C, C // 2 + 3)                            # K l > n
    vals = np.stack([cells(evaluations(native, curve, p, N, w), idx, l) for p in polys])
    vals[1, 5, 2, 1] ^= np.uint64(1)                               # one limb of one value of polynomial 1
    got, ok = recover(ctx, n, N, l, w, idx, vals, b=3)
    assert ok.tolist() == [1, 0, 1]
    for j in (0, 2):
        assert np.array_equal(got[j], limbs(native, polys[j])), j


@pytest.mark.parametrize("curve", CURVES)
def test_a_changed_value_is_interpolated_when_the_cells_just_determine(native, ctxs, curve):
    n, N, l = 1 << 6, 1 << 7, 4
    cv, ctx = O.curve(curve), ctxs[curve]
    r, w, C = cv.r, cv.root_of_unity(N), N // l
    rng = rng_for("interp", curve)
    p = [rng.randrange(r) for _ in range(n)]
    idx = index_set(rng, C, n // l)                                # K l = n: every input is consistent
    vals = cells(evaluations(native, curve, p, N, w), idx, l)
    vals[5, 2, 1] ^= np.uint64(1)
    got, ok = recover(ctx, n, N, l, w, idx, vals)
    assert ok.tolist() == [1]
    assert not np.array_equal(got[0], limbs(native, p))
    coeffs = native.limbs_to_ints(got[0])
    given = native.limbs_to_ints(vals.reshape(-1, 4))
    for k, i in enumerate(idx):
        for j, x in enumerate(coset_points(i, l, N, w, r)):
            assert O.poly_eval(coeffs, x, r) == given[k * l + j], (k, j)


# ---- 5. batch and chunks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_chunks_keep_the_batch_in_order(native, curve):
    n, N, l, b = 1 << 8, 1 << 9, 16, 5
    cv = O.curve(curve)
    r, w, C = cv.r, cv.root_of_unity(N), N // l
    rng = rng_for("chunks", curve)
    polys = [[rng.randrange(r) for _ in range(n)] for _ in range(b)]
    idx = index_set(rng, C, C // 2 + 1)
    vals = np.stack([cells(evaluations(native, curve, p, N, w), idx, l) for p in polys])
    want = np.stack([limbs(native, p) for p in polys])
    ctx = native.Context(curve)
    try:
        outs = []
        for chunk in (1, 2, 0):
            ctx.set_tuning("recover_chunk", chunk)
            got, ok = recover(ctx, n, N, l, w, idx, vals, b=b)
            assert ok.tolist() == [1] * b, chunk
            outs.append(got.copy())
        assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want) and np.array_equal(outs[2], want)
        with pytest.raises(native.NativeError):
            ctx.set_tuning("recover_chunk", 1025)
    finally:
        ctx.close()


# ---- 6. the device form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_device_form_on_torch_tensors(native, curve):
    import torch
    n, N, l, b, guard = 1 << 8, 1 << 9, 16, 3, 64
    cv = O.curve(curve)
    r, w, C = cv.r, cv.root_of_unity(N), N // l
    rng = rng_for("device", curve)
    polys = [[rng.randrange(r) for _ in range(n)] for _ in range(b)]
    idx = index_set(rng, C, C // 2 + 2)
    vals = np.stack([cells(evaluations(native, curve, p, N, w), idx, l) for p in polys])
    vals[2, 0, 0, 0] ^= np.uint64(1)
    ctx = native.Context(curve)
    try:
        host, host_ok = recover(ctx, n, N, l, w, idx, vals, b=b)
        stream = torch.cuda.Stream(device="cuda:0")
        ctx.bind_torch_stream(stream)
        with torch.cuda.stream(stream):
            d_vals = torch.from_numpy(vals.view(np.int64)).to("cuda:0")        # on the bound stream: ordered
            d_out = torch.full((b * n + guard, 4), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda:0")
            _, ok = ctx.recover_cosets(log2(n), log2(N), log2(l), w, np.asarray(idx, dtype=np.uint32),
                                       d_vals.data_ptr(), b, d_coeffs=d_out.data_ptr())
            out = d_out.cpu().numpy().view(np.uint64)
        assert ok.tolist() == host_ok.tolist() == [1, 1, 0]
        assert np.array_equal(out[:b * n].reshape(b, n, 4), host)
        assert np.all(out[b * n:] == np.uint64(0x5a5a5a5a5a5a5a5a))
        with pytest.raises(native.NativeError) as e:                            # a misaligned device pointer
            ctx.recover_cosets(log2(n), log2(N), log2(l), w, np.asarray(idx, dtype=np.uint32), d_vals.data_ptr() + 8,
                               b, d_coeffs=d_out.data_ptr())
        assert e.value.code == KZG_ERR_ARG
    finally:
        ctx.close()


# ---- 7. errors ----------------------------------------------------------------------------------------------------------
def raw_call(native, ctx, log_n, log_N, log_l, w, idx, vals, b, out, ok):
    vp = native._as_vp
    idx = np.asarray(idx, dtype=np.uint32)
    return native.lib().kzg_recover_cosets(ctx._h, log_n, log_N, log_l, vp(native.int_to_words(w)), vp(idx), idx.size,
                                           vp(vals), b, vp(out), vp(ok))


@pytest.mark.parametrize("curve", CURVES)
def test_bad_arguments_are_refused_and_the_library_goes_on(native, ctxs, curve):
    n, N, l = 8, 16, 2
    cv, ctx = O.curve(curve), ctxs[curve]
    r, w, C = cv.r, cv.root_of_unity(N), N // l
    rng = rng_for("errors", curve)
    p = [rng.randrange(r) for _ in range(n)]
    ev = evaluations(native, curve, p, N, w)
    good = [0, 3, 5, 6]
    big = np.zeros((1 << 14, 4), dtype=np.uint64)                  # room for whatever a refused call might have read
    out, ok = np.zeros((1 << 14, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint8)
    w22 = 0                                                        # log_N = 22 is refused before w is looked at
    bad = [
        ("K l = n - l", (3, 4, 1, w, good[:3])),
        ("an index = C", (3, 4, 1, w, [0, 3, 5, C])),
        ("a repeated index", (3, 4, 1, w, [0, 3, 5, 3])),
        ("w^2 as the root", (3, 4, 1, w * w % r, good)),
        ("log_l = 13", (13, 14, 13, cv.root_of_unity(1 << 14), [0])),
        ("log_N = 22", (3, 22, 1, w22, good)),
        ("log_n > log_N", (5, 4, 1, w, good + [1, 2, 4, 7])),
    ]
    for what, (log_n, log_N, log_l, root, idx) in bad:
        rc = raw_call(native, ctx, log_n, log_N, log_l, root, idx, big, 1, out, ok)
        assert rc == KZG_ERR_ARG, what
        msg = native.lib().kzg_last_error(ctx._h).decode()
        assert "kzg_recover_cosets" in msg, what
        got, flags = recover(ctx, n, N, l, w, good, cells(ev, good, l))           # the next call works normally
        assert flags.tolist() == [1] and np.array_equal(got[0], limbs(native, p)), what


# ---- 8. round trip with open_cosets and verify_cosets ------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_recovered_cells_and_proofs_equal_the_opened_ones(curve):
    from kzg_snark_amd.kzg import KZG
    kzg = KZG(curve)
    r = kzg.curve_order
    n, N, l, b = 1 << 12, 1 << 13, 64, 4                           # the PeerDAS shape
    C = N // l
    rng = rng_for("roundtrip", curve)
    ck, _ = kzg.setup(n - 1, tau=TAU)
    rk_l = kzg.coset_verification_key(l, TAU)
    polys = [[rng.randrange(r) for _ in range(n)] for _ in range(b)]
    table = kzg.coset_table(ck, n, l)
    proofs, values = kzg.open_cosets_each(table, polys, l, N=N, with_values=True)
    idx = index_set(rng, C, C // 2)
    kept = [[values[j][i] for i in idx] for j in range(b)]
    assert kzg.recover_cosets(idx, kept, l, n, N=N) == polys
    got_proofs, got_values = kzg.recover_cosets_and_open(table, idx, kept, l, N=N)
    assert got_values == values
    assert got_proofs == proofs
    comms = kzg.commit(ck, polys)
    ci = [j for j in range(b) for _ in range(C)]
    ki = [i for _ in range(b) for i in range(C)]
    assert kzg.verify_cosets(ck, rk_l, comms, ci, ki, [v for row in got_values for v in row],
                             [q for row in got_proofs for q in row], l, N, r=0x1234567 ** 7 % r)
    # 64 cells of 64 values just determine 4096 coefficients, so any values are consistent; with a 65th cell a changed
    # value is not, and the facade names the polynomial
    more = idx + [next(i for i in range(C) if i not in idx)]
    bad = [[list(values[j][i]) for i in more] for j in range(b)]
    assert kzg.recover_cosets(more, bad, l, n, N=N) == polys
    bad[2][7][3] = (bad[2][7][3] + 1) % r
    with pytest.raises(ValueError, match="polynomial 2"):
        kzg.recover_cosets(more, bad, l, n, N=N)


# ---- 9. one at size -----------------------------------------------------------------------------------------------------
def test_one_polynomial_at_two_to_the_sixteen(native, ctxs):
    curve = "bls12_381"
    n, N, l = 1 << 16, 1 << 17, 64
    cv, ctx = O.curve(curve), ctxs[curve]
    w, C = cv.root_of_unity(N), N // l
    gen = np.random.default_rng(16)
    want = gen.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    want[:, 3] >>= np.uint64(2)                                    # below 2^252 < r
    ev = evaluations(native, curve, want, N, w, big=True)
    idx = index_set(random.Random(16), C, C // 2)
    got, ok = recover(ctx, n, N, l, w, idx, cells(ev, idx, l))
    assert ok.tolist() == [1]
    assert np.array_equal(got[0], want)


# ---- 10. one profiling span per call -------------------------------------------------------------------------------------
def test_one_span_per_call(native):
    curve = "bn254"
    n, N, l = 8, 16, 2
    cv = O.curve(curve)
    w = cv.root_of_unity(N)
    p = list(range(1, n + 1))
    ev = evaluations(native, curve, p, N, w)
    idx = [7, 0, 2, 5, 4]
    ctx = native.Context(curve)
    try:
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(3):
            got, ok = recover(ctx, n, N, l, w, idx, cells(ev, idx, l))
        assert ok.tolist() == [1] and np.array_equal(got[0], limbs(native, p))
        ms, count = ctx.prof_read("recover_cosets")
        assert count == 3 and ms > 0
        ctx.prof_reset()
        assert ctx.prof_read("recover_cosets") == (0.0, 0)
        recover(ctx, n, N, l, w, idx, cells(ev, idx, l))
        assert ctx.prof_read("recover_cosets")[1] == 1
    finally:
        ctx.prof_enable(False)
        ctx.close()

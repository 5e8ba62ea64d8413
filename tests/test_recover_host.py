"""Coset recovery without a GPU: the algebra of DESIGN.md 4.8 restated in Python integers (recover_restated) equals
direct Lagrange interpolation for every K at small shapes -- the independent statement the GPU tests' expectations rest
on; the product tree's wrap repair in restated form; the facade refuses bad arguments before any native call; the two
new C-ABI symbols are declared, exported and bound; the new kernels fit their budget (resources only; CPU suite)."""
import os
import re
import subprocess

import pytest

from oracle import py_oracle as O
from recover_restated import (GENERATOR, cells_of, coset_points, index_set, lagrange, pair_product, poly_mul, recover,
                              rng_for, vanishing_tree)
from restated import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")
CURVES = ["bls12_381", "bn254"]
SMALL_SHAPES = [(8, 16, 1), (8, 16, 2), (8, 32, 4), (16, 16, 4), (4, 16, 4), (8, 16, 8)]      # (n, N, l)
NEW_SYMBOLS = ["kzg_recover_cosets", "kzg_recover_cosets_device"]
NEW_KERNELS = ["fr_pow_table_kernel", "rec_leaf_kernel", "rec_pair_mul_kernel", "rec_expand_kernel",
               "rec_to_mont_kernel", "rec_scatter_kernel", "rec_shift_kernel", "rec_divide_kernel", "rec_finish_kernel"]


@pytest.fixture(scope="module")
def built():
    from kzg_snark_amd import build
    return build.build(verbose=False)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "n%d-N%d-l%d" % s)
def test_restated_algebra_equals_lagrange_interpolation(curve, shape):
    n, N, l = shape
    cv = O.curve(curve)
    r, w, s = cv.r, cv.root_of_unity(N), GENERATOR[curve]
    assert pow(s, N, r) != 1
    C = N // l
    for K in range(-(-n // l), C + 1):
        rng = rng_for(curve, shape, K)
        idx = index_set(rng, C, K)
        xs = [x for i in idx for x in coset_points(i, l, N, w, r)]
        # a polynomial of degree < n: consistent, and the unique interpolant of degree < K l is p itself
        p = [rng.randrange(r) for _ in range(n)]
        evals = O.fft_ff(p + [0] * (N - n), w, r)
        cells = cells_of(evals, idx, l, N)
        for leaf in (2, 64):                                   # a tree with levels, and the single leaf
            got, ok = recover(idx, cells, l, n, N, w, s, r, leaf=leaf)
            assert ok and got[:n] == p and not any(got[n:])
        ys = [v for cell in cells for v in cell]
        assert lagrange(xs, ys, r) == p + [0] * (K * l - n)
        # arbitrary values: the interpolant of degree < K l, consistent iff its coefficients n .. vanish
        cells = [[rng.randrange(r) for _ in range(l)] for _ in idx]
        want = lagrange(xs, [v for cell in cells for v in cell], r)
        got, ok = recover(idx, cells, l, n, N, w, s, r, leaf=2)
        assert got == want + [0] * (N - K * l)
        assert ok == (not any(want[n:]))
        if K * l == n:
            assert ok                                          # every input is consistent


@pytest.mark.parametrize("curve", CURVES)
def test_wrap_repair_of_the_product_tree(curve):
    r = O.curve(curve).r
    rng = rng_for(curve, "wrap")
    d = 4

    def monic(deg):
        c = [1]
        for _ in range(deg):
            c = poly_mul(c, [rng.randrange(r), 1], r)
        return c
    full_a, full_b, short_a, short_b = monic(d), monic(d), monic(d - 1), monic(1)
    for a, b in ((full_a, full_b), (full_a, short_a), (short_a, short_b), (full_a, [1]), (short_b, [1]), ([1], [1])):
        assert pair_product(a, b, d, r) == poly_mul(a, b, r)
    # only the full pair wraps: without the repair position 0 carries the leading 1 as well
    from recover_restated import cyclic_mul
    wrapped = cyclic_mul(full_a, full_b, 2 * d, r)
    exact = poly_mul(full_a, full_b, r)
    assert wrapped[0] == (exact[0] + 1) % r and wrapped[1:] == exact[1:2 * d] and exact[2 * d] == 1
    # the whole tree, every count around a leaf of 4 and its levels
    for count in list(range(0, 19)) + [31, 32, 33]:
        roots = [rng.randrange(r) for _ in range(count)]
        want = [1]
        for x in roots:
            want = poly_mul(want, [(-x) % r, 1], r)
        assert vanishing_tree(roots, 4, r) == want


@pytest.mark.parametrize("curve", CURVES)
def test_facade_rejects_bad_arguments_before_the_device(curve, monkeypatch):
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG, LagrangeKey

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_native, "get_context", no_device)
    kzg = KZG(curve)
    r = kzg.curve_order
    w16 = int(kzg.Fq.root_of_unity(16))
    cell = [1, 2]
    good_idx, good_vals = [0, 3, 5, 6], [[cell] * 4]                          # n = 8, N = 16, l = 2, C = 8
    bad = [
        dict(coset_indices=[0, 3, 5], values=[[cell] * 3]),                   # K l = n - l
        dict(coset_indices=[0, 3, 5, 8]),                                     # an index = C
        dict(coset_indices=[0, 3, 5, 3]),                                     # a repeated index
        dict(w=w16 * w16 % r),                                                # w^2 as the root
        dict(l=1 << 13, n=1 << 13, N=1 << 14),                                # log_l = 13
        dict(N=1 << 22),                                                      # log_N = 22
        dict(n=32),                                                           # log_n > log_N
        dict(l=3),                                                            # l not a power of two
        dict(n=12),                                                           # n not a power of two
        dict(values=[[cell] * 3]),                                            # cells and indices differ in number
        dict(values=[[[1, 2, 3]] * 4]),                                       # a cell of 3 values for l = 2
        dict(values=[]),                                                      # no polynomial
    ]
    for change in bad:
        args = dict(coset_indices=good_idx, values=good_vals, l=2, n=8, N=16, w=None)
        args.update(change)
        with pytest.raises(ValueError):
            kzg.recover_cosets(**args)
        with pytest.raises(ValueError):
            kzg.recover_cosets_and_open([kzg.G1] * 8, **args)
    with pytest.raises(ValueError):
        kzg.recover_cosets_and_open([kzg.G1] * 4, good_idx, good_vals, 2, n=8, N=16)     # key shorter than n
    with pytest.raises(ValueError):
        kzg.recover_cosets_and_open([kzg.G1] * 8, [0], [[[1] * 8]], 8, n=8, N=16)        # open_cosets needs l <= n/2
    lk = LagrangeKey.__new__(LagrangeKey)
    lk.n, lk.w, lk.log_n = 16, w16, 4
    with pytest.raises(TypeError):
        kzg.recover_cosets_and_open(lk, good_idx, good_vals, 2, n=8, N=16)


def test_new_symbols_are_declared_exported_and_bound(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from kzg_snark_amd import _native
    L = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in exported and sym in _native.SIGNATURES, sym
        assert getattr(L, sym).argtypes == _native.SIGNATURES[sym][1]
    assert _native.MISSING == []
    assert L.kzg_abi_version() == 1                            # symbols were only added
    assert hasattr(_native.Context, "recover_cosets")


def test_new_kernels_fit_their_budget(built):
    out, rows = kernel_resources(built)
    for name in NEW_KERNELS:
        mine = [k for k in rows if name in k[0]]
        assert len(mine) == 2, (name, out)                     # one instantiation per scalar field
        for _, vgpr, agpr, _, lds, scratch in mine:
            assert scratch == 0 and vgpr + agpr <= 256, name
            if name == "rec_leaf_kernel":
                assert 0 < lds <= 64 * 1024

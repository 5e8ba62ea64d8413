"""tests/msm_profiles.py on the CPU: the restated recode is a signed-digit expansion of the scalar, and every case that
tests/test_msm_regimes_gpu.py sends to the device IS in the regime its name says -- measured with profile() on the
finished scalars, never taken from the builder.  A case that misses its regime fails here; the GPU file does not get
to test less in silence."""
import random

import numpy as np
import pytest

import msm_profiles as P
from oracle import py_oracle as O

CASES = [(c, wb) for c in P.CURVES for wb in P.WIDTHS]
ids = [f"{c}-{wb}" for c, wb in CASES]


def test_constants_are_the_ones_the_sources_state():
    """what the regex found, against the relations the kernels rely on (not against retyped numbers)"""
    for wb in P.WIDTHS:
        assert P.NB[wb] == 1 << (P.LO[wb] + P.HI[wb]) and P.NWIN[wb] * wb >= 256 > (P.NWIN[wb] - 1) * wb
        assert P.NB[wb] % (64 // P.FIN[wb]) == 0 and (1 << P.LO[wb]) % P.RC_CH == 0 and (1 << P.HI[wb]) % P.RC_CH == 0
        assert P.TOP_BIT[wb] == 240
    assert P.BPB == P.TPB and P.STAGE_CAP % P.TPB == 0 and P.STAGE_CAP < P.CH2 and P.CH1 % P.TPB == 0
    assert P.HEAVY_NS * max(P.SEG.values()) > 257 and P.NSLOT == 4
    assert P.top_digit_max(O.BN254.r, 16) == 12388 and P.top_digit_max(O.BLS12_381.r, 20) == 29677
    assert P.KEY_POINTS == {16: 1 << 16, 20: 1 << 18}


def extreme_scalars(r, wb):
    """the digit-edge values of test_commit_2_20_with_extreme_coefficients, at this width, and r - 1"""
    nw = P.NWIN[wb]
    out = [r - 1 - i for i in range(64)] + [r - (1 << wb) + i for i in range(64)]
    out += [sum(1 << (wb * j + wb - 1) for j in range(nw)) % r, sum(((1 << wb) - 1) << (wb * j) for j in range(nw)) % r]
    out += [(1 << 255) % r, ((1 << 255) - 1) % r, ((1 << 255) - 19) % r]
    out += [v for v in (1 << 254, (1 << 254) - 1) if v < r]
    out += [1 << (wb * j) for j in range(nw)] + [(1 << (wb * j)) - 1 for j in range(1, nw)]
    out += [1 << (wb * j + wb - 1) for j in range(nw - 1)]
    return out + [0, 1, r - 1]


@pytest.mark.parametrize("curve,wb", CASES, ids=ids)
def test_recode_is_a_signed_digit_expansion(curve, wb):
    r = O.curve(curve).r
    rng = random.Random(wb)
    scalars = [rng.randrange(r) for _ in range(2000)] + extreme_scalars(r, wb)
    half = 1 << (wb - 1)
    arr = P.digits(scalars, wb)
    for i, s in enumerate(scalars):
        ds = P.recode(s, wb)
        assert sum(d << (wb * j) for j, d in ds) == s, hex(s)
        assert all(d != 0 and -half < d <= half for _, d in ds), hex(s)
        assert [(j, int(d)) for j, d in enumerate(arr[i]) if d] == ds, hex(s)      # the array form is the same recode
    assert P.recode(half, wb) == [(0, half)] and P.recode(half + 1, wb) == [(0, -(half - 1)), (1, 1)]
    assert np.array_equal(P.to_limbs(scalars), P.to_limbs(P.to_ints(P.to_limbs(scalars))))
    assert P.to_ints(P.to_limbs(scalars)) == scalars


@pytest.mark.parametrize("curve,wb", CASES, ids=ids)
def test_designed_digits_come_back_from_the_recode(curve, wb):
    """from_digits -> digits is the identity on designed digit matrices, the top bucket's digit included"""
    r = O.curve(curve).r
    rs = np.random.RandomState(wb)
    half, nw = 1 << (wb - 1), P.NWIN[wb]
    d = rs.randint(-half + 1, half, size=(500, nw)).astype(np.int64)
    d[::5, 1::2] = 0
    d[:, nw - 1] = rs.randint(1, P.top_digit_max(r, wb), size=500)      # the top digit: positive, below r's
    d[::7, 3] = half                                                    # digit 2^(wb-1) stays positive
    assert np.array_equal(P.digits(P.from_digits(d, wb, r), wb), d)
    with pytest.raises(AssertionError):
        bad = np.zeros((1, nw), dtype=np.int64)
        bad[0, 2] = -5                                                  # a negative scalar
        P.from_digits(bad, wb, r)
    with pytest.raises(AssertionError):
        bad = np.zeros((1, nw), dtype=np.int64)
        bad[0, nw - 1] = P.top_digit_max(r, wb) + 1                     # >= r
        P.from_digits(bad, wb, r)


@pytest.mark.parametrize("background", [False, True], ids=["sparse", "background"])
@pytest.mark.parametrize("curve,wb", CASES, ids=ids)
def test_edges_case_has_one_bucket_of_every_listed_length(curve, wb, background):
    c = P.edges(curve, wb, background)
    pr = P.profile(c.limbs, wb)
    s, f = P.SEG[wb], P.FIN[wb]
    want = [1, 2, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, f * s, f * s + 1, 254, 255, 256, 257, 64 * s - 1, 64 * s,
            64 * s + 1, 65 * s, 65 * s + 1]
    assert P.HEAVY_NS == 64 and sorted(c.designed.values()) == sorted(want)
    assert {k: int(pr.lengths[k]) for k in c.designed} == c.designed
    assert len({k >> P.LOB for k in c.designed}) == len(want)           # one bin each
    if background:
        assert c.meta["background"] == P.EDGE_BACKGROUND[wb] and len(pr.buckets) > 4 * len(want)
    else:
        assert pr.buckets == c.designed
    # slices: exactly on the edges, and the heavy predicate on both sides of HEAVY_NS
    by_len = {v: k for k, v in c.designed.items()}
    assert [int(pr.ns[by_len[v]]) for v in (s - 1, s, s + 1, 64 * s - 1, 64 * s, 64 * s + 1, 65 * s, 65 * s + 1)] == \
        [1, 1, 2, 64, 64, 65, 65, 66]
    assert int((pr.cls == 0).sum()) < P.HEAVY_RANKS                      # so the ranks of class 0 decide nothing here
    assert sorted(int(pr.lengths[k]) for k in np.nonzero(pr.heavy)[0]) == [64 * s + 1, 65 * s, 65 * s + 1]
    assert [int(pr.cls[by_len[v]]) for v in (1, 254, 255, 257)] == [254, 1, 0, 0]
    assert c.meta["negatives"] > len(want) and pr.windows_used == list(range(P.NWIN[wb]))
    assert 10_000 < c.n < (16_000 if wb == 16 else 40_000)


@pytest.mark.parametrize("curve,wb", CASES, ids=ids)
def test_many_heavy_case_has_more_heavy_buckets_than_heavy_blocks(curve, wb):
    c = P.many_heavy(curve, wb)
    pr = P.profile(c.limbs, wb)
    assert pr.buckets == c.designed and set(pr.buckets) == set(range(P.HEAVY_RANKS + 8))
    assert pr.heavy_candidates >= P.HEAVY_RANKS + 8 and int(pr.heavy.sum()) == P.HEAVY_RANKS
    assert int((pr.cls == 0).sum()) == P.HEAVY_RANKS + 8                 # one class: the order among them is arbitrary
    lens = sorted(pr.buckets.values())
    assert lens[0] > P.HEAVY_NS * P.SEG[wb] and 2.9 < lens[-1] / lens[0] <= 3.01
    assert pr.entries == c.n * P.NWIN[wb] and pr.bins[2:].sum() == 0 and pr.bins[1] > P.CH2
    assert 90 <= -(-int(pr.bins[0]) // P.CH2) + -(-int(pr.bins[1]) // P.CH2) <= 220       # chunks of partition 2
    d = P.digits(c.limbs, wb)
    assert (d < 0).sum() > pr.entries // 3 and (d[:, -1] > 0).all()
    assert c.n < (56_000 if wb == 16 else 135_000)


@pytest.mark.parametrize("curve,wb", CASES, ids=ids)
def test_bin_sizes_case_has_exactly_the_listed_bins(curve, wb):
    c = P.bin_sizes(curve, wb)
    pr = P.profile(c.limbs, wb)
    want = [P.STAGE_CAP, P.STAGE_CAP + 1, P.CH2 - 1, P.CH2, P.CH2 + 1, 2 * P.CH2, 2 * P.CH2 + 1]
    assert [int(v) for v in pr.bins[:2 * len(want)]] == [v for w in want for v in (w, 0)]
    assert pr.bins[2 * len(want):].sum() == 0
    for i in range(len(want)):                                          # spread over all buckets of the bin
        assert (pr.lengths[2 * i * P.BPB:(2 * i + 1) * P.BPB] > 0).all()
    # chunks per bin as prep_bins_kernel cuts them: none (sorted in LDS), then 1, 1, 1, 2, 2, 3
    assert [0 if v <= P.STAGE_CAP else -(-v // P.CH2) for v in want] == [0, 1, 1, 1, 2, 2, 3]
    assert pr.windows_used == list(range(P.NWIN[wb]))


@pytest.mark.parametrize("curve,wb", CASES, ids=ids)
def test_chunk_edge_and_filler_cases(curve, wb):
    assert [P.chunk1_edge(curve, wb, d).n for d in (-1, 0, 1)] == [P.CH1 - 1, P.CH1, P.CH1 + 1]
    assert P.profile(P.zeros_case(curve, wb, 777).limbs, wb).entries == 0
    u = P.uniform_case(curve, wb, 100)
    assert u.n == 100 and P.profile(u.limbs, wb).entries > 90 * P.NWIN[wb]


@pytest.mark.parametrize("curve,wb", CASES, ids=ids)
def test_single_magnitude_cases_occupy_one_bucket(curve, wb):
    lo, hi, half = P.LO[wb], P.HI[wb], 1 << (wb - 1)
    vals = dict(P.matrix_edge_values(wb))
    want = {1, (1 << lo) - 1, 1 << lo, (1 << lo) + 1, P.RC_CH * (1 << lo) - 1, P.RC_CH * (1 << lo),
            ((1 << hi) - 1) << lo, half - 1, half} | {1 << b for b in range(wb)}
    assert set(vals.values()) == want and len(vals) == len(want)
    assert P.top_lengths(wb) == [1, P.SEG[wb] + 1, 64 * P.SEG[wb] + 1]
    windows = set()
    for k, v in enumerate(vals.values()):
        for length in (P.top_lengths(wb) if v >= half - 1 else [1]):
            c = P.single_magnitude(curve, wb, v, length, first=k)
            pr = P.profile(c.limbs, wb)
            assert pr.buckets == {v - 1: length}, (v, length)
            assert (P.digits(c.limbs, wb) >= 0).all()
            assert int(pr.heavy.sum()) == (1 if length > P.HEAVY_NS * P.SEG[wb] else 0)
            windows |= set(pr.windows_used)
    assert windows == set(range(P.NWIN[wb]))
    top = P.single_magnitude(curve, wb, half, 3)
    assert all(d == half for row in P.digits(top.limbs, wb) for d in row if d)      # the top bucket's digit stays positive


@pytest.mark.parametrize("curve,wb", CASES, ids=ids)
def test_repeated_digit_cases(curve, wb):
    for n in (1 << 13, (1 << 13) - 1, 40 * P.SEG[wb], 40 * P.SEG[wb] + 1):
        c = P.repeated_digit(curve, wb, n, (1 << P.LO[wb]) + 3, 2)
        pr = P.profile(c.limbs, wb)
        assert pr.buckets == {(1 << P.LO[wb]) + 2: n} and pr.windows_used == [2]
        assert int(pr.heavy.sum()) == (1 if n >= (1 << 13) - 1 else 0) and int(pr.ns.max()) > P.FIN[wb]

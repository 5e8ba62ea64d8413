"""Scalars DESIGNED to put the commit MSM (csrc/msm_prep.hip, csrc/msm.hip) into one named bucket regime each, and a CPU
restatement of how the device routes them.  Pure Python / numpy: no GPU, no library.

The constants a regime is defined by (slice length, finalize lanes, heavy thresholds, sort-stage capacity, chunk sizes)
are READ from the sources by regex -- a pattern that no longer matches raises at import, it is never replaced by a
retyped number -- so a change of one of them moves the cases with it or fails tests/test_msm_profiles_host.py.

    recode / digits   the signed-digit cut of for_each_digit (msm_prep.hip): one int, or a whole uint64[n, 4] array
    profile           bucket lengths, bin sizes and per-bucket routing (slices, length class, rank, heavy)
    from_digits       designed signed digits -> scalars; asserts 0 <= s < r and the digit bounds that make recode
                      return exactly the designed digits
    builders          edges, many_heavy, bin_sizes, uniform, single_magnitude, repeated_digit -> Case

A designed entry (magnitude d, window j) lands in bucket d-1 with table index j * srs_n + i.  Builders cycle the
windows so that every table stride is used; the top window starts at bit 240 for both widths, so a digit d there
needs d * 2^240 < r."""
import os
import re

import numpy as np

from oracle import py_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_snark_amd", "csrc")
CURVES = ["bls12_381", "bn254"]
WIDTHS = (16, 20)


# ---- constants, from the sources -------------------------------------------------------------------------------------

def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _match(text, pattern, what):
    m = re.search(pattern, text)
    if m is None:
        raise RuntimeError(f"tests/msm_profiles.py: the source no longer states {what} as /{pattern}/")
    return m


_MSM, _PREP = _source("msm.hip"), _source("msm_prep.hip")


def _int(text, pattern, what):
    return int(_match(text, pattern, what).group(1))


def _by_width(name):
    """`NAME = WB >= T ? A : B` of msm.hip's Win -> {16: .., 20: ..}"""
    m = _match(_MSM, r"constexpr uint32_t %s = WB >= (\d+) \? (\d+) : (\d+);" % name, "Win::" + name)
    t, a, b = (int(g) for g in m.groups())
    return {wb: (a if wb >= t else b) for wb in WIDTHS}


SEG = _by_width("SEG")                      # entries per slice (one accumulate lane)
FIN = _by_width("FIN")                      # lanes per bucket in msm_finalize_kernel
_LO_DIV = _int(_MSM, r"constexpr int LO = WB / (\d+);", "Win::LO")
_match(_MSM, r"constexpr int HI = WB - 1 - LO;", "Win::HI")
_match(_MSM, r"constexpr int NWIN = \(256 \+ WB - 1\) / WB;", "Win::NWIN")
_match(_MSM, r"constexpr uint32_t NB = 1u << \(WB - 1\);", "Win::NB")
LO = {wb: wb // _LO_DIV for wb in WIDTHS}   # the bucket matrix has 2^HI rows of 2^LO columns
HI = {wb: wb - 1 - LO[wb] for wb in WIDTHS}
NWIN = {wb: (256 + wb - 1) // wb for wb in WIDTHS}
NB = {wb: 1 << (wb - 1) for wb in WIDTHS}   # bucket k holds digit magnitude k + 1
HEAVY_RANKS = _int(_MSM, r"constexpr uint32_t HEAVY_RANKS = (\d+);", "HEAVY_RANKS")
HEAVY_NS = _int(_MSM, r"constexpr uint32_t HEAVY_NS = (\d+);", "HEAVY_NS")
RC_CH = _int(_MSM, r"constexpr uint32_t RC_CH = (\d+);", "RC_CH")
RC_L2 = _int(_MSM, r"constexpr uint32_t RC_L2 = (\d+);", "RC_L2")
NSLOT = _int(_MSM, r"constexpr int NSLOT = (\d+);", "NSLOT")
_m = _match(_MSM, r"int pick_win_bits\(size_t n\) \{ return n >= \(1u << (\d+)\) \? (\d+) : (\d+); \}", "pick_win_bits")
WIDE_KEY_LOG = int(_m.group(1))             # keys of 2^18 points and more take the wide windows
assert (int(_m.group(3)), int(_m.group(2))) == WIDTHS, "pick_win_bits chooses other widths than the cases are built for"
CH1 = _int(_PREP, r"#define KZG_PREP_CH1 (\d+)", "KZG_PREP_CH1")                  # scalars per partition-1 chunk
CH2 = _int(_PREP, r"#define KZG_PREP_CH2 (\d+)", "KZG_PREP_CH2")                  # entries per partition-2 chunk
STAGE_CAP = _int(_PREP, r"#define KZG_PREP_STAGE_CAP (\d+)", "KZG_PREP_STAGE_CAP")   # entries one workgroup sorts in LDS
TPB = _int(_PREP, r"constexpr uint32_t TPB = (\d+);", "TPB")
LOB = _int(_PREP, r"template <int WB, int LOBV = (\d+)>", "the default LOB of PW")
_match(_PREP, r"if \(win_bits != 20\) return 8;", "lob_for: 8 bucket bits per bin on the 16-bit path")
BPB = 1 << LOB                              # buckets per bin
# 20-bit keys keep LOB = 8 while n * NWIN / NBIN + 4 * 82 <= STAGE_CAP (lob_for): every case here stays below that
_m = _match(_PREP, r"if \(m / \(PW<20>::NB >> lob\) \+ (\d+) \* (\d+) <= STAGE_CAP\) return lob;", "lob_for's bound")
LOB8_MAX_N = {16: None, 20: ((STAGE_CAP - int(_m.group(1)) * int(_m.group(2)) + 1) * (NB[20] >> LOB) - 1) // NWIN[20]}
KEY_POINTS = {16: 1 << (WIDE_KEY_LOG - 2), 20: 1 << WIDE_KEY_LOG}     # the two keys of tests/test_msm_regimes_gpu.py
TOP_BIT = {wb: wb * (NWIN[wb] - 1) for wb in WIDTHS}


def top_digit_max(r, wb):
    """largest d with d * 2^TOP_BIT < r: what a digit of the top window may be"""
    return (r - 1) >> TOP_BIT[wb]


# ---- the recode, restated ----------------------------------------------------------------------------------------------

def recode(s, wb):
    """for_each_digit of msm_prep.hip on one integer: [(window, signed digit)] for the non-zero digits, |d| <= 2^(wb-1).
    A digit equal to 2^(wb-1) stays positive; s < 2^255, so the top digit never wraps."""
    out, carry, half = [], 0, 1 << (wb - 1)
    for j in range(NWIN[wb]):
        d = ((s >> (wb * j)) & ((1 << wb) - 1)) + carry
        if d > half:
            d, carry = d - (1 << wb), 1
        else:
            carry = 0
        if d:
            out.append((j, d))
    assert carry == 0, "the top digit wrapped: s >= 2^255"
    return out


def to_limbs(values):
    """ints (0 <= v < 2^256) -> uint64[n, 4], little-endian"""
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype="<u8").reshape(len(values), 4).copy()


def to_ints(limbs):
    raw = np.ascontiguousarray(limbs, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _as_limbs(scalars):
    if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint64:
        return scalars.reshape(-1, 4)
    return to_limbs(scalars) if len(scalars) else np.zeros((0, 4), dtype=np.uint64)


def digits(scalars, wb):
    """recode of every scalar at once: int64[n, NWIN] signed digits (zero where the digit is zero)"""
    limbs = _as_limbs(scalars)
    n = limbs.shape[0]
    ext = np.concatenate([limbs, np.zeros((n, 1), dtype=np.uint64)], axis=1)
    out = np.zeros((n, NWIN[wb]), dtype=np.int64)
    carry = np.zeros(n, dtype=np.int64)
    half, mask = 1 << (wb - 1), np.uint64((1 << wb) - 1)
    for j in range(NWIN[wb]):
        k, sh = (wb * j) >> 6, (wb * j) & 63
        v = ext[:, k] >> np.uint64(sh)
        if sh + wb > 64:
            v = v | (ext[:, k + 1] << np.uint64(64 - sh))
        d = (v & mask).astype(np.int64) + carry
        neg = d > half
        out[:, j] = np.where(neg, d - (1 << wb), d)
        carry = neg.astype(np.int64)
    assert not carry.any(), "the top digit wrapped: a scalar >= 2^255"
    return out


class Profile:
    """What the device makes of a polynomial.  lengths[k]: entries of bucket k; bins[b]: entries of bin b = k >> LOB;
    ns[k]: slices; cls[k]: length class (buckets of 255 entries and more share class 0 and are unordered among
    themselves: `order` is ONE order the device may produce, ranks inside a class are handed out by atomics);
    heavy[k]: folded by msm_finalize_heavy_kernel under that order; heavy_candidates: buckets with more than HEAVY_NS
    slices, of which the device takes those that land on the first HEAVY_RANKS ranks."""

    def __init__(self, scalars, wb):
        d = digits(scalars, wb)
        mag = np.abs(d[d != 0])
        self.wb = wb
        self.entries = int(mag.size)
        self.lengths = np.bincount(mag - 1, minlength=NB[wb]).astype(np.int64)
        self.bins = self.lengths.reshape(-1, BPB).sum(axis=1)
        self.ns = -(-self.lengths // SEG[wb])
        self.cls = 255 - np.minimum(self.lengths, 255)
        self.order = np.argsort(self.cls, kind="stable")
        rank = np.empty(NB[wb], dtype=np.int64)
        rank[self.order] = np.arange(NB[wb])
        self.rank = rank
        self.heavy = (rank < HEAVY_RANKS) & (self.ns > HEAVY_NS)
        self.heavy_candidates = int((self.ns > HEAVY_NS).sum())
        self.windows_used = sorted(set(np.nonzero(d)[1].tolist()))

    @property
    def buckets(self):
        """{bucket: length} of the non-empty buckets"""
        return {int(k): int(self.lengths[k]) for k in np.nonzero(self.lengths)[0]}


def profile(scalars, wb):
    return Profile(scalars, wb)


# ---- designed digits -> scalars ------------------------------------------------------------------------------------

def from_digits(d, wb, r):
    """int64[n, NWIN] signed digits -> uint64[n, 4] scalars s = sum_j d_j 2^(wb j).  Asserts what makes recode return
    exactly these digits and the library accept the scalar: -2^(wb-1) < d_j <= 2^(wb-1), the top non-zero digit is
    positive (s >= 0) and s < r."""
    d = np.asarray(d, dtype=np.int64)
    n, half = d.shape[0], 1 << (wb - 1)
    assert d.shape[1] == NWIN[wb] and (d <= half).all() and (d > -half).all(), "digit out of range"
    limbs = np.zeros((n, 4), dtype=np.uint64)
    borrow = np.zeros(n, dtype=np.int64)
    for j in range(NWIN[wb]):
        t = d[:, j] + borrow
        neg = t < 0
        u = np.where(neg, t + (1 << wb), t).astype(np.uint64)
        borrow = -neg.astype(np.int64)
        k, sh = (wb * j) >> 6, (wb * j) & 63
        limbs[:, k] |= u << np.uint64(sh)
        if sh + wb > 64:
            spill = u >> np.uint64(64 - sh)
            if k + 1 < 4:
                limbs[:, k + 1] |= spill
            else:
                assert not spill.any(), "scalar >= 2^256"
    assert not borrow.any(), "a scalar's top non-zero digit is negative"
    assert_below(limbs, r)
    return limbs


def assert_below(limbs, r):
    """0 <= s < r for every row"""
    lt = np.zeros(limbs.shape[0], dtype=bool)
    eq = np.ones(limbs.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        rk = np.uint64((r >> (64 * k)) & ((1 << 64) - 1))
        lt |= eq & (limbs[:, k] < rk)
        eq &= limbs[:, k] == rk
    assert lt.all(), "scalar >= r"


def uniform(rs, n, r):
    """n scalars over [0, r), near enough uniform: 255 random bits, the top word folded below r's"""
    raw = rs.randint(0, 1 << 63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2)
    raw += rs.randint(0, 2, size=(n, 4)).astype(np.uint64)
    raw[:, 3] %= np.uint64(r >> 192)
    assert_below(raw, r)
    return raw


class Case:
    """One designed polynomial.  limbs: uint64[n, 4]; designed: {bucket: length} the builder aimed at (checked against
    profile() by the host test, never trusted); exact: no bucket outside `designed` is occupied."""

    def __init__(self, name, curve, wb, limbs, designed, exact, **meta):
        self.name, self.curve, self.wb = name, curve, wb
        self.limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
        self.designed, self.exact, self.meta = designed, exact, meta
        self._ints = None
        assert 0 < self.n < KEY_POINTS[wb], (name, self.n)                 # shorter than its key
        assert LOB8_MAX_N[wb] is None or self.n <= LOB8_MAX_N[wb], (name, self.n)
        assert_below(self.limbs, O.curve(curve).r)

    @property
    def n(self):
        return self.limbs.shape[0]

    @property
    def ints(self):
        if self._ints is None:
            self._ints = to_ints(self.limbs)
        return self._ints

    def label(self):
        return f"{self.curve} / {self.wb}-bit windows / {self.name}"


def _seed(curve, wb, salt):
    return 7919 * salt + 31 * wb + CURVES.index(curve)


def _single_digit_rows(mags, negs, wb, r, first=0):
    """One scalar per designed entry: +d 2^(wb j), or for a negative entry 2^(wb (j+1)) - d 2^(wb j), which recodes as
    -d in window j and +1 in window j+1 (an entry of bucket 0 that the caller has counted).  j cycles over the
    windows: all of them for a positive d that fits the top window, all but the top one otherwise."""
    mags = np.asarray(mags, dtype=np.int64)
    negs = np.asarray(negs, dtype=bool)
    e, nw = mags.size, NWIN[wb]
    c = first + np.arange(e)
    top_ok = ~negs & (mags <= top_digit_max(r, wb))
    j = np.where(top_ok, c % nw, c % (nw - 1))
    d = np.zeros((e, nw), dtype=np.int64)
    rows = np.arange(e)
    d[rows, j] = np.where(negs, -mags, mags)
    d[rows[negs], j[negs] + 1] = 1
    return from_digits(d, wb, r)


def _pack_rows(rs, mags, n, wb, r):
    """Designed magnitudes -> n multi-digit scalars sum_j d_j 2^(wb j): entry e goes to scalar e mod n, in the window
    (e div n + scalar) mod NWIN, so consecutive scalars start in consecutive windows; signs are random, the top
    non-zero digit of every scalar positive.  Every scalar must receive an entry."""
    mags = np.asarray(mags, dtype=np.int64)
    nw, half = NWIN[wb], 1 << (wb - 1)
    assert n <= mags.size <= n * nw and mags.min() >= 1 and mags.max() < min(half, top_digit_max(r, wb))
    mags = mags[rs.permutation(mags.size)]
    e = np.arange(mags.size)
    row = e % n
    col = (e // n + row) % nw
    d = np.zeros((n, nw), dtype=np.int64)
    d[row, col] = np.where(rs.randint(0, 2, size=mags.size) == 1, -mags, mags)
    top = nw - 1 - np.argmax(d[:, ::-1] != 0, axis=1)
    d[np.arange(n), top] = np.abs(d[np.arange(n), top])
    return from_digits(d, wb, r)


# ---- A: slice and class edges --------------------------------------------------------------------------------------

def edge_lengths(wb):
    s, f = SEG[wb], FIN[wb]
    return [1, 2, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, f * s, f * s + 1, 254, 255, 256, 257,
            HEAVY_NS * s - 1, HEAVY_NS * s, HEAVY_NS * s + 1, (HEAVY_NS + 1) * s, (HEAVY_NS + 1) * s + 1]


EDGE_BACKGROUND = {16: 4096, 20: 16384}     # uniform scalars under the designed buckets: ~2 / ~0.4 entries per bucket


def edges(curve, wb, background):
    """One bucket of every length of edge_lengths(wb), in single-digit scalars of both signs.  A negative entry carries
    +1 into the next window, i.e. one entry into bucket 0: bucket 0 is the LAST length of the list and is filled by
    those carries (and positive entries for the rest).  With `background`, uniform scalars lie underneath; what they
    put into a designed bucket is counted, so the lengths stay exact."""
    r = O.curve(curve).r
    rs = np.random.RandomState(_seed(curve, wb, 1 + int(background)))
    lens = edge_lengths(wb)
    bg = uniform(rs, EDGE_BACKGROUND[wb] if background else 0, r)
    have = profile(bg, wb).lengths
    mags, bins = [], {0}
    for length in lens[:-1]:                 # distinct bins, buckets the background left empty, no top bucket
        while True:
            m = int(rs.randint(2, NB[wb]))
            if have[m - 1] == 0 and (m - 1) >> LOB not in bins:
                break
        bins.add((m - 1) >> LOB)
        mags.append(m)
    sink = lens[-1] - int(have[0])
    period = 2                               # every period-th entry of a bucket is negative: as many as bucket 0 takes
    while sum((need - 2) // period + 1 for need in lens[:-1] if need >= 2) > sink:
        period += 1
    m_all = np.repeat(np.array(mags, dtype=np.int64), lens[:-1])
    within = np.concatenate([np.arange(k) for k in lens[:-1]])
    negs = within % period == 1
    direct = sink - int(negs.sum())
    assert direct >= 0
    m_all = np.concatenate([m_all, np.ones(direct, dtype=np.int64)])
    negs = np.concatenate([negs, np.zeros(direct, dtype=bool)])
    mix = rs.permutation(m_all.size)
    limbs = np.concatenate([_single_digit_rows(m_all[mix], negs[mix], wb, r), bg])
    limbs = limbs[rs.permutation(limbs.shape[0])]
    designed = {m - 1: k for m, k in zip(mags, lens[:-1])}
    designed[0] = lens[-1]
    return Case("edges over a uniform background" if background else "edges, sparse", curve, wb, limbs, designed,
                exact=not background, negatives=int(negs.sum()), background=bg.shape[0])


# ---- B: more heavy buckets than heavy blocks -------------------------------------------------------------------------

HEAVY_BUCKETS = HEAVY_RANKS + 8


def many_heavy(curve, wb):
    """Every digit of every scalar is one of HEAVY_BUCKETS magnitudes 1 .. HEAVY_BUCKETS, both signs.  The magnitudes'
    shares are exact, not sampled: weight (K-1)^3 + 2 k^3 for the k-th of K, handed to the magnitudes in a random
    order, so the longest bucket is 3x the shortest; n is the smallest for which the shortest still exceeds
    HEAVY_NS * SEG entries.  All of them are class 0 (unordered), more than HEAVY_RANKS need more than HEAVY_NS
    slices, and all lie in bins 0 and 1."""
    r = O.curve(curve).r
    rs = np.random.RandomState(_seed(curve, wb, 3))
    K, nw = HEAVY_BUCKETS, NWIN[wb]
    w = [(K - 1) ** 3 + 2 * k ** 3 for k in range(K)]
    W = sum(w)
    floor = HEAVY_NS * SEG[wb] + 1
    n = -(-floor * W // (nw * w[0]))
    counts = [n * nw * wk // W for wk in w]
    for k in range(n * nw - sum(counts)):     # the rounding remainder goes to the longest
        counts[K - 1 - k % K] += 1
    assert min(counts) >= floor and sum(counts) == n * nw
    owner = rs.permutation(K) + 1
    mags = np.repeat(owner, counts)
    limbs = _pack_rows(rs, mags, n, wb, r)
    return Case("more heavy buckets than heavy blocks", curve, wb, limbs,
                {int(m) - 1: int(c) for m, c in zip(owner, counts)}, exact=True)


# ---- C: bin sizes for the chunked sort ---------------------------------------------------------------------------------

def bin_size_list():
    return [STAGE_CAP, STAGE_CAP + 1, CH2 - 1, CH2, CH2 + 1, 2 * CH2, 2 * CH2 + 1]


def bin_sizes(curve, wb):
    """Bins 0, 2, 4, ... of exactly bin_size_list() entries (the odd bins between them stay empty), every one of a
    bin's BPB buckets occupied; two designed digits per scalar."""
    r = O.curve(curve).r
    rs = np.random.RandomState(_seed(curve, wb, 4))
    mags = []
    for i, size in enumerate(bin_size_list()):
        inside = np.concatenate([np.arange(BPB), rs.randint(0, BPB, size=size - BPB)])
        mags.append(2 * i * BPB + 1 + inside)
    mags = np.concatenate(mags)
    n = -(-mags.size // 2)
    limbs = _pack_rows(rs, mags, n, wb, r)
    return Case("bins at the edges of the chunked sort", curve, wb, limbs, None, exact=True)


def chunk1_edge(curve, wb, delta):
    """uniform scalars, n = CH1 + delta: one partition-1 chunk less one, exactly one, one and a scalar"""
    r = O.curve(curve).r
    rs = np.random.RandomState(_seed(curve, wb, 6 + delta))
    return Case(f"uniform, n = CH1{delta:+d}" if delta else "uniform, n = CH1", curve, wb, uniform(rs, CH1 + delta, r),
                None, exact=False)


def uniform_case(curve, wb, n, salt=0):
    r = O.curve(curve).r
    return Case(f"{n} uniform scalars", curve, wb, uniform(np.random.RandomState(_seed(curve, wb, 20 + salt)), n, r),
                None, exact=False)


def zeros_case(curve, wb, n):
    """a polynomial of non-zero length whose every digit is zero: no entry at all, the commitment is infinity"""
    return Case(f"{n} zero scalars", curve, wb, np.zeros((n, 4), dtype=np.uint64), {}, exact=True)


# ---- D: one bucket per commit ------------------------------------------------------------------------------------------

def matrix_edge_values(wb):
    """(name, v): digit magnitudes on the row, column and RC_CH edges of the bucket matrix (v = hi 2^LO + lo, bucket
    v - 1), the last bucket below the top one and the top bucket itself, then every single-bit v"""
    lo, hi = LO[wb], HI[wb]
    vals = [("1", 1), ("2^LO-1", (1 << lo) - 1), ("2^LO", 1 << lo), ("2^LO+1", (1 << lo) + 1),
            ("RC_CH*2^LO-1", RC_CH * (1 << lo) - 1), ("RC_CH*2^LO", RC_CH * (1 << lo)),
            ("(2^HI-1)*2^LO", ((1 << hi) - 1) << lo), ("2^(WB-1)-1", (1 << (wb - 1)) - 1),
            ("2^(WB-1), the top bucket", 1 << (wb - 1))]
    seen = {v for _, v in vals}
    vals += [(f"2^{b}", 1 << b) for b in range(wb) if (1 << b) not in seen]
    return vals


def top_lengths(wb):
    return [1, SEG[wb] + 1, HEAVY_NS * SEG[wb] + 1]


def single_magnitude(curve, wb, v, length, first=0):
    """`length` positive single-digit scalars v 2^(wb j), j cycling from `first`, scattered over n = length + 5
    coefficients: bucket v - 1 alone is occupied, so a wrong weight of that bucket cannot be masked"""
    r = O.curve(curve).r
    rs = np.random.RandomState(_seed(curve, wb, 40) + v % 1009 + length)
    n = length + 5
    limbs = np.zeros((n, 4), dtype=np.uint64)
    rows = np.sort(rs.permutation(n)[:length])
    limbs[rows] = _single_digit_rows(np.full(length, v), np.zeros(length, dtype=bool), wb, r, first)
    return Case(f"only digit magnitude v = {v}, {length} entries", curve, wb, limbs, {v - 1: length}, exact=True, v=v)


# ---- E: cancellation inside one bucket -------------------------------------------------------------------------------

def repeated_digit(curve, wb, n, d, j):
    """n copies of the single-digit scalar d 2^(wb j): over a key of alternating G, -G one bucket receives them all"""
    r = O.curve(curve).r
    dd = np.zeros((n, NWIN[wb]), dtype=np.int64)
    dd[:, j] = d
    return Case(f"{n} times the digit {d} in window {j}", curve, wb, from_digits(dd, wb, r), {d - 1: n}, exact=True,
                d=d, j=j)

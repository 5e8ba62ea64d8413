"""The commit MSM (csrc/msm_prep.hip, csrc/msm.hip) at every bucket regime, on both curves and both window widths,
through the C ABI.  Every polynomial is built by tests/msm_profiles.py to sit in ONE named regime -- and proved on the
CPU to sit there by tests/test_msm_profiles_host.py -- at the smallest size that reaches it:

    A  slice and length-class edges (SEG, FIN*SEG, 255, HEAVY_NS*SEG, each -1 / +1), sparse and over a uniform background
    B  more heavy buckets than msm_finalize_heavy_kernel has blocks: ranks 256.. are folded by the FIN lanes
    C  bins of exactly STAGE_CAP, STAGE_CAP+1, CH2-1 .. 2*CH2+1 entries; n = CH1-1, CH1, CH1+1
    D  one occupied bucket per commit: the row, column and RC_CH edges of the bucket matrix, every single-bit digit, the
       top bucket (digit 2^(WB-1)) at 1, SEG+1 and HEAVY_NS*SEG+1 entries
    E  a key of alternating G, -G: P+P, P-P and restarts from infinity inside one bucket, in both finalize kernels
    F  nine polynomials of alternating regimes and widths through the four pipeline slots, no flush in between

Expected values: the trapdoor identity commit = (sum c_i tau^i mod r) G1, one scalar multiplication by the Python
oracle; equality is on the affine integers and the infinity flag.  A failure names curve, width and case."""
import numpy as np
import pytest

import msm_profiles as P
from oracle import py_oracle as O

pytestmark = pytest.mark.gpu

COMBOS = [(c, wb) for c in P.CURVES for wb in P.WIDTHS]
IDS = [f"{c}-{wb}" for c, wb in COMBOS]
TAU = 0x6d736d5f726567696d65735f74617521
DEV = "cuda:0"


class Rig:
    """One curve: a context, the 16-bit key (2^16 points) and the 20-bit key (2^18 points) of one tau, and tau's
    powers.  Built once per module, closed at its end."""

    def __init__(self, native, curve):
        self.native, self.curve, self.cv = native, curve, O.curve(curve)
        self.tau = TAU % self.cv.r
        self.ctx = native.Context(curve)
        self.L = self.ctx.fp_limbs
        self.keys = self.make_keys(self.ctx)
        self.G = O.from_affine(self.cv.g1)
        self.pows = [1] * P.KEY_POINTS[20]
        for i in range(1, len(self.pows)):
            self.pows[i] = self.pows[i - 1] * self.tau % self.cv.r
        self._want = {}

    def make_keys(self, ctx):
        keys = {wb: ctx.srs_generate(self.native.int_to_words(self.tau), P.KEY_POINTS[wb]) for wb in P.WIDTHS}
        assert [keys[wb].n >= (1 << P.WIDE_KEY_LOG) for wb in P.WIDTHS] == [False, True]
        return keys

    def close(self):
        for k in self.keys.values():
            k.close()
        self.ctx.close()

    def multiple_of_g(self, k):
        """(infinity flag, (x, y)) of k G1, as the library reports it: zero words beside the flag"""
        k %= self.cv.r
        return (1, (0, 0)) if k == 0 else (0, tuple(O.normalize(O.multiply(self.G, k, self.cv), self.cv)))

    def want(self, case):
        """the trapdoor value of a case, computed once"""
        key = (case.wb, case.name)
        if key not in self._want:
            self._want[key] = self.multiple_of_g(sum(c * self.pows[i] for i, c in enumerate(case.ints) if c))
        return self._want[key]

    def point(self, xy, inf):
        return int(inf), tuple(self.native.limbs_to_ints(np.asarray(xy).reshape(2, self.L)))

    def commit(self, case, key=None):
        n = case.n
        xy, inf = self.ctx.commit(self.keys[case.wb] if key is None else key, case.limbs.reshape(1, n, 4), [n], n)
        return xy[0].copy(), int(inf[0])

    def check(self, case):
        xy, inf = self.commit(case)
        assert self.point(xy, inf) == self.want(case), case.label()
        return xy, inf


_rigs = {}


@pytest.fixture(scope="module")
def rigs(native):
    def get(curve):
        if curve not in _rigs:
            _rigs[curve] = Rig(native, curve)
        return _rigs[curve]
    yield get
    for r in _rigs.values():
        r.close()
    _rigs.clear()


_built = {}


def built(fn, *args):
    """a case of msm_profiles, built once for the module (F sends A, B and D's polynomials again)"""
    key = (fn.__name__,) + args
    if key not in _built:
        _built[key] = fn(*args)
    return _built[key]


# ---- A ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("background", [False, True], ids=["sparse", "background"])
@pytest.mark.parametrize("curve,wb", COMBOS, ids=IDS)
def test_slice_and_class_edges(rigs, curve, wb, background):
    """one bucket each of 1, 2, SEG-1, SEG, SEG+1, 2SEG-1, 2SEG, 2SEG+1, FIN*SEG, FIN*SEG+1, 254 .. 257, 64*SEG-1,
    64*SEG, 64*SEG+1, 65*SEG, 65*SEG+1 entries of both signs: single-slice buckets, FIN-lane buckets on every slice
    edge, the 255-cap of the length classes, and the heavy predicate from both sides"""
    rigs(curve).check(built(P.edges, curve, wb, background))


# ---- B ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve,wb", COMBOS, ids=IDS)
def test_more_heavy_buckets_than_heavy_blocks(rigs, curve, wb):
    """HEAVY_RANKS + 8 buckets of more than HEAVY_NS slices, all in one length class: which eight the FIN lanes fold is
    decided by LDS atomics and differs between runs -- the commitment must not.  All entries lie in bins 0 and 1, so
    the chunked partition-2 kernels run over ~100 (16-bit) / ~200 (20-bit) chunks."""
    rig, case = rigs(curve), built(P.many_heavy, curve, wb)
    xy1, inf1 = rig.check(case)
    xy2, inf2 = rig.commit(case)
    assert inf1 == inf2 and np.array_equal(xy1, xy2), case.label() + ": two commits of one input differ"


# ---- C ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve,wb", COMBOS, ids=IDS)
def test_bin_sizes_of_the_chunked_sort(rigs, curve, wb):
    """bins of STAGE_CAP (sorted in LDS), STAGE_CAP+1, CH2-1, CH2 (one chunk), CH2+1, 2*CH2 (two), 2*CH2+1 (three)
    entries, each beside an empty bin"""
    rigs(curve).check(built(P.bin_sizes, curve, wb))


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("curve,wb", COMBOS, ids=IDS)
def test_partition_1_chunk_edges(rigs, curve, wb, delta):
    """uniform scalars, n = CH1-1, CH1, CH1+1: the last partition-1 chunk is one short, full, or one scalar"""
    rigs(curve).check(built(P.chunk1_edge, curve, wb, delta))


# ---- D ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve,wb", COMBOS, ids=IDS)
def test_one_bucket_per_commit(rigs, curve, wb):
    """only digit magnitude v occurs, so bucket v-1's weight in msm_rc1 / msm_rc2 / msm_planes and the host's Horner
    cannot be masked by another bucket: v on the row, column and RC_CH edges of the bucket matrix, every single bit,
    and the top bucket, which only msm_planes_kernel's last block reads -- that one and its neighbour also as a
    two-slice and as a heavy bucket.  Expected: v * sum 2^(wb j) tau^i over the used (i, j)."""
    rig = rigs(curve)
    half = 1 << (wb - 1)
    wrong = []
    for k, (name, v) in enumerate(P.matrix_edge_values(wb)):
        for length in (P.top_lengths(wb) if v >= half - 1 else [1]):
            case = built(P.single_magnitude, curve, wb, v, length, k)
            used = [(i, P.recode(s, wb)) for i, s in enumerate(case.ints) if s]
            assert all(len(ds) == 1 and ds[0][1] == v for _, ds in used) and len(used) == length
            want = rig.multiple_of_g(v * sum(rig.pows[i] << (wb * ds[0][0]) for i, ds in used))
            if rig.point(*rig.commit(case)) != want:
                wrong.append(f"v = {name} ({v}), {length} entries")
    assert not wrong, f"{curve} / {wb}-bit windows / one bucket per commit: wrong point for " + "; ".join(wrong)


# ---- E ---------------------------------------------------------------------------------------------------------------

CANCEL_KEY_POINTS = {16: 1 << 13, 20: 1 << 18}
_cancel_keys = {}


@pytest.fixture(scope="module")
def cancel_keys(rigs, native):
    """[G, -G] tiled, loaded with kzg_srs_load_g1 into the curve's shared context"""
    def get(curve, wb):
        if (curve, wb) not in _cancel_keys:
            rig = rigs(curve)
            x, y = rig.cv.g1
            pair = native.ints_to_limbs([x, y, x, rig.cv.p - y], rig.L).reshape(2, 2 * rig.L)
            n = CANCEL_KEY_POINTS[wb]
            xy = np.ascontiguousarray(np.tile(pair, (n // 2, 1)))
            _cancel_keys[curve, wb] = rig.ctx.srs_load_g1(xy, np.zeros(n, dtype=np.uint8))
        return _cancel_keys[curve, wb]
    yield get
    for k in _cancel_keys.values():
        k.close()
    _cancel_keys.clear()


@pytest.mark.parametrize("curve,wb", COMBOS, ids=IDS)
def test_cancellation_inside_one_bucket(rigs, cancel_keys, curve, wb):
    """Every scalar is the same single digit, so one bucket receives G and -G (times 2^(wb j)) in the order the LDS
    atomics hand out: its slices run P+P, P-P and restarts from infinity in madd_finite, and the slice partials are
    small multiples of G -- infinity and equal pairs among them -- that meet Ec::add in the heavy fold (2^13 entries)
    and in the FIN lanes (40*SEG entries).  An even count cancels to infinity (flag 1, zero words); one scalar more and
    d 2^(wb j) G is left.  The 16-bit key has 2^13 points, so the even heavy case fills it and the odd one is 2^13 - 1."""
    rig, key = rigs(curve), cancel_keys(curve, wb)
    d, j = (1 << P.LO[wb]) + 3, 2
    for n in (1 << 13, (1 << 13) - 1, 40 * P.SEG[wb], 40 * P.SEG[wb] + 1):
        case = built(P.repeated_digit, curve, wb, n, d, j)
        assert n <= key.n and max(case.ints) == min(case.ints) == d << (wb * j)
        xy, inf = rig.commit(case, key)
        if n % 2 == 0:
            assert inf == 1 and not xy.any(), case.label() + ": G and -G in equal number do not cancel"
        else:
            assert rig.point(xy, inf) == rig.multiple_of_g(d << (wb * j)), case.label()


# ---- F ---------------------------------------------------------------------------------------------------------------

def slot_sequence(curve):
    """2 * NSLOT + 1 polynomials; polynomial k takes slot k mod NSLOT, and the widths are laid out so that every slot
    changes width each time it is reused, after a polynomial of another regime"""
    top = {}
    for wb in P.WIDTHS:                                                   # D's heavy top bucket, the very case D built
        k = [v for _, v in P.matrix_edge_values(wb)].index(1 << (wb - 1))
        top[wb] = built(P.single_magnitude, curve, wb, 1 << (wb - 1), P.top_lengths(wb)[-1], k)
    seq = [built(P.many_heavy, curve, 20), built(P.uniform_case, curve, 16, 100), built(P.edges, curve, 16, False),
           built(P.uniform_case, curve, 20, 1), top[16], built(P.zeros_case, curve, 20, 777),
           built(P.edges, curve, 20, True), built(P.many_heavy, curve, 16), top[20]]
    assert len(seq) == 2 * P.NSLOT + 1
    assert all(seq[k].wb != seq[k + P.NSLOT].wb for k in range(len(seq) - P.NSLOT))
    return seq


@pytest.mark.parametrize("curve", P.CURVES)
def test_regimes_and_widths_back_to_back_through_the_slots(rigs, native, curve):
    """A fresh context (its slot buffers have never been used and only grow) takes nine polynomials with
    kzg_commit_device_async and no flush in between, alternating the two keys and the regimes: stale bstart,
    slice_off, buckets or counters of the slot's previous polynomial -- of the other width -- would show.  Each result
    equals word for word the synchronous commit of the same input in the module's context, which is checked by
    trapdoor."""
    import torch
    rig = rigs(curve)
    seq = slot_sequence(curve)
    ref = [rig.check(c) for c in seq]
    assert ref[5][1] == 1 and not ref[5][0].any()                          # no entry at all: infinity
    ctx = native.Context(curve)
    keys = rig.make_keys(ctx)                                             # keys belong to their context
    try:
        dev = [torch.from_numpy(c.limbs.view(np.int64)).to(DEV) for c in seq]
        torch.cuda.synchronize()
        outs = []
        for c, d in zip(seq, dev):
            xy, inf = np.zeros((1, 2 * rig.L), dtype=np.uint64), np.zeros(1, dtype=np.uint8)
            ctx.commit_device_async(keys[c.wb], d.data_ptr(), [c.n], c.n, xy, inf)
            outs.append((xy, inf))
        ctx.commit_flush()
        wrong = [f"#{k} {c.label()}" for k, (c, (xy, inf), (rxy, rinf)) in enumerate(zip(seq, outs, ref))
                 if int(inf[0]) != rinf or not np.array_equal(xy[0], rxy)]
        assert not wrong, "pipelined result differs from the synchronous one: " + "; ".join(wrong)
    finally:
        for k in keys.values():
            k.close()
        ctx.close()

"""The commit pipeline's slot and deferral logic (csrc/msm.hip): prep and reduce share ONE side stream, so stage B of a
polynomial is queued only behind the next polynomial's prep -- or when a path is about to wait for it (slot recycling,
kzg_commit_flush, a synchronous commit or open, teardown).  A stage B that is never queued, queued twice or queued for
the wrong slot shows as a wrong, stale or missing commitment, so every pipelined result here is compared WORD FOR WORD
with the synchronous kzg_commit_device / kzg_open_device of the same inputs (one polynomial at a time, drained after
each: nothing is deferred across polynomials there), and at the smallest size also with the oracle.

Shapes: n = 2^10 and 2^12 + 3 (16-bit windows; NSLOT = 4 slots, so 5 and 9 polynomials recycle slots once and twice),
both curves, and 5 polynomials of 2^18 (20-bit windows) on BLS12-381.  No timing is asserted: overlap is a property of
the recorded timeline (profiles/), not of a test."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import py_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
SIZES = [1 << 10, (1 << 12) + 3]
COUNTS = [1, 3, 4, 5, 9]            # NSLOT = 4: below, at, one above and twice above the number of slots
NPOLY = 9
TAU = 0x2718281828459045235360287471 % O.BN254.r
DEV = "cuda:0"


def host_polys(curve, n, count=NPOLY):
    """count x n canonical scalars (uint64[count, n, 4]) from a fixed seed: the child process of the queue-count test
    rebuilds exactly these"""
    rs = np.random.RandomState(1000 + n % 997 + 7 * CURVES.index(curve))
    a = rs.randint(0, 1 << 62, size=(count, n, 4), dtype=np.int64)
    a[..., 3] >>= 3                                       # < 2^251: below both group orders
    return a


class Case:
    """One (curve, n): its own context on a torch stream, the key, the polynomials on the device and the synchronous
    commitments of each of them.  Built once per module and never modified."""

    def __init__(self, native, curve, n, count=NPOLY):
        import torch
        self.native, self.curve, self.n, self.count = native, curve, n, count
        self.cv = O.curve(curve)
        self.ctx = native.Context(curve)
        self.stream = torch.cuda.Stream(device=DEV)
        self.ctx.bind_torch_stream(self.stream)
        self.L = self.ctx.fp_limbs
        self.srs = self.ctx.srs_generate(native.int_to_words(TAU), n)
        self.host = host_polys(curve, n, count)
        self.polys = torch.from_numpy(self.host).to(DEV)
        torch.cuda.synchronize()
        # lengths: full, shorter, odd -- cycled over the polynomials
        self.lens = [(n, n - 5, n // 2 + 1)[i % 3] for i in range(count)]
        self.ref_xy = np.zeros((count, 2 * self.L), dtype=np.uint64)
        self.ref_inf = np.zeros(count, dtype=np.uint8)
        for i in range(count):                            # synchronous, one at a time
            xy, inf = self.ctx.commit_device(self.srs, self.polys[i].data_ptr(), [self.lens[i]], n)
            self.ref_xy[i], self.ref_inf[i] = xy[0], inf[0]
        assert not self.ref_inf.any()

    def ptr(self, i):
        return self.polys[i].data_ptr()

    def outs(self, k):
        return np.zeros((k, 2 * self.L), dtype=np.uint64), np.zeros(k, dtype=np.uint8)

    def check(self, xy, inf, first, k):
        assert np.array_equal(inf, self.ref_inf[first:first + k]), (first, k)
        assert np.array_equal(xy, self.ref_xy[first:first + k]), (first, k)


_cases = {}


@pytest.fixture(scope="module")
def cases(native):
    def get(curve, n, count=NPOLY):
        key = (curve, n, count)
        if key not in _cases:
            _cases[key] = Case(native, curve, n, count)
        return _cases[key]
    yield get
    for c in _cases.values():
        c.ctx.close()
    _cases.clear()


def async_batch(case, ctx, first, k):
    """one kzg_commit_device_async call over polynomials first .. first+k-1 (contiguous on the device)"""
    xy, inf = case.outs(k)
    ctx.commit_device_async(case.srs, case.ptr(first), case.lens[first:first + k], case.n, xy, inf)
    return xy, inf, first, k


@pytest.mark.parametrize("curve", CURVES)
def test_reference_matches_the_oracle_at_the_smallest_size(cases, native, curve):
    """what every other test compares with: the synchronous commitments at n = 2^10 are p(tau) G1"""
    c = cases(curve, SIZES[0])
    for i in range(c.count):
        coeffs = native.limbs_to_ints(c.host[i, :c.lens[i]].view(np.uint64))
        want = O.normalize(O.commit_trapdoor(coeffs, TAU, c.cv), c.cv)
        assert tuple(native.limbs_to_ints(c.ref_xy[i].reshape(2, c.L))) == want


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_one_call(cases, native, curve, n, count):
    """count polynomials in ONE asynchronous call, then a flush: the last one's stage B is queued by the flush, the
    others' by their successor's enqueue, and above four the slots are recycled inside the call"""
    c = cases(curve, n)
    xy, inf, _, _ = async_batch(c, c.ctx, 0, count)
    c.ctx.commit_flush()
    c.check(xy, inf, 0, count)
    if n == SIZES[0]:                                     # and the oracle itself
        for i in range(count):
            coeffs = native.limbs_to_ints(c.host[i, :c.lens[i]].view(np.uint64))
            assert tuple(native.limbs_to_ints(xy[i].reshape(2, c.L))) == \
                O.normalize(O.commit_trapdoor(coeffs, TAU, c.cv), c.cv)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_across_calls_and_flushes(cases, curve, n):
    """the same counts spread over several calls (the deferred stage B crosses the call boundary), a flush after each
    count, two flushes in a row and a flush with nothing pending"""
    c = cases(curve, n)
    c.ctx.commit_flush()                                  # nothing pending
    for count in COUNTS:
        jobs, first, k = [], 0, 1
        while first < count:                              # calls of 1, 2, 1, 2, ... polynomials
            k = min(k, count - first)
            jobs.append(async_batch(c, c.ctx, first, k))
            first, k = first + k, 3 - k
        c.ctx.commit_flush()
        for xy, inf, f, kk in jobs:
            c.check(xy, inf, f, kk)
        c.ctx.commit_flush()                              # a second flush changes nothing
        for xy, inf, f, kk in jobs:
            c.check(xy, inf, f, kk)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_zero_length_polynomials(cases, curve, n):
    """a zero-length polynomial takes no slot and defers nothing: first, in the middle and last in a batch, and as a
    call of its own between two others"""
    c = cases(curve, n)
    for zeros in ((0,), (2,), (4,), (0, 2, 4), (0, 1, 2, 3, 4)):
        lens = [0 if i in zeros else c.lens[i] for i in range(5)]
        xy, inf = c.outs(5)
        c.ctx.commit_device_async(c.srs, c.ptr(0), lens, n, xy, inf)
        zxy, zinf = c.outs(1)
        c.ctx.commit_device_async(c.srs, c.ptr(5), [0], n, zxy, zinf)
        tail = async_batch(c, c.ctx, 5, 2)
        c.ctx.commit_flush()
        for i in range(5):
            if i in zeros:
                assert inf[i] == 1 and not xy[i].any()
            else:
                assert inf[i] == 0 and np.array_equal(xy[i], c.ref_xy[i])
        assert zinf[0] == 1 and not zxy.any()
        c.check(*tail)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_mixed_entry_points(cases, native, curve, n):
    """kzg_open_device_async shares the slots with kzg_commit_device_async, and a SYNCHRONOUS commit between two
    asynchronous ones drains the pipeline: what was pending must still be right when the caller flushes"""
    c = cases(curve, n)
    ctx, L = c.ctx, c.L
    z, xi = 0x1234567 % c.cv.r, 0x7654321 % c.cv.r
    zw, xw = native.int_to_words(z), native.int_to_words(xi)
    opens = [(0, [n, n - 1, 7]), (3, [n - 5]), (4, [n // 2, n])]         # (first polynomial, lens)
    want = [ctx.open(c.srs, c.ptr(f), lens, n, zw, xw, device=True) for f, lens in opens]
    if n == SIZES[0]:                                     # the synchronous opening against the oracle's trapdoor form
        f, lens = opens[0]
        ps = [native.limbs_to_ints(c.host[f + i, :m].view(np.uint64)) for i, m in enumerate(lens)]
        wxy, winf, wev = want[0]
        assert winf[0] == 0
        assert tuple(native.limbs_to_ints(wxy.reshape(2, L))) == O.normalize(O.open_trapdoor(ps, z, xi, TAU, c.cv), c.cv)
        assert native.limbs_to_ints(wev.reshape(1, 4))[0] == O.poly_eval(O.combine(ps, xi, c.cv.r), z, c.cv.r)
    got, commits = [], []
    for j, (f, lens) in enumerate(opens):
        commits.append(async_batch(c, ctx, j, 2))
        out = (np.zeros(2 * L, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(4, dtype=np.uint64))
        ctx.open_device_async(c.srs, c.ptr(f), lens, n, zw, xw, *out)
        got.append(out)
        if j == 1:                                        # synchronous, with three polynomials pending around it
            sxy, sinf = ctx.commit_device(c.srs, c.ptr(6), c.lens[6:9], n)
            c.check(sxy, sinf, 6, 3)
    commits.append(async_batch(c, ctx, 8, 1))
    ctx.commit_flush()
    for job in commits:
        c.check(*job)
    for (wxy, winf, wev), (xy, inf, ev) in zip(want, got):
        assert inf[0] == winf[0] and np.array_equal(xy, wxy) and np.array_equal(ev, wev)


@pytest.mark.parametrize("which", ["torch_stream", "null_stream", "own_stream"])
@pytest.mark.parametrize("curve", CURVES)
def test_caller_streams(cases, native, curve, which):
    """the caller's stream carries ev_in and the scalar copy: a torch stream, HIP's null stream, the context's own"""
    import torch
    c = cases(curve, SIZES[1])
    ctx = native.Context(curve)
    try:
        if which == "torch_stream":
            ctx.bind_torch_stream(torch.cuda.Stream(device=DEV))
        elif which == "null_stream":
            ctx.bind_torch_stream(torch.cuda.default_stream(DEV))
        srs = ctx.srs_generate(native.int_to_words(TAU), c.n)           # keys belong to their context
        jobs = []
        for first, k in ((0, 5), (5, 1), (6, 3)):
            xy, inf = c.outs(k)
            ctx.commit_device_async(srs, c.ptr(first), c.lens[first:first + k], c.n, xy, inf)
            jobs.append((xy, inf, first, k))
        ctx.commit_flush()
        for job in jobs:
            c.check(*job)
        srs.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_two_contexts_interleaved(cases, native, curve):
    """two contexts alive at once: each has its own slots, streams and deferred stage"""
    import torch
    c = cases(curve, SIZES[1])
    ctxs = [native.Context(curve) for _ in range(2)]
    try:
        keys, jobs = [], ([], [])
        for ctx in ctxs:
            ctx.bind_torch_stream(torch.cuda.Stream(device=DEV))
            keys.append(ctx.srs_generate(native.int_to_words(TAU), c.n))
        for first, k in ((0, 1), (1, 3), (4, 5)):
            for w in (0, 1):
                f = first if w == 0 else NPOLY - first - k               # the second context walks backwards
                xy, inf = c.outs(k)
                ctxs[w].commit_device_async(keys[w], c.ptr(f), c.lens[f:f + k], c.n, xy, inf)
                jobs[w].append((xy, inf, f, k))
        ctxs[1].commit_flush()
        ctxs[0].commit_flush()
        for w in (0, 1):
            for job in jobs[w]:
                c.check(*job)
        for k in keys:
            k.close()
    finally:
        for ctx in ctxs:
            ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_teardown_and_recreate(cases, native, curve):
    """a context destroyed after a flush -- and one destroyed with a polynomial still pending, whose deferred stage is
    dropped with it -- and a new one created: fresh streams, fresh slots, the same results"""
    c = cases(curve, SIZES[0])
    for pending_at_close in (False, True, False):
        ctx = native.Context(curve)
        srs = ctx.srs_generate(native.int_to_words(TAU), c.n)
        xy, inf = c.outs(5)
        ctx.commit_device_async(srs, c.ptr(0), c.lens[:5], c.n, xy, inf)
        ctx.commit_flush()
        c.check(xy, inf, 0, 5)
        if pending_at_close:
            pxy, pinf = c.outs(2)
            ctx.commit_device_async(srs, c.ptr(5), c.lens[5:7], c.n, pxy, pinf)
        srs.close()
        ctx.close()
        if pending_at_close:
            assert not pxy[1].any()                       # never retired: the newest result is dropped, not written


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_input_buffer_overwritten_after_enqueue(cases, curve, n):
    """the caller's buffer is free as soon as the call returns: the slot's scalar copy is ordered on the caller's
    stream in front of whatever it enqueues next"""
    import torch
    c = cases(curve, n)
    jobs = []
    with torch.cuda.stream(c.stream):
        buf = torch.empty((3, n, 4), dtype=torch.int64, device=DEV)
        for first in (0, 3, 6):
            buf.copy_(c.polys[first:first + 3])
            xy, inf = c.outs(3)
            c.ctx.commit_device_async(c.srs, buf.data_ptr(), c.lens[first:first + 3], n, xy, inf)
            jobs.append((xy, inf, first, 3))
            buf.fill_(-1)                                 # right behind the enqueue, on the caller's stream
    c.ctx.commit_flush()
    for job in jobs:
        c.check(*job)


def test_twenty_bit_windows(cases):
    """n = 2^18 takes the 20-bit windows (another prep plan, another reduce grid): 5 polynomials in one call, then
    spread over calls"""
    c = cases("bls12_381", 1 << 18, 5)
    one = async_batch(c, c.ctx, 0, 5)
    c.ctx.commit_flush()
    c.check(*one)
    jobs = [async_batch(c, c.ctx, f, k) for f, k in ((0, 1), (1, 1), (2, 3))]
    c.ctx.commit_flush()
    for job in jobs:
        c.check(*job)


# ---- another number of hardware queues: only a process that has not started HIP yet can have one

def _child(path):
    """runs in a fresh interpreter (python <this file> <out.npz>): the 9-polynomial call for both curves"""
    from kzg_snark_amd import _native
    import torch
    out = {}
    for curve in CURVES:
        n = SIZES[1]
        ctx = _native.Context(curve)
        ctx.bind_torch_stream(torch.cuda.Stream(device=DEV))
        srs = ctx.srs_generate(_native.int_to_words(TAU), n)
        polys = torch.from_numpy(host_polys(curve, n)).to(DEV)
        torch.cuda.synchronize()
        lens = [(n, n - 5, n // 2 + 1)[i % 3] for i in range(NPOLY)]
        xy = np.zeros((NPOLY, 2 * ctx.fp_limbs), dtype=np.uint64)
        inf = np.zeros(NPOLY, dtype=np.uint8)
        ctx.commit_device_async(srs, polys.data_ptr(), lens, n, xy, inf)
        ctx.commit_flush()
        out[curve + "_xy"], out[curve + "_inf"] = xy, inf
        srs.close()
        ctx.close()
    out["queues"] = np.array([int(os.environ["GPU_MAX_HW_QUEUES"])])
    np.savez(path, **out)


def test_other_queue_count(cases, tmp_path):
    """the results do not depend on how many hardware queues the process has: a NEW interpreter (started, never an
    exec of this one) runs the 9-polynomial call with GPU_MAX_HW_QUEUES=8 set before its HIP runtime starts"""
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(path)
    assert int(got["queues"][0]) == 8
    for curve in CURVES:
        c = cases(curve, SIZES[1])
        xy, inf, _, _ = async_batch(c, c.ctx, 0, NPOLY)
        c.ctx.commit_flush()
        c.check(xy, inf, 0, NPOLY)
        assert np.array_equal(got[curve + "_xy"], xy) and np.array_equal(got[curve + "_inf"], inf)


if __name__ == "__main__":
    _child(sys.argv[1])

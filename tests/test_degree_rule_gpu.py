"""The degree rule on the GPU: the case table of tests/degree_cases.py (pinned to the oracle by
tests/test_degree_rule_host.py) through every entry point that states the rule.

DEGREE decides in kzg_open, kzg_open_device, kzg_open_device_async and kzg_open_points[_device]: when the quotient is
longer than the key, any_nonzero_kernel looks at the elements [key size, quotient length) -- a range that starts off a
multiple of 256, ends before stale words of an earlier opening, and holds zeros that were computed, not written.  LENGTH
decides in kzg_commit* and kzg_open_shard_finish.  The facade maps KZG_ERR_DEGREE to the reference's ValueError.  After a
refusal the caller's buffers are as they were and the context and its pipeline go on as if the call had not been made.

Keys of m points come from a known tau, so that every expected point is one scalar multiplication (the trapdoor
identity); every comparison is exact."""
import ctypes
import random

import numpy as np
import pytest

import degree_cases as D
from multi_restated import check_in_the_exponent
from oracle import py_oracle as O

pytestmark = pytest.mark.gpu

CURVES = D.CURVES
ENTRY = ("host", "device", "async")
FILL = 0xA5


class Env:
    def __init__(self, native, curve):
        self.native, self.curve, self.cv = native, curve, O.curve(curve)
        self.r = self.cv.r
        self.ctx = native.get_context(curve)
        self.tau = D.tau_of(curve)
        self._keys = {}

    def key(self, m):
        """the key of m points [tau^i] G1, made once"""
        if m not in self._keys:
            self._keys[m] = self.ctx.srs_generate(self.native.int_to_words(self.tau), m)
        return self._keys[m]

    def close(self):
        for k in self._keys.values():
            k.close()

    def words(self, v):
        return self.native.int_to_words(v)

    def point(self, xy, inf):
        return None if inf[0] else tuple(self.native.limbs_to_ints(xy.reshape(2, self.ctx.fp_limbs)))

    def commitment(self, coeffs):
        return O.normalize(O.commit_trapdoor(coeffs, self.tau, self.cv), self.cv)

    def filled(self):
        """result buffers of one opening, every byte FILL"""
        return (np.full(2 * self.ctx.fp_limbs, FILL * 0x0101010101010101, dtype=np.uint64),
                np.full(1, FILL, dtype=np.uint8), np.full(4, FILL * 0x0101010101010101, dtype=np.uint64))


@pytest.fixture(scope="module")
def envs(native):
    out = {c: Env(native, c) for c in CURVES}
    yield out
    for e in out.values():
        e.close()


def pack(native, polys, extra_rows=0):
    """the polynomials as rows of one array (`extra_rows` rows of FILL bytes above them) -> (array, lens, stride)"""
    stride = max(max((len(p) for p in polys), default=0), 1)
    arr = np.zeros((len(polys) + extra_rows, stride, 4), dtype=np.uint64)
    for i, p in enumerate(polys):
        if p:
            arr[i, :len(p)] = native.ints_to_limbs(p)
    arr[len(polys):] = FILL * 0x0101010101010101
    return arr, [len(p) for p in polys], stride


def to_device(arr):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return d


def row_ints(native, tensor, row, count):
    import torch
    torch.cuda.synchronize()
    flat = tensor[row, :count].cpu().numpy().view(np.uint64).reshape(count, 4)
    return native.limbs_to_ints(flat) if count else []


def as_int(words):
    return int.from_bytes(np.ascontiguousarray(words).tobytes(), "little")


def open_once(env, case, how, arr, lens, stride, d):
    """one opening -> ("refuse", None, None) or ("accept", point, P(z)); any error but KZG_ERR_DEGREE propagates"""
    native, ctx = env.native, env.ctx
    key, zw, xw = env.key(case.m), env.words(case.z), env.words(case.xi)
    try:
        if how == "host":
            xy, inf, ev = ctx.open(key, arr, lens, stride, zw, xw)
        elif how == "device":
            xy, inf, ev = ctx.open(key, d.data_ptr(), lens, stride, zw, xw, device=True)
        else:
            xy, inf, ev = env.filled()
            try:
                ctx.open_device_async(key, d.data_ptr(), lens, stride, zw, xw, xy, inf, ev)
            finally:
                ctx.commit_flush()
    except native.NativeError as e:
        if e.code != native.KZG_ERR_DEGREE:
            raise
        assert "longer than the commitment key" in str(e)
        return ("refuse", None, None)
    return ("accept", env.point(xy, inf), as_int(ev))


def check_case(env, case, hows=ENTRY, before=None, note=""):
    """the case through the entry points `hows` (after `before()`, each): the table's verdict, point and evaluation"""
    want = D.expect(env.curve, case)
    arr, lens, stride = pack(env.native, case.polys)
    d = to_device(arr) if set(hows) - {"host"} else None
    for how in hows:
        if before is not None:
            before()
        got = open_once(env, case, how, arr, lens, stride, d)
        assert got[0] == want.verdict, (case.label, how, note)
        if want.verdict == "accept":
            assert got[1] == want.point, (case.label, how, note, "point")
            assert got[2] == want.value, (case.label, how, note, "evaluation")


def family_cases(curve, letters):
    return [c for c in D.table(curve) if D.family(c) in letters]


# ---- verdicts, every entry point ----------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", ["A", "B", "C", "E"])
@pytest.mark.parametrize("curve", CURVES)
def test_the_verdict_of_every_entry_point(envs, curve, fam):
    """kzg_open, kzg_open_device and kzg_open_device_async + flush agree with the table case by case: KZG_ERR_DEGREE
    exactly where the reference refuses, the trapdoor's point and P(z) everywhere else"""
    for case in family_cases(curve, fam):
        check_case(envs[curve], case)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_words_beyond_the_range_do_not_count(envs, curve):
    """family D: each opening follows one of 700 coefficients more on the same context, whose combination and quotient
    -- random, non-zero -- lie in the same buffer beyond the new quotient's end"""
    env = envs[curve]
    rng = random.Random(41)
    for case in family_cases(curve, "D"):
        stale = D.stale_poly(curve, case)
        arr, lens, stride = pack(env.native, [stale])
        z, xi = rng.randrange(1, env.r), rng.randrange(1, env.r)

        def before():
            env.ctx.open(env.key(D.MAX_N), arr, lens, stride, env.words(z), env.words(xi))

        check_case(env, case, before=before)


@pytest.mark.parametrize("curve", CURVES)
def test_the_verdict_at_every_tile_plan(envs, curve):
    """families B and E in tiles of 1024 (`open_tile_threads` = 128), and the longest of them with the aggregates of
    64 tiles folded first (`open_direct_tiles` = 1)"""
    env = envs[curve]
    cases = family_cases(curve, "BE")
    longest = max(D.length(c) for c in cases)
    try:
        env.ctx.set_tuning("open_tile_threads", 128)
        for case in cases:
            check_case(env, case, hows=("device", "async"), note="tiles of 1024")
        env.ctx.set_tuning("open_direct_tiles", 1)
        for tb in (128, 0):
            env.ctx.set_tuning("open_tile_threads", tb)
            for case in cases:
                if D.length(case) == longest:
                    check_case(env, case, note=("grouped tiles", tb))
    finally:
        env.ctx.set_tuning("open_tile_threads", 0)
        env.ctx.set_tuning("open_direct_tiles", 0)


# ---- kzg_open_points ------------------------------------------------------------------------------------------------

def points_once(env, pc, device):
    """-> ("refuse", None, None) or ("accept", point, the n - 1 words d_quot received)"""
    native, ctx = env.native, env.ctx
    k = len(pc.polys)
    arr, lens, stride = pack(native, pc.polys, extra_rows=1)
    n = max(lens)
    d = to_device(arr)
    d_quot = d.data_ptr() + k * stride * 32
    try:
        xy, inf = ctx.open_points(env.key(pc.m), d.data_ptr() if device else arr[:k], lens, stride, pc.points,
                                  pc.weights, d_quot=d_quot, device=device)
    except native.NativeError as e:
        if e.code != native.KZG_ERR_DEGREE:
            raise
        return ("refuse", None, None)
    return ("accept", env.point(xy, inf), row_ints(native, d, k, n - 1))


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_open_points_restates_the_plain_opening(envs, curve, device):
    """t = 1 and the weights xi^(i+1): kzg_open's verdicts and points on families B and E; on accept every one of the
    n - 1 words of d_quot, the zeros beyond the key included"""
    env = envs[curve]
    for case in family_cases(curve, "BE"):
        want = D.expect(curve, case)
        got = points_once(env, D.as_points(case, env.r), device)
        assert got[0] == want.verdict, case.label
        if want.verdict == "accept":
            q = D.witness(case, env.r)[0]
            assert got[1] == want.point, case.label
            assert got[2] == q + [0] * (D.length(case) - 1 - len(q)), case.label


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_open_points_degree_decides(envs, curve, device):
    """t = 4 (two launches of three points) with a quotient that cancels beyond the key although no point's own does,
    and the same one off; nothing but zero weights (no launch at all); a polynomial longer than the key without weight"""
    env = envs[curve]
    seen = set()
    for pc in D.points_table(curve):
        want = D.expect_points(curve, pc)
        got = points_once(env, pc, device)
        seen.add(got[0])
        assert got[0] == want.verdict, pc.label
        if want.verdict == "accept":
            assert got[1] == want.point, pc.label
            assert got[2] == want.quotient, pc.label
    assert seen == {"accept", "refuse"}


# ---- the facade -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


def facade_key(kzg, env, m):
    from kzg_snark_amd.kzg import CommitmentKey
    assert kzg._context() is env.ctx
    return CommitmentKey(env.ctx, env.key(m))


def refusal_of_the_reference(m):
    return pytest.raises(ValueError, match=f"exceeds maximum allowed degree {m - 1}$")


@pytest.mark.parametrize("curve", CURVES)
def test_facade_open(envs, kzgs, curve):
    """KZG.open: the reference's ValueError exactly for the refused cases of A and E (lists), and of B given as limb
    buffers, whose trailing zeros the facade trims itself"""
    env, kzg = envs[curve], kzgs[curve]
    seen = set()
    for case in family_cases(curve, "ABE"):
        want = D.expect(curve, case)
        polys = case.polys
        if D.family(case) == "B":
            polys = [np.ascontiguousarray(env.native.ints_to_limbs(p), dtype=np.uint64) for p in polys]
            assert polys[0].shape == (D.length(case), 4)
        ck = facade_key(kzg, env, case.m)
        seen.add((D.family(case), want.verdict))
        if want.verdict == "refuse":
            with refusal_of_the_reference(case.m):
                kzg.open(ck, polys, case.z, case.xi)
        else:
            got = kzg.open(ck, polys, case.z, case.xi)
            assert O.eq(tuple(int(c) for c in got), O.from_affine(want.point) if want.point else O.Z1(), env.cv), case.label
    assert seen == {(f, v) for f in "ABE" for v in ("accept", "refuse")}


@pytest.mark.parametrize("curve", CURVES)
def test_facade_open_multi(envs, kzgs, curve):
    env, kzg = envs[curve], kzgs[curve]
    cv, r, tau = env.cv, env.r, env.tau
    rng = random.Random(53)
    m = 300
    ck = facade_key(kzg, env, m)
    gamma, zeta, z = (rng.randrange(1, r) for _ in range(3))

    def holds(polys, sets, proof):
        comms = [O.commit_trapdoor(p, tau, cv) for p in polys]
        W, W2 = (tuple(int(c) for c in pt) for pt in (proof.W, proof.W2))
        assert not O.is_inf(W) and not O.is_inf(W2)
        assert proof.evaluations == [[O.poly_eval(p, y, r) for y in S] for p, S in zip(polys, sets)]
        return check_in_the_exponent(comms, sets, proof.evaluations, W, W2, gamma, zeta, tau, cv)

    # one polynomial of m + 1 coefficients at one point: both quotients fill the key exactly
    p = D.rand_poly(rng, m + 1, r)
    assert holds([p], [[z]], kzg.open_multi(ck, [p], [[z]], gamma, zeta))
    with refusal_of_the_reference(m):
        kzg.open_multi(ck, [D.rand_poly(rng, m + 2, r)], [[z]], gamma, zeta)
    # two polynomials of 2 m + 1 coefficients whose gamma-combination vanishes above the key, at a shared point
    polys = D.cancelling(rng, r, 2, m, m, "cancel", gamma)
    assert all(len(q) == 2 * m + 1 and q[-1] for q in polys)
    assert holds(polys, [[z], [z]], kzg.open_multi(ck, polys, [[z], [z]], gamma, zeta))
    off = D.cancelling(rng, r, 2, m, m, "high", gamma)
    with refusal_of_the_reference(m):
        kzg.open_multi(ck, off, [[z], [z]], gamma, zeta)


# ---- where length decides -------------------------------------------------------------------------------------------

def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else ctypes.c_void_p(a)


@pytest.mark.parametrize("curve", CURVES)
def test_commit_refuses_by_length_before_any_work(envs, kzgs, curve):
    """lens = [m, m + 1, 3] with the second row all zeros: KZG_ERR_DEGREE from kzg_commit, kzg_commit_device and
    kzg_commit_device_async, and not a byte of the outputs written -- polynomial 0's neither, then or at the flush"""
    env, kzg = envs[curve], kzgs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    m = 300
    rng = random.Random(7)
    rows = [D.rand_poly(rng, m, r), [0] * (m + 1), D.rand_poly(rng, 3, r)]
    arr, lens, stride = pack(native, rows)
    assert lens == [m, m + 1, 3] and not arr[1].any()
    d = to_device(arr)
    lens_a = np.asarray(lens, dtype=np.uint64)
    key = env.key(m)
    for name, data in (("kzg_commit", arr), ("kzg_commit_device", d.data_ptr()), ("kzg_commit_device_async", d.data_ptr())):
        xy = np.full((3, 2 * ctx.fp_limbs), FILL * 0x0101010101010101, dtype=np.uint64)
        inf = np.full(3, FILL, dtype=np.uint8)
        rc = getattr(native.lib(), name)(ctx._h, key._h, vp(data), vp(lens_a), 3, stride, vp(xy), vp(inf))
        assert rc == native.KZG_ERR_DEGREE, name
        assert (xy.view(np.uint8) == FILL).all() and (inf == FILL).all(), name
        ctx.commit_flush()
        assert (xy.view(np.uint8) == FILL).all() and (inf == FILL).all(), (name, "after the flush")
        # the context goes on: the rows that fit, through the same entry point's wrapper
        fits = [0, 2]
        if name == "kzg_commit":
            got = [ctx.commit(key, arr[i:i + 1], [lens[i]], stride) for i in fits]
        else:
            got = [ctx.commit_device(key, d.data_ptr() + i * stride * 32, [lens[i]], stride) for i in fits]
        assert [env.point(x[0], i) for x, i in got] == [env.commitment(rows[i]) for i in fits], name
    with pytest.raises(native.NativeError) as e:
        ctx.commit_device_async(key, d.data_ptr(), lens, stride, xy, inf)
    assert e.value.code == native.KZG_ERR_DEGREE and ctx._inflight == []
    # the facade trims, so its rule is the degree
    ck = facade_key(kzg, env, m)
    got = kzg.commit(ck, [[5] + [0] * (m + 3)])[0]
    assert O.eq(tuple(int(c) for c in got), O.commit_trapdoor([5], env.tau, env.cv), env.cv)
    with pytest.raises(ValueError, match=f"Polynomial degree {m} exceeds maximum allowed degree {m - 1}$"):
        kzg.commit(ck, [D.rand_poly(rng, m + 1, r)])


@pytest.mark.parametrize("curve", CURVES)
def test_shard_finish_refuses_by_length_and_keeps_the_slice(envs, curve):
    """a slice of L coefficients: the first rank commits L - 1 of them, any other rank L.  One key point too few is
    KZG_ERR_DEGREE even when the slice's top coefficient is a literal zero; the slice is still held afterwards"""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    L = 301
    rng = random.Random(19)
    none = env.words(0)
    for z in (rng.randrange(1, r), 0):
        for top_zero in (False, True):
            polys = [D.rand_poly(rng, L, r), D.rand_poly(rng, L - 5, r)]
            if top_zero:
                polys[0][-1] = 0
            xi = rng.randrange(1, r)
            arr, lens, stride = pack(native, polys)
            d = to_device(arr)
            zw, xw = env.words(z), env.words(xi)
            comb = O.combine(polys, xi, r)
            comb += [0] * (L - len(comb))
            S = [0] * (L + 1)                                   # S_j = c_j + z S_(j+1): the suffix values of the slice
            for j in range(L - 1, -1, -1):
                S[j] = (comb[j] + z * S[j + 1]) % r
            ctx.open_shard_begin(d.data_ptr(), lens, stride, zw, xw)
            for first, vec in ((1, S[1:L]), (0, S[:L])):
                fits, short = env.key(len(vec)), env.key(len(vec) - 1)
                xy, inf, ev = ctx.open_shard_finish(fits, zw, none, first)
                assert env.point(xy, inf) == env.commitment(vec), (z == 0, top_zero, first)
                assert as_int(ev) == S[0]
                with pytest.raises(native.NativeError) as e:
                    ctx.open_shard_finish(short, zw, none, first)
                assert e.value.code == native.KZG_ERR_DEGREE and "key shard" in str(e.value)
                again = ctx.open_shard_finish(fits, zw, none, first)          # the slice is still held
                assert env.point(again[0], again[1]) == env.point(xy, inf) and as_int(again[2]) == S[0]
            # the first rank's vector is the quotient: what the plain opening commits
            xy, inf, ev = ctx.open(env.key(L - 1), d.data_ptr(), lens, stride, zw, xw, device=True)
            assert env.point(xy, inf) == env.commitment(S[1:L]) and as_int(ev) == S[0]


# ---- state after a refusal ------------------------------------------------------------------------------------------

def pick(curve, label):
    return next(c for c in D.table(curve) if c.label == label)


@pytest.mark.parametrize("curve", CURVES)
def test_the_context_after_each_kind_of_refusal(envs, curve):
    """after a refused kzg_open, kzg_open_device, kzg_open_device_async, kzg_open_points, kzg_commit and
    kzg_open_shard_finish a valid opening on the same context gives the right point; the synchronous forms leave
    out_xy / out_inf as the caller had them"""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    good = pick(curve, "B:m300:R257:fits:zr")
    bad = pick(curve, "E:k2:m300:R300:high:zr")
    assert D.expect(curve, good).verdict == "accept" and D.expect(curve, bad).verdict == "refuse"
    arr, lens, stride = pack(native, bad.polys)
    d = to_device(arr)
    key, zw, xw = env.key(bad.m), env.words(bad.z), env.words(bad.xi)
    lens_a = np.asarray(lens, dtype=np.uint64)

    def raw(name, data):
        xy, inf, ev = env.filled()
        rc = getattr(native.lib(), name)(ctx._h, key._h, vp(data), vp(lens_a), len(lens), stride, vp(zw), vp(xw), vp(xy),
                                         vp(inf), vp(ev))
        assert rc == native.KZG_ERR_DEGREE, name
        assert (xy.view(np.uint8) == FILL).all() and inf[0] == FILL, name

    def refused_points():
        assert points_once(env, D.as_points(bad, r), True)[0] == "refuse"

    def refused_commit():
        with pytest.raises(native.NativeError) as e:
            ctx.commit_device(key, d.data_ptr(), [bad.m + 1], stride)
        assert e.value.code == native.KZG_ERR_DEGREE

    def refused_finish():
        ctx.open_shard_begin(d.data_ptr(), lens, stride, zw, xw)
        with pytest.raises(native.NativeError) as e:
            ctx.open_shard_finish(key, zw, env.words(0), True)
        assert e.value.code == native.KZG_ERR_DEGREE

    refusals = [lambda: raw("kzg_open", arr), lambda: raw("kzg_open_device", d.data_ptr()),
                lambda: raw("kzg_open_device_async", d.data_ptr()), refused_points, refused_commit, refused_finish]
    for i, refuse in enumerate(refusals):
        check_case(env, good, hows=("device", "async"), before=refuse, note=("after refusal", i))


def enqueue(env, case, d, lens, stride):
    """kzg_open_device_async into buffers of FILL bytes -> (buffers, the NativeError or None)"""
    bufs = env.filled()
    try:
        env.ctx.open_device_async(env.key(case.m), d.data_ptr(), lens, stride, env.words(case.z), env.words(case.xi), *bufs)
    except env.native.NativeError as e:
        return bufs, e
    return bufs, None


@pytest.mark.parametrize("curve", CURVES)
def test_a_refusal_in_the_middle_of_the_pipeline(envs, curve):
    """accept, refuse, accept, flush: both accepted openings are right, and the refused call's out_xy / out_inf are at
    the flush what they were when the call returned -- as the caller had them.  Then six refusals in a row (more than
    the pipeline's four slots), four accepted openings and a flush: a refusal holds no slot."""
    env = envs[curve]
    native, ctx = env.native, env.ctx
    labels = ["E:k2:m300:R300:cancel:zr", "E:k17:m300:R1:low:zmax", "B:m2048:R513:fits:z0", "B:m255:R256:over:zr",
              "E:k17:m2048:R300:cancel:z0", "C:R257:mirror"]
    cases = {c.label: c for c in D.table(curve) if c.label in labels}
    assert len(cases) == len(labels)
    dev = {}
    for label, case in cases.items():
        arr, lens, stride = pack(native, case.polys)
        dev[label] = (to_device(arr), lens, stride)
    want = {label: D.expect(curve, case) for label, case in cases.items()}
    assert [want[x].verdict for x in labels] == ["accept", "refuse", "accept", "refuse", "accept", "accept"]

    def result(bufs):
        return env.point(bufs[0], bufs[1]), as_int(bufs[2])

    a, err_a = enqueue(env, cases[labels[0]], *dev[labels[0]])
    b, err_b = enqueue(env, cases[labels[1]], *dev[labels[1]])
    snapshot = (b[0].copy(), b[1].copy())
    c, err_c = enqueue(env, cases[labels[2]], *dev[labels[2]])
    ctx.commit_flush()
    assert err_a is None and err_c is None and err_b is not None and err_b.code == native.KZG_ERR_DEGREE
    assert result(a) == (want[labels[0]].point, want[labels[0]].value)
    assert result(c) == (want[labels[2]].point, want[labels[2]].value)
    assert np.array_equal(b[0], snapshot[0]) and np.array_equal(b[1], snapshot[1])          # no late write
    assert (b[0].view(np.uint8) == FILL).all() and b[1][0] == FILL

    refused = [enqueue(env, cases[labels[1 + 2 * (i % 2)]], *dev[labels[1 + 2 * (i % 2)]]) for i in range(6)]
    accepted = [labels[0], labels[2], labels[4], labels[5]]
    pending = [enqueue(env, cases[x], *dev[x]) for x in accepted]
    ctx.commit_flush()
    assert all(e is not None and e.code == native.KZG_ERR_DEGREE for _, e in refused)
    assert all((bufs[0].view(np.uint8) == FILL).all() and bufs[1][0] == FILL for bufs, _ in refused)
    for x, (bufs, e) in zip(accepted, pending):
        assert e is None and result(bufs) == (want[x].point, want[x].value), x
    assert ctx._inflight == []

"""kzg_open_coset at every level, edge and carry of its blocked scan (coset_tile_kernel, coset_fill_kernel,
coset_scan_level and open_coset_quotient_t, csrc/poly.hip): the shapes of tests/coset_scan_profiles.py -- what they
reach is pinned by tests/test_coset_scan_profiles_host.py -- on both curves, against Python integers that never pass
through the library.  Every comparison is exact.

The expectation of one call, from the definition alone:
    comb      = O.combine(polys, xi, r)                       sum_j xi^(j+1) p_j
    (q, rho)  = coset_divide(comb, l, h^l, r)                 the plain suffix recursion
    proof     = [q(tau)] G1                                   one scalar multiplication of the oracle's
    values    = O.fft_ff([rho_j h^j], zeta, r)                and values 0, 1, l-1 also = comb(h zeta^k), by Horner
The keys come from a known tau; a key is at least as long as the polynomial (the next power of two), exactly as long
where the length rule is the subject."""
import ctypes
import random

import numpy as np
import pytest

import coset_scan_profiles as P
from oracle import c_oracle
from oracle import py_oracle as O

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
KZG_ERR_ARG = -1
FILL = 0xA5
FILL64 = FILL * 0x0101010101010101
H_KINDS = ("random", "one", "minus_one")                      # h^l: anything | 1 | r - 1


class Env:
    """One curve's context and its keys of [tau^i] G1 (made once per size)"""

    def __init__(self, native, curve, ctx=None):
        self.native, self.curve, self.cv = native, curve, O.curve(curve)
        self.r = self.cv.r
        self.ctx = ctx or native.get_context(curve)
        self.tau = TAU % self.r
        self._keys = {}
        self._g = native.ints_to_limbs(list(self.cv.g1), self.ctx.fp_limbs).reshape(-1)

    def key_exact(self, m):
        if m not in self._keys:
            self._keys[m] = self.ctx.srs_generate(self.native.int_to_words(self.tau), m)
        return self._keys[m]

    def key(self, n):
        """a key of at least n points: the next power of two"""
        return self.key_exact(1 << max(n - 1, 0).bit_length())

    def close(self):
        for k in self._keys.values():
            k.close()
        self._keys = {}

    def g1_scalar(self, s):
        """[s] G1 through the C oracle, as (x, y) / None"""
        xy, inf = c_oracle.g1_mul(self.curve, self._g, s % self.r)
        return None if inf else tuple(self.native.limbs_to_ints(np.asarray(xy).reshape(2, self.ctx.fp_limbs)))

    def point(self, xy, inf):
        assert inf[0] in (0, 1)
        return None if inf[0] else tuple(self.native.limbs_to_ints(np.asarray(xy).reshape(2, self.ctx.fp_limbs)))


@pytest.fixture(scope="module")
def envs(native):
    out = {c: Env(native, c) for c in CURVES}
    yield out
    for e in out.values():
        e.close()


def pack(native, polys, stride=None, extra_rows=0):
    """the polynomials as rows of one array, `extra_rows` rows of FILL bytes after them -> (array, lens, stride)"""
    stride = stride or max(max((len(p) for p in polys), default=0), 1)
    arr = np.zeros((len(polys) + extra_rows, stride, 4), dtype=np.uint64)
    for i, p in enumerate(polys):
        if p:
            arr[i, :len(p)] = native.ints_to_limbs(p)
    arr[len(polys):] = FILL64
    return arr, [len(p) for p in polys], stride


def to_device(arr):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return d


def expect(env, polys, xi, log_l, h, zeta):
    """(proof point or None, the l values) from Python integers alone"""
    r, l = env.r, 1 << log_l
    comb = O.combine(polys, xi, r)
    q, rho = P.coset_divide(comb, l, pow(h, l, r), r)
    assert len(q) == max(len(comb) - l, 0)
    point = env.g1_scalar(O.poly_eval(q, env.tau, r))
    scaled, hp = [], 1
    for c in rho:
        scaled.append(c * hp % r)
        hp = hp * h % r
    values = list(O.fft_ff(scaled, zeta, r))
    for k in sorted({0, 1 % l, l - 1}):                        # the DFT restatement itself, pinned to the polynomial
        assert values[k] == O.poly_eval(comb, h * pow(zeta, k, r) % r, r), k
    return point, values


def got(env, out):
    xy, inf, ev = out
    return env.point(xy, inf), env.native.limbs_to_ints(ev)


def open_host(env, key, polys, log_l, h, zeta, xi):
    arr, lens, stride = pack(env.native, polys)
    return got(env, env.ctx.open_coset(key, arr, lens, stride, log_l, h, zeta, xi))


# ---- the case table ---------------------------------------------------------------------------------------------------
TABLE = P.cases()
_WANT = {}


def case_poly(env, case):
    """the case's polynomial: random coefficients, the top one non-zero -- the same at every call"""
    rng = random.Random("%s:%s:poly" % (env.curve, case.label))
    p = [rng.randrange(env.r) for _ in range(case.n)]
    p[-1] = rng.randrange(1, env.r)
    return p


def coset_of(cv, rng, l, kind, cubed):
    """(h, zeta): h of the asked kind, zeta the primitive l-th root of unity or its cube"""
    r = cv.r
    zeta = cv.root_of_unity(l)
    if cubed:
        zeta = pow(zeta, 3, r)
    if kind == "random":
        h = rng.randrange(1, r)
    elif kind == "one":
        h = pow(cv.root_of_unity(l), rng.randrange(l), r)
        assert pow(h, l, r) == 1
    else:
        h = pow(cv.root_of_unity(2 * l), 2 * rng.randrange(l) + 1, r)
        assert pow(h, l, r) == r - 1
    return h, zeta


def case_runs(env, idx, case, p):
    """[(h, zeta, expectation)] of case number idx: its kind of h (the three in turn) and, where that fixes h^l to
    1 or r - 1 -- a multiplier whose powers a scan cannot get wrong --, a random h as well; zeta in turn the root and
    its cube.  l = 4096, where the Python expectation is the cost, runs once per case: the kind in turn while one tile
    holds every row, a random h once there is a level above.  Computed once per curve and case."""
    k = (env.curve, case.label)
    if k not in _WANT:
        rng = random.Random("%s:%s:coset" % k)
        l = 1 << case.log_l
        kind = H_KINDS[idx % 3]
        if case.log_l == P.CS_MAX_LOG_L:
            kinds = [kind if P.plan(case.n, case.log_l).depth == 1 else "random"]
        else:
            kinds = [kind] + (["random"] if kind != "random" else [])
        runs = []
        for kind in kinds:
            h, zeta = coset_of(env.cv, rng, l, kind, idx % 2 == 1)
            runs.append((h, zeta, expect(env, [p], 1, case.log_l, h, zeta)))
        _WANT[k] = runs
    return _WANT[k]


def check_case(env, idx, case, note=""):
    p = case_poly(env, case)
    arr, lens, stride = pack(env.native, [p])
    key = env.key(case.n)
    l = 1 << case.log_l
    for h, zeta, want in case_runs(env, idx, case, p):
        xy, inf, ev = env.ctx.open_coset(key, arr, lens, stride, case.log_l, h, zeta, 1)
        point, values = got(env, (xy, inf, ev))
        assert len(values) == l
        assert values == want[1], (case.label, note, "values")
        assert point == want[0], (case.label, note, "point")
        if case.n <= l:                                       # no quotient: infinity, the zero-padded polynomial's values
            assert inf[0] == 1 and want[0] is None, (case.label, note)


@pytest.mark.parametrize("curve", CURVES)
def test_every_case_of_the_table(envs, curve):
    """k = 1, xi = 1: the point, the infinity flag and all l values of every shape.  Collects the failures, so that one
    run names every case that is wrong."""
    env = envs[curve]
    failed = []
    for idx, case in enumerate(TABLE):
        try:
            check_case(env, idx, case)
        except AssertionError:
            failed.append((case.label, P.plan(case.n, case.log_l).depth))
    assert not failed, "%d of %d cases (label, depth): %s" % (len(failed), len(TABLE), failed)


# ---- combination and padding ------------------------------------------------------------------------------------------
COMBO_SHAPES = [(0, 273), (3, 256 * 8 + 5), (8, 256 * 256 + 5)]          # three levels, each ragged; the last row short


@pytest.mark.parametrize("log_l,n", COMBO_SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_combination_and_padding(envs, curve, log_l, n):
    """k = 3 with lengths (n, n - l - 1, 1) and k = 17 with lengths falling by 7, polynomial 1 all r - 1, xi in
    {0, 1, r - 1, random}: launch_lincomb pads the last row with zeros over what a LONGER opening left there.  xi = 0
    gives the point at infinity and zero values."""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    l = 1 << log_l
    plan = P.plan(n, log_l)
    assert plan.depth == 3 and all(v.ragged for v in plan.levels) and (l == 1 or n % l)
    rng = random.Random("%s:combo:%d" % (curve, log_l))
    key = env.key(n + 3 * l)
    stale = [rng.getrandbits(253) | 1 for _ in range(n + 3 * l)]             # 2^253 < r on both curves
    stale_arr = pack(native, [stale])[0]
    for lens in ([n, n - l - 1, 1], [n - 7 * i for i in range(17)]):
        polys = [[rng.getrandbits(253) for _ in range(m - 1)] + [rng.randrange(1, r)] for m in lens]
        polys[1] = [r - 1] * lens[1]
        arr, _, stride = pack(native, polys)
        for i, xi in enumerate((0, 1, r - 1, rng.randrange(2, r - 1))):
            h, zeta = coset_of(env.cv, rng, l, "random", i % 2 == 1)
            ctx.open_coset(key, stale_arr, [len(stale)], len(stale), log_l, h, zeta, 1)   # non-zero words up to n + 3 l
            want = expect(env, polys, xi, log_l, h, zeta)
            out = ctx.open_coset(key, arr, lens, stride, log_l, h, zeta, xi)
            assert got(env, out) == want, (len(lens), i)
            if xi == 0:
                assert out[1][0] == 1 and want == (None, [0] * l)


# ---- order on one context ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_l", [0, 3])
@pytest.mark.parametrize("curve", CURVES)
def test_any_order_on_one_context(native, curve, log_l):
    """The cases of one l on a FRESH context, longest first and then shortest first -- the aggregates of a longer
    opening lie in the scratch when a shorter one runs, and the buffers grow on the way up -- with a plain kzg_open and
    a kzg_open_points of other lengths in between (they work in the same buffers).  Every result is the one
    test_every_case_of_the_table expects."""
    ctx = native.Context(curve)
    env = Env(native, curve, ctx=ctx)
    r = env.r
    try:
        mine = sorted(((c.n, idx, c) for idx, c in enumerate(TABLE) if c.log_l == log_l), reverse=True)
        assert len(mine) >= 10 and {P.plan(n, log_l).depth for n, _, _ in mine} >= {1, 2, 3}
        rng = random.Random("%s:order:%d" % (curve, log_l))
        others = []
        for m in (777, 3001):
            q = [rng.randrange(r) for _ in range(m)]
            others.append((pack(native, [q]), q))
        for turn, order in enumerate((mine, mine[::-1])):
            for step, (_, idx, case) in enumerate(order):
                check_case(env, idx, case, note=("order", turn, step))
                (arr, lens, stride), q = others[step % 2]
                z = rng.randrange(1, r)
                if step % 2:
                    ctx.open_points(env.key(len(q)), arr, lens, stride, [z, 1], [[1, 2]])
                else:
                    ev = ctx.open(env.key(len(q)), arr, lens, stride, native.int_to_words(z), native.int_to_words(1))[2]
                    assert native.limbs_to_ints(ev.reshape(1, 4))[0] == O.poly_eval(q, z, r)
    finally:
        env.close()
        ctx.close()


# ---- the device entry point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_the_device_entry_point(envs, curve):
    """kzg_open_coset_device on rows `stride` > n apart with a row of non-zero words after the last polynomial: the
    host twin's results, the expectation's, and not a word of the input changed."""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    rng = random.Random("%s:device" % curve)
    for log_l, n in COMBO_SHAPES[:2]:
        l = 1 << log_l
        polys = [[rng.randrange(r) for _ in range(m - 1)] + [rng.randrange(1, r)] for m in (n, n - l - 3)]
        h, zeta = coset_of(env.cv, rng, l, "random", True)
        xi = rng.randrange(2, r)
        arr, lens, stride = pack(native, polys, stride=n + 11, extra_rows=1)
        assert (arr[2].view(np.uint8) == FILL).all()
        d = to_device(arr)
        key = env.key(n)
        dev = ctx.open_coset(key, d.data_ptr(), lens, stride, log_l, h, zeta, xi, device=True)
        host = ctx.open_coset(key, arr[:2], lens, stride, log_l, h, zeta, xi)
        assert all(np.array_equal(a, b) for a, b in zip(dev, host))
        assert got(env, dev) == expect(env, polys, xi, log_l, h, zeta)
        assert np.array_equal(d.cpu().numpy().view(np.uint64), arr)


# ---- the held slice ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_a_held_sharded_slice_is_dropped(envs, curve):
    """kzg_open_coset works in the opening's buffers: after it kzg_open_shard_finish refuses with KZG_ERR_ARG, as it
    does after kzg_open_points; a new begin is then finished as usual."""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    rng = random.Random("%s:held" % curve)
    polys = [[rng.randrange(r) for _ in range(m)] for m in (3000, 2500)]
    arr, lens, stride = pack(native, polys)
    d = to_device(arr)
    z, xi = rng.randrange(1, r), rng.randrange(1, r)
    zw, xw, none = native.int_to_words(z), native.int_to_words(xi), native.int_to_words(0)
    key = env.key(3000)
    ctx.open_shard_begin(d.data_ptr(), lens, stride, zw, xw)
    first = ctx.open_shard_finish(key, zw, none, True)
    h, zeta = coset_of(env.cv, rng, 8, "random", False)
    small = [polys[0][:300]]
    assert open_host(env, key, small, 3, h, zeta, 1) == expect(env, small, 1, 3, h, zeta)
    with pytest.raises(native.NativeError) as e:
        ctx.open_shard_finish(key, zw, none, True)
    assert e.value.code == KZG_ERR_ARG and "another opening" in str(e.value)
    ctx.open_shard_begin(d.data_ptr(), lens, stride, zw, xw)
    again = ctx.open_shard_finish(key, zw, none, True)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    want, pz = O.poly_divide_linear(O.combine(polys, xi, r), z, r)
    assert env.point(again[0], again[1]) == env.g1_scalar(O.poly_eval(want, env.tau, r))
    assert native.limbs_to_ints(again[2].reshape(1, 4))[0] == pz


# ---- the length rule --------------------------------------------------------------------------------------------------
def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else ctypes.c_void_p(a)


@pytest.mark.parametrize("curve", CURVES)
def test_the_length_rule_as_the_header_states_it(envs, curve):
    """lens[j] above the key is KZG_ERR_DEGREE "before any work is queued": a key of n points takes n coefficients, a
    key of n - 1 refuses them from both entry points with no span recorded and not a byte of out_xy, out_inf and
    eval_out written, and the next call on the context is right.  log_l = 13 likewise, with KZG_ERR_ARG."""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    rng = random.Random("%s:length" % curve)
    log_l, n = 3, 299
    l = 1 << log_l
    polys = [[rng.randrange(r) for _ in range(m - 1)] + [rng.randrange(1, r)] for m in (n, n - 20)]
    xi = rng.randrange(2, r)
    h, zeta = coset_of(env.cv, rng, l, "random", False)
    want = expect(env, polys, xi, log_l, h, zeta)
    arr, lens, stride = pack(native, polys)
    d = to_device(arr)
    lens_a = np.asarray(lens, dtype=np.uint64)
    fits, short = env.key_exact(n), env.key_exact(n - 1)
    hw, zw, xw = (native.int_to_words(v) for v in (h, zeta, xi))

    def raw(name, data, key, lg):
        xy = np.full(2 * ctx.fp_limbs, FILL64, dtype=np.uint64)
        inf = np.full(1, FILL, dtype=np.uint8)
        ev = np.full((1 << lg, 4), FILL64, dtype=np.uint64)
        rc = getattr(native.lib(), name)(ctx._h, key._h, vp(data), vp(lens_a), len(lens), stride, lg, vp(hw), vp(zw),
                                         vp(xw), vp(xy), vp(inf), vp(ev))
        untouched = (xy == FILL64).all() and inf[0] == FILL and (ev == FILL64).all()
        return rc, untouched

    ctx.prof_enable(True)
    try:
        for name, data in (("kzg_open_coset", arr), ("kzg_open_coset_device", d.data_ptr())):
            device = name.endswith("_device")
            assert got(env, ctx.open_coset(fits, data, lens, stride, log_l, h, zeta, xi, device=device)) == want, name
            for key, lg, code in ((short, log_l, native.KZG_ERR_DEGREE), (fits, 13, KZG_ERR_ARG),
                                  (short, 13, KZG_ERR_ARG)):
                ctx.prof_reset()
                assert raw(name, data, key, lg) == (code, True), (name, lg)
                assert ctx.prof_read("open_coset_poly")[1] == 0, (name, lg)
                assert got(env, ctx.open_coset(fits, data, lens, stride, log_l, h, zeta, xi, device=device)) == want
                assert ctx.prof_read("open_coset_poly")[1] == 1, (name, lg)
        with pytest.raises(native.NativeError) as e:
            ctx.open_coset(short, arr, lens, stride, log_l, h, zeta, xi)
        assert e.value.code == native.KZG_ERR_DEGREE and "longer than the commitment key" in str(e.value)
    finally:
        ctx.prof_enable(False)

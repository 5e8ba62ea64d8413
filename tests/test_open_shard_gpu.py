"""The sharded opening (kzg_open_shard_begin / kzg_open_shard_finish, csrc/poly.hip) at every tile plan, carry and
slice edge, rank by rank against the plain-Python restatement (tests/open_shard_restated.py, pinned to the oracle by
tests/test_open_shard_host.py).  One GPU plays every rank.  Integer work: every comparison is exact.

The code's constants the sizes are chosen from: chunks of 8 coefficients, tiles of T = 1024 (128 threads) or 2048 (256
threads), groups of 64 tiles once a slice has more than `open_direct_tiles` tiles, 16 polynomials per combine launch,
six products per Field::dot group.

Tile plans reached, from tile_plan's arithmetic (ntiles = ceil(n / T), gap = ntiles T - n, nsuper = ceil(ntiles / 64)
once ntiles > open_direct_tiles, else 0):

  case (slice n)                               ntiles  gap   nsuper  width  rank
  tile_boundaries  n = T                          1       0    0    128/256  first, middle
  tile_boundaries  n = T + 1                      2     T-1    0    128/256  first, middle
  tile_boundaries  n = 4T + 3                     5     T-3    0    128/256  first, middle
  grouped up       n = 65536, direct 1 / 2       64       0    1      128    first
  grouped up       n = 66560, direct 1 / 2       65       0    2      128    middle
  grouped down     n = 132099, direct 1 / 2     130    1021    3      128    first (carry != 0)
  grouped width 256  n = 132099, direct 1        65    1021    2      256    first
  grouped width 256  n = 66560, direct 1         33    1024    1      256    middle
  ragged ends      [700, e), k = 1 .. 64          2    >500    0      128    middle (k <= 16 and k > 16)
  special points   n = 2053 | 2447 | 500      2 | 2 | 1  2043 | 1649 | 1548  0  256 (the library's choice)
  special points   z = 0                         the copy route of both calls, no tiles
  pending commits  n = 1500 | 1600 | 500         the library's choice (128 while an accumulate kernel is in flight)
  grouping changed n = 1500 | 1600 | 500      2 | 2 | 1  >= 448    1 | 0    128    begin with direct 1, finish with 0, and back"""
import random

import numpy as np
import pytest

from oracle import py_oracle as O
from open_shard_restated import restate_sharded_open

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
KZG_ERR_ARG = -1


class Env:
    """One curve's context, secret and key shards (a shard is generated once per (start, size) and kept)."""

    def __init__(self, native, curve, ctx=None):
        self.native, self.curve, self.cv = native, curve, O.curve(curve)
        self.r = self.cv.r
        self.ctx = ctx or native.get_context(curve)
        self.tau = 0x1d0c5eed0badc0ffee1234567 % self.r
        self.tw = native.int_to_words(self.tau)
        self.G1 = O.from_affine(self.cv.g1)
        self.keys = {}

    def shard(self, g, lo, hi, fresh=False):
        """the key rank g commits its quotient slice against: points start .. hi-2, start = 0 or lo-1 (at least one
        point: a first rank holding one coefficient commits nothing)"""
        start = 0 if g == 0 else lo - 1
        n = max(hi - 1 - start, 1)
        if fresh:
            return self.ctx.srs_generate(self.tw, n, start=start)
        if (start, n) not in self.keys:
            self.keys[(start, n)] = self.ctx.srs_generate(self.tw, n, start=start)
        return self.keys[(start, n)]

    def close(self):
        for k in self.keys.values():
            k.close()
        self.keys = {}


@pytest.fixture(scope="module")
def envs(native):
    out = {c: Env(native, c) for c in CURVES}
    yield out
    for e in out.values():
        e.close()


def upload(native, polys, lo, hi, pad=0):
    """rank [lo, hi)'s slices of every polynomial on the device -> (tensor, slice lengths, stride)"""
    import torch
    stride = hi - lo + pad
    arr = np.zeros((len(polys), stride, 4), dtype=np.uint64)
    lens = []
    for i, p in enumerate(polys):
        part = p[lo:hi]
        lens.append(len(part))
        if part:
            arr[i, :len(part)] = native.ints_to_limbs(part)
    return torch.from_numpy(arr.view(np.int64)).to("cuda:0"), lens, stride


def play_ranks(env, polys, xi, z, bounds, want=None, total=None, pad=0, hook=None, fresh_keys=False):
    """Every rank of one sharded opening on the one GPU: begin on every rank, the host exchange of the H the DEVICE
    returned (as the real job does), then begin + finish on every rank (a context holds one slice at a time).
    Asserts per rank: H, the carry, eval_out, the partial point (or its infinity flag); then the sum of the points.
    hook(stage, g) runs before "begin2" / "finish" of rank g.  -> [(H, ev, affine point or None)] per rank."""
    native, ctx, cv, r = env.native, env.ctx, env.cv, env.r
    L = ctx.fp_limbs
    if want is None:
        want = restate_sharded_open(polys, xi, z, bounds, env.tau, r)
    zw, xw = native.int_to_words(z), native.int_to_words(xi)
    ranges = list(zip(bounds, bounds[1:]))
    dev = [upload(native, polys, lo, hi, pad) for lo, hi in ranges]
    H = []
    for g, (t, lens, stride) in enumerate(dev):
        h = native.limbs_to_ints(ctx.open_shard_begin(t.data_ptr(), lens, stride, zw, xw).reshape(1, 4))[0]
        assert h == want.H[g], ("H", g, ranges[g])
        H.append(h)
    carries = [sum(H[g2] * pow(z, ranges[g2][0] - hi, r) for g2 in range(g + 1, len(ranges))) % r
               for g, (lo, hi) in enumerate(ranges)]
    out, acc = [], O.Z1()
    for g, (lo, hi) in enumerate(ranges):
        assert carries[g] == want.carry[g], ("carry", g, ranges[g])
        t, lens, stride = dev[g]
        if hook:
            hook("begin2", g)
        h = native.limbs_to_ints(ctx.open_shard_begin(t.data_ptr(), lens, stride, zw, xw).reshape(1, 4))[0]
        assert h == want.H[g], ("H again", g, ranges[g])
        key = env.shard(g, lo, hi, fresh=fresh_keys)           # the real call order: the shard between the two calls
        if hook:
            hook("finish", g)
        xy, inf, ev = ctx.open_shard_finish(key, zw, native.int_to_words(carries[g]), g == 0)
        if fresh_keys:
            key.close()
        ev = native.limbs_to_ints(ev.reshape(1, 4))[0]
        assert ev == want.ev[g], ("ev", g, ranges[g])
        pt = None if inf[0] else tuple(native.limbs_to_ints(xy.reshape(2, L)))
        assert pt == O.normalize(O.multiply(env.G1, want.scalar[g], cv), cv), ("point", g, ranges[g])
        if want.scalar[g] == 0:
            assert inf[0] == 1, ("infinity flag", g)
        if pt is not None:
            acc = O.add(acc, O.from_affine(pt), cv)
        out.append((h, ev, pt))
    assert O.normalize(acc, cv) == O.normalize(O.multiply(env.G1, sum(want.scalar) % r, cv), cv), "sum of the points"
    if z != env.tau:                                            # (c(tau) - c(z)) / (tau - z) has a value
        if total is None:
            total = O.normalize(O.open_trapdoor(polys, z, xi, env.tau, cv), cv)
        assert O.normalize(acc, cv) == total, "trapdoor identity"
    return out


def mixed_polys(rng, r, lens, salt=0):
    """r-1 / random / alternating r-1 and 0, as the unsharded tile test mixes them"""
    polys = []
    for i, m in enumerate(lens):
        kind = (i + salt) % 3
        polys.append([r - 1] * m if kind == 0 else [rng.randrange(r) for _ in range(m)] if kind == 1
                     else [(r - 1) if j % 2 else 0 for j in range(m)])
    return polys


def reset_tuning(ctx):
    ctx.set_tuning("open_tile_threads", 0)
    ctx.set_tuning("open_direct_tiles", 0)


# ---- a. tile boundaries of the slice ----------------------------------------------------------------------------------
@pytest.mark.parametrize("position", ["middle", "first"])
@pytest.mark.parametrize("tb", [128, 256])
@pytest.mark.parametrize("curve", CURVES)
def test_shard_slice_at_the_tile_boundaries(envs, curve, tb, position):
    """A slice of 1 .. 4T+3 coefficients as a middle rank (slices of 11 below and 21 above) and as the first rank (21
    above), both tile widths: gap 0 (T, 2T) and T-1 (T+1, 2T+1), a full (8, T, 2T) and a partial end chunk, the carry
    reaching tile 0 through 1 .. 5 tiles.  (z, xi) = (r-1, r-1) on odd lengths."""
    env = envs[curve]
    r, T = env.r, 8 * tb
    rng = random.Random(1000 + tb)
    try:
        env.ctx.set_tuning("open_tile_threads", tb)
        for n in (1, 7, 8, 9, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 5, 4 * T + 3):
            bounds = [0, 11, 11 + n, 11 + n + 21] if position == "middle" else [0, n, n + 21]
            N = bounds[-1]
            polys = mixed_polys(rng, r, [N, N - 3, N - 6], salt=n)
            z, xi = (r - 1, r - 1) if n % 2 else (rng.randrange(1, r), rng.randrange(r))
            play_ranks(env, polys, xi, z, bounds)
    finally:
        reset_tuning(env.ctx)


# ---- b. the carry together with grouped aggregates -------------------------------------------------------------------
GROUP_T = 1024
GROUP_SLICES = (64 * GROUP_T, 65 * GROUP_T, 129 * GROUP_T + 3)     # one full group | 64 + 1 tiles | 130 tiles, 3 groups


def group_bounds(order):
    sl = GROUP_SLICES if order == "up" else GROUP_SLICES[::-1]
    return [0, sl[0], sl[0] + sl[1], sl[0] + sl[1] + sl[2]]


@pytest.fixture(scope="module")
def grouped(envs):
    """per curve: two polynomials of 258 * 1024 + 3 and five fewer coefficients, one (z, xi), and for both orders of
    the three slices the restatement and the trapdoor total -- computed once, read by every grouped test"""
    cache = {}

    def get(curve):
        if curve not in cache:
            env = envs[curve]
            r = env.r
            rng = random.Random(4242)
            N = sum(GROUP_SLICES)
            polys = [[rng.getrandbits(253) for _ in range(m)] for m in (N, N - 5)]
            for j in range(0, N - 5, 4099):
                polys[0][j], polys[1][j] = r - 1, 0
            z, xi = rng.randrange(2, r), rng.randrange(1, r)
            total = O.normalize(O.open_trapdoor(polys, z, xi, env.tau, env.cv), env.cv)
            want = {o: restate_sharded_open(polys, xi, z, group_bounds(o), env.tau, r) for o in ("up", "down")}
            cache[curve] = (polys, z, xi, total, want)
        return cache[curve]
    return get


@pytest.mark.parametrize("order", ["up", "down"])
@pytest.mark.parametrize("curve", CURVES)
def test_shard_carry_with_grouped_aggregates(envs, grouped, curve, order):
    """Width 128, `open_direct_tiles` = 1 and 2: every rank sums its own group's tiles, the groups above (A) and the
    carry of the virtual tile (has_hv) -- 64 tiles (one full group, gap 0), 65 (a second group of one tile) and 130
    (three groups, gap 1021), in both orders so that each is once the first rank and once the top one.  The same
    slices ungrouped give the same H, eval_out and points."""
    env = envs[curve]
    polys, z, xi, total, want = grouped(curve)
    try:
        env.ctx.set_tuning("open_tile_threads", 128)
        got = {}
        for direct in (1, 2, 0):
            env.ctx.set_tuning("open_direct_tiles", direct)
            got[direct] = play_ranks(env, polys, xi, z, group_bounds(order), want=want[order], total=total)
        assert got[1] == got[0] and got[2] == got[0]
    finally:
        reset_tuning(env.ctx)


@pytest.mark.parametrize("curve", CURVES)
def test_shard_carry_with_grouped_aggregates_width_256(envs, grouped, curve):
    """The same slices in tiles of 2048: 65 tiles in two groups with gap 1021 on the first rank, then 33 tiles (gap
    1024) and 32 (gap 0) in one group each."""
    env = envs[curve]
    polys, z, xi, total, want = grouped(curve)
    try:
        env.ctx.set_tuning("open_tile_threads", 256)
        got = {}
        for direct in (1, 0):
            env.ctx.set_tuning("open_direct_tiles", direct)
            got[direct] = play_ranks(env, polys, xi, z, group_bounds("down"), want=want["down"], total=total)
        assert got[1] == got[0]
    finally:
        reset_tuning(env.ctx)


# ---- c. polynomial counts and ragged ends ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,pad", [(1, 0), (6, 0), (7, 5), (12, 0), (13, 0), (16, 0), (17, 3000), (64, 0)])
@pytest.mark.parametrize("curve", CURVES)
def test_shard_polynomial_counts_and_ragged_ends(envs, curve, k, pad):
    """k polynomials of n - 3i coefficients (one to eleven Field::dot groups, the pre-combined form beyond sixteen)
    over [0, 700, e, n + 5, n + 9), e = the length of polynomial k // 2: that one ends on the boundary, the shorter
    ones strictly inside [700, e) and are empty above, the longer ones strictly inside [e, n + 5), and the top rank
    holds nothing: begin returns 0 there, finish the point at infinity and a zero eval_out, and the rank below
    receives carry 0.  pad: a stride larger than the slice."""
    env = envs[curve]
    r, n = env.r, 2300
    rng = random.Random(100 + k)
    lens = [n - 3 * i for i in range(k)]
    bounds = [0, 700, lens[k // 2], n + 5, n + 9]
    polys = mixed_polys(rng, r, lens, salt=k)
    z, xi = rng.randrange(2, r), rng.randrange(1, r)
    try:
        env.ctx.set_tuning("open_tile_threads", 128)          # [700, e) is a slice of two tiles
        got = play_ranks(env, polys, xi, z, bounds, pad=pad)
    finally:
        reset_tuning(env.ctx)
    assert got[-1] == (0, 0, None)


# ---- d. special points -----------------------------------------------------------------------------------------------
SPECIAL_BOUNDS = [0, 2053, 4500, 5000]            # default width: two tiles (gap 2043), two tiles (gap 1649), one


def special_case(name, env):
    r = env.r
    rng = random.Random(31)
    polys = [[rng.randrange(r) for _ in range(m)] for m in (5000, 4997, 3100)]
    z, xi = rng.randrange(2, r), rng.randrange(1, r)
    xinv = pow(xi, -1, r)
    if name == "z_zero":
        z = 0
    elif name == "z_one":
        z = 1
    elif name == "z_minus_one":
        z = r - 1
    elif name == "z_tau":
        z = env.tau
    elif name == "root_at_z":
        pz = O.poly_eval(O.combine(polys, xi, r), z, r)
        polys[0][0] = (polys[0][0] - pz * xinv) % r
    elif name == "zero_above":
        for p in polys:
            for j in range(4500, len(p)):
                p[j] = 0
    elif name == "carry_minus_one":
        s = restate_sharded_open(polys, xi, z, SPECIAL_BOUNDS, env.tau, r).S[4500]
        polys[0][4500] = (polys[0][4500] + (r - 1 - s) * xinv) % r
    return polys, z, xi


@pytest.mark.parametrize("name", ["z_zero", "z_one", "z_minus_one", "z_tau", "root_at_z", "zero_above",
                                  "carry_minus_one"])
@pytest.mark.parametrize("curve", CURVES)
def test_shard_special_points(envs, curve, name):
    """z = 0 (the copy route of both calls: the ranks above return non-zero H, the carry handed down is c_hi and
    must not enter), z = 1, z = r-1, z = tau (no trapdoor total there: the per-rank scalars stand), a root at z
    (S_0 = 0), all-zero coefficients above 4500 (carry 0 on a rank that is not the last) and a carry of r-1."""
    env = envs[curve]
    polys, z, xi = special_case(name, env)
    want = restate_sharded_open(polys, xi, z, SPECIAL_BOUNDS, env.tau, env.r)
    if name == "z_zero":
        assert want.H[1] and want.H[2] and want.carry[0] and want.carry[1]
    elif name == "root_at_z":
        assert want.S[0] == 0 and want.ev[0] == 0
    elif name == "zero_above":
        assert want.carry[1] == 0 and want.H[2] == 0 and want.carry[0] != 0
    elif name == "carry_minus_one":
        assert want.carry[1] == env.r - 1
    play_ranks(env, polys, xi, z, SPECIAL_BOUNDS, want=want)


# ---- e. state between the two calls ---------------------------------------------------------------------------------
STATE_BOUNDS = [0, 1500, 3100, 3600]              # 1500 and 1600: two tiles of 1024, one of 2048


def state_case(env, seed=8):
    rng = random.Random(seed)
    polys = [[rng.randrange(env.r) for _ in range(m)] for m in (3600, 3333)]
    return polys, rng.randrange(2, env.r), rng.randrange(1, env.r)


@pytest.mark.parametrize("tb_begin,tb_finish", [(128, 256), (256, 128)])
@pytest.mark.parametrize("curve", CURVES)
def test_shard_finish_uses_the_width_begin_recorded(envs, curve, tb_begin, tb_finish):
    """`open_tile_threads` changed between begin and finish: the aggregates on the device were formed with begin's
    tiles, and finish fills with those."""
    env = envs[curve]
    polys, z, xi = state_case(env)

    def hook(stage, g):
        env.ctx.set_tuning("open_tile_threads", tb_begin if stage == "begin2" else tb_finish)
    try:
        play_ranks(env, polys, xi, z, STATE_BOUNDS, hook=hook)
    finally:
        reset_tuning(env.ctx)


@pytest.mark.parametrize("curve", CURVES)
def test_shard_finish_continues_the_last_begin(envs, curve):
    """begin on another slice (other length, other point) right before each rank's own begin: finish returns the
    result of the LAST begin.  The key shard is generated between begin and finish, as the real job does."""
    env = envs[curve]
    native, ctx = env.native, env.ctx
    polys, z, xi = state_case(env)
    other, oz, oxi = state_case(env, seed=9)
    t, lens, stride = upload(native, other, 100, 2900)

    def hook(stage, g):
        if stage == "begin2":
            ctx.open_shard_begin(t.data_ptr(), lens, stride, native.int_to_words(oz), native.int_to_words(oxi))
    play_ranks(env, polys, xi, z, STATE_BOUNDS, hook=hook, fresh_keys=True)


@pytest.mark.parametrize("direct_begin,direct_finish", [(0, 1), (1, 0)])
@pytest.mark.parametrize("curve", CURVES)
def test_shard_finish_uses_the_grouping_begin_recorded(envs, curve, direct_begin, direct_finish):
    """`open_direct_tiles` changed between begin and finish, width 128 (slices of two, two and one tiles: with the
    value 1 the two-tile slices sum through one group aggregate, with 0 they do not).  A begin on another slice with
    grouping on runs first, so that a foreign group aggregate lies where finish would look for one; finish fills
    from the shape begin left, whatever the tuning says by then."""
    env = envs[curve]
    native, ctx = env.native, env.ctx
    polys, z, xi = state_case(env)
    other, oz, oxi = state_case(env, seed=9)
    t, lens, stride = upload(native, other, 100, 2900)

    def hook(stage, g):
        if stage == "begin2":
            ctx.set_tuning("open_direct_tiles", 1)
            ctx.open_shard_begin(t.data_ptr(), lens, stride, native.int_to_words(oz), native.int_to_words(oxi))
            ctx.set_tuning("open_direct_tiles", direct_begin)
        else:
            ctx.set_tuning("open_direct_tiles", direct_finish)
    try:
        ctx.set_tuning("open_tile_threads", 128)
        play_ranks(env, polys, xi, z, STATE_BOUNDS, hook=hook)
    finally:
        reset_tuning(ctx)


def refused_finish(env, key, z, first_rank):
    """finish is KZG_ERR_ARG -> the message"""
    native = env.native
    with pytest.raises(native.NativeError) as e:
        env.ctx.open_shard_finish(key, native.int_to_words(z), native.int_to_words(7), first_rank)
    assert e.value.code == KZG_ERR_ARG
    return str(e.value)


@pytest.mark.parametrize("curve", CURVES)
def test_shard_finish_with_another_z_is_refused(envs, curve):
    """finish must be given begin's z: another one is an argument error whose message names z, the slice stays, and
    the same finish with begin's z returns the restated result."""
    env = envs[curve]
    polys, z, xi = state_case(env)

    def hook(stage, g):
        if stage == "finish":
            key = env.shard(g, STATE_BOUNDS[g], STATE_BOUNDS[g + 1])
            for wrong in ((z + 1) % env.r, 0):
                assert "z differs" in refused_finish(env, key, wrong, g == 0)
    play_ranks(env, polys, xi, z, STATE_BOUNDS, hook=hook)


@pytest.mark.parametrize("between", ["open", "open_coset"])
@pytest.mark.parametrize("curve", CURVES)
def test_shard_finish_after_another_opening_is_refused(envs, curve, between):
    """kzg_open_device / kzg_open_coset_device between begin and finish overwrite what begin left: finish is an
    argument error that says so (not the "never begun" one), and the context then completes a sharded opening."""
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    polys, z, xi = state_case(env)
    zw, xw = native.int_to_words(z), native.int_to_words(xi)
    t, lens, stride = upload(native, polys, 0, 1500)
    ctx.open_shard_begin(t.data_ptr(), lens, stride, zw, xw)
    if between == "open":
        key = ctx.srs_generate(env.tw, 1600)
        ev = ctx.open(key, t.data_ptr(), lens, stride, zw, xw, device=True)[2]
        assert native.limbs_to_ints(ev.reshape(1, 4))[0] == O.poly_eval(O.combine([p[:1500] for p in polys], xi, r), z, r)
    else:
        key = ctx.srs_generate(env.tw, 64)
        t64, lens64, stride64 = upload(native, polys, 0, 64)
        ctx.open_coset(key, t64.data_ptr(), lens64, stride64, 1, 5, r - 1, xi, device=True)
    try:
        msg = refused_finish(env, key, z, True)
        assert "another opening" in msg and "without kzg_open_shard_begin" not in msg
    finally:
        key.close()
    play_ranks(env, polys, xi, z, STATE_BOUNDS)


@pytest.mark.parametrize("curve", CURVES)
def test_shard_slice_is_kept_across_other_calls(envs, curve):
    """kzg_fr_poly_eval (3000 coefficients: two tiles of 2048, its own plan in its own buffers), a prefix product of
    100 elements and a change of `open_tile_threads` between begin and finish: each gives its own result and the
    slice stands.  (Key generation and commits in between: test_shard_finish_continues_the_last_begin,
    test_shard_begin_beside_pending_async_commits.)"""
    import torch
    env = envs[curve]
    native, ctx, r = env.native, env.ctx, env.r
    polys, z, xi = state_case(env)
    rng = random.Random(77)
    vec = [rng.randrange(r) for _ in range(3000)]
    d_vec = upload(native, [vec], 0, 3000)[0]
    pz = rng.randrange(2, r)
    want_eval = O.poly_eval(vec, pz, r)
    want_prefix, acc = [], 1
    for y in vec[:100]:
        want_prefix.append(acc)
        acc = acc * y % r
    d_out = torch.zeros((100, 4), dtype=torch.int64, device="cuda:0")

    def hook(stage, g):
        if stage == "finish":
            assert ctx.poly_eval(3000, d_vec.data_ptr(), pz) == want_eval
            ctx.vec_prefix_product(100, d_vec.data_ptr(), d_out.data_ptr())
            ctx.synchronize()
            assert native.limbs_to_ints(d_out.cpu().numpy().view(np.uint64)) == want_prefix
            ctx.set_tuning("open_tile_threads", 256 if g % 2 else 128)
    try:
        play_ranks(env, polys, xi, z, STATE_BOUNDS, hook=hook)
    finally:
        reset_tuning(ctx)


@pytest.mark.parametrize("curve", CURVES)
def test_shard_begin_that_fails_leaves_no_slice(envs, curve):
    """A begin refused for its arguments (lens[0] > stride) after a good begin: the earlier slice is gone, finish is
    an argument error."""
    env = envs[curve]
    native, ctx = env.native, env.ctx
    polys, z, xi = state_case(env)
    zw, xw = native.int_to_words(z), native.int_to_words(xi)
    t, lens, stride = upload(native, polys, 0, 1500)
    ctx.open_shard_begin(t.data_ptr(), lens, stride, zw, xw)
    with pytest.raises(native.NativeError) as e:
        ctx.open_shard_begin(t.data_ptr(), [stride + 1, lens[1]], stride, zw, xw)
    assert e.value.code == KZG_ERR_ARG
    refused_finish(env, env.shard(0, 0, 1500), z, True)


@pytest.mark.parametrize("curve", CURVES)
def test_shard_finish_twice_after_one_begin(envs, curve):
    """finish does not consume the slice: every rank finishes twice after its one begin, and both calls return the
    same eval_out and point -- the restated ones."""
    env = envs[curve]
    native, ctx = env.native, env.ctx
    polys, z, xi = state_case(env)
    want = restate_sharded_open(polys, xi, z, STATE_BOUNDS, env.tau, env.r)
    first = []

    def hook(stage, g):
        if stage == "finish":
            key = env.shard(g, STATE_BOUNDS[g], STATE_BOUNDS[g + 1])
            xy, inf, ev = ctx.open_shard_finish(key, native.int_to_words(z), native.int_to_words(want.carry[g]), g == 0)
            first.append((native.limbs_to_ints(ev.reshape(1, 4))[0],
                          None if inf[0] else tuple(native.limbs_to_ints(xy.reshape(2, ctx.fp_limbs)))))
    second = play_ranks(env, polys, xi, z, STATE_BOUNDS, want=want, hook=hook)
    assert first == [(ev, pt) for _, ev, pt in second]


@pytest.mark.parametrize("curve", CURVES)
def test_shard_finish_without_begin_is_refused(native, curve):
    """A fresh context has no slice: finish is an argument error (not an empty result), and the context then
    completes a sharded opening."""
    ctx = native.Context(curve)
    env = Env(native, curve, ctx=ctx)
    try:
        key = env.shard(0, 0, 1500)
        z = native.int_to_words(12345)
        with pytest.raises(native.NativeError) as e:
            ctx.open_shard_finish(key, z, native.int_to_words(7), True)
        assert e.value.code == KZG_ERR_ARG and "without kzg_open_shard_begin" in str(e.value)
        with pytest.raises(native.NativeError) as e:
            ctx.open_shard_finish(key, z, native.int_to_words(0), False)
        assert e.value.code == KZG_ERR_ARG
        polys, z, xi = state_case(env)
        play_ranks(env, polys, xi, z, STATE_BOUNDS)
    finally:
        env.close()
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_shard_begin_beside_pending_async_commits(envs, curve):
    """Every rank's begin runs right behind a pipelined commit of 2^16 + 5 coefficients (the tile width is then the
    library's own choice: 128 while an accumulate kernel is in flight), the pipeline is flushed, then finish: the
    opening is what the restatement says and the pending commitments equal their synchronous values."""
    import torch
    env = envs[curve]
    native, ctx = env.native, env.ctx
    L = ctx.fp_limbs
    n = (1 << 16) + 5
    srs = env.shard(0, 0, n + 1)
    g = torch.Generator(device="cuda:0").manual_seed(17)
    d = torch.randint(0, 1 << 62, (n, 4), generator=g, dtype=torch.int64, device="cuda:0")
    d[..., 3] >>= 3
    torch.cuda.synchronize()
    want_xy, want_inf = ctx.commit_device(srs, d.data_ptr(), [n], n)
    polys, z, xi = state_case(env)
    pending = []

    def hook(stage, g):
        if stage == "begin2":
            out = (np.zeros((1, 2 * L), dtype=np.uint64), np.zeros(1, dtype=np.uint8))
            ctx.commit_device_async(srs, d.data_ptr(), [n], n, *out)
            pending.append(out)
        else:
            ctx.commit_flush()
    try:
        play_ranks(env, polys, xi, z, STATE_BOUNDS, hook=hook)
    finally:
        ctx.commit_flush()
    assert len(pending) == 3
    for xy, inf in pending:
        assert np.array_equal(xy, want_xy) and inf[0] == want_inf[0] == 0


# ---- f. spans ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_two_open_shard_poly_spans_per_begin_finish_pair(envs, curve):
    """include/kzg_mi355x.h: "open_shard_poly" counts one span per kzg_open_shard_begin and one per _finish"""
    env = envs[curve]
    native, ctx = env.native, env.ctx
    polys, z, xi = state_case(env)
    t, lens, stride = upload(native, polys, 0, 3600)
    key = env.shard(0, 0, 3600)
    zw, xw = native.int_to_words(z), native.int_to_words(xi)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for pairs in (1, 2, 3):
            ctx.open_shard_begin(t.data_ptr(), lens, stride, zw, xw)
            ctx.open_shard_finish(key, zw, native.int_to_words(0), True)
            ms, cnt = ctx.prof_read("open_shard_poly")
            assert cnt == 2 * pairs and ms > 0
    finally:
        ctx.prof_enable(False)

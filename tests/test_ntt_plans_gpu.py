"""Every launch plan of the NTT (launch_passes in csrc/ntt.hip) and batches above one, bit-exact.

ntt_pass_kernel is one generic kernel; a call fixes the line length k, the lines per tile logC, the thread count, the
pair_tiles remap of blockIdx, the load order and the epilogue from log_n, the tile preference (ntt_tile_log 8..12), the
direction and the batch (blockIdx.y).  The tests here walk that space: every single-pass size, every two-pass split up to
2^19 under every tile preference, the three sizes whose halves are 11 and 12 levels long, batches with a guard vector
behind them, and -- in child processes, since the library reads them once -- the two environment-selected paths.

References: oracle/kzg_oracle.c (the recursion of fft_ff.py:15-37 / :51-58 as written) up to 2^19; above it
oracle/fast_cpu.cpp on several threads, which tests/test_fast_cpu.py pins to that oracle at 2^13 and 2^19.  Inputs span
[0, r) with r-1, r-2, 0, 1 planted (ntt_helpers.edge_vector).  No tolerance anywhere: np.array_equal on the limbs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import fast_cpu as FC
from oracle import py_oracle as O
from ntt_helpers import assert_same, edge_vector, transform_on_device

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CURVES = ["bls12_381", "bn254"]
TILE_LOGS = (8, 9, 10, 11, 12)
ANY_W = 0x123456789abcdef0fedcba9876543210f00dfeed          # no root of unity in either field


def _vectors(native, curve, log_n, count=1):
    """`count` different edge-planted vectors of 2^log_n elements, one after the other"""
    rs = np.random.RandomState(7000 + 64 * log_n + CURVES.index(curve))
    r = O.curve(curve).r
    return np.concatenate([edge_vector(rs, 1 << log_n, r, native, turn=v) for v in range(count)])


def _fast_cpu(curve, raw, w, inverse):
    return FC.ntt(curve, raw.copy(), w, inverse=inverse, threads=min(FC.max_threads(), 16))


def _forced(native, ctx, tile_log, raw, log_n, w, inverse, batch=1):
    """one transform under set_tuning("ntt_tile_log", tile_log); 0 leaves the choice to the library"""
    ctx.set_tuning("ntt_tile_log", tile_log)
    try:
        got = transform_on_device(native, ctx, raw, log_n, w, inverse, batch)
        if tile_log:
            assert ctx.prof_read("ntt_tile_log")[0] == tile_log
    finally:
        ctx.set_tuning("ntt_tile_log", 0)
    return got


# ---- 1. the plan matrix ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", range(1, 13))
def test_single_pass_every_size(native, curve, log_n):
    """log_n 1..12: one tile, k = log_n, 64 .. 1024 threads, odd k through the leading radix-2 level; forward
    (EPI_REDUCE) and inverse (EPI_SCALE)."""
    w = O.curve(curve).root_of_unity(1 << log_n)
    raw = _vectors(native, curve, log_n)
    ctx = native.get_context(curve)
    for inverse in (False, True):
        want = CO.fft(curve, raw.copy(), w, inverse=inverse)
        assert_same(transform_on_device(native, ctx, raw, log_n, w, inverse), want, (curve, log_n, inverse))


@pytest.mark.parametrize("curve", CURVES)
def test_one_element_is_left_alone(native, curve):
    """log_n = 0 (fft_ff.py:16-17 returns the input; 1^-1 = 1): KZG_OK and no byte written, whatever w is"""
    r = O.curve(curve).r
    raw = native.ints_to_limbs([r - 1, r - 2]).copy()            # the element and the one behind it
    ctx = native.get_context(curve)
    for w in (1, ANY_W % r):
        for inverse in (False, True):
            got = transform_on_device(native, ctx, raw, 0, w, inverse)       # raises unless the call returns KZG_OK
            assert np.array_equal(got, raw), (w, inverse)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", range(13, 20))
def test_two_pass_every_tile_preference(native, curve, log_n):
    """log_n 13..19, the splits (k1, k2) = (7,6) .. (10,9), forward and inverse, under ntt_tile_log 8, 9, 10, 11, 12
    and the library's own choice: tiles of 64 and 128 threads, logC from 0 (with the pair_tiles remap, g = 2) over 1
    (g = 1) to 6, lines longer than the preferred tile (tl = k)."""
    w = O.curve(curve).root_of_unity(1 << log_n)
    raw = _vectors(native, curve, log_n)
    ctx = native.get_context(curve)
    for inverse in (False, True):
        want = CO.fft(curve, raw.copy(), w, inverse=inverse)      # once per direction, shared by the tile logs
        for tile_log in TILE_LOGS + (0,):
            got = _forced(native, ctx, tile_log, raw, log_n, w, inverse)
            assert_same(got, want, (curve, log_n, inverse, "tile_log", tile_log))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", range(14, 20))
def test_two_pass_twist_for_any_w(native, curve, log_n):
    """The factor-table twist w^(t*v) = twA[e >> h] * twB[e & (2^h - 1)] is an identity for every w: a w that is no
    root of unity and one of order 2n, forward, at the library's own tile."""
    cv = O.curve(curve)
    raw = _vectors(native, curve, log_n)
    ctx = native.get_context(curve)
    for w in (ANY_W % cv.r, cv.root_of_unity(2 << log_n)):
        want = CO.fft(curve, raw.copy(), w, inverse=False)
        assert_same(transform_on_device(native, ctx, raw, log_n, w, False), want, (curve, log_n, hex(w)[:12]))


@pytest.mark.parametrize("log_n", [21, 22, 23])
def test_long_lines_against_the_threaded_cpu_transform(native, log_n):
    """2^21, 2^22, 2^23: the only sizes with lines of 2^11 and 2^12 elements where k1 != k2 ((11,10), (11,11), (12,11)),
    so a 2048-element preference is overridden by the line in one pass or both.  BLS12-381, forward and inverse, the
    library's tile and 4096-element tiles, against oracle/fast_cpu.cpp (one upload; the working copy is refilled on
    the device)."""
    import torch
    curve = "bls12_381"
    w = O.curve(curve).root_of_unity(1 << log_n)
    raw = _vectors(native, curve, log_n)
    ctx = native.get_context(curve)
    src = torch.from_numpy(raw.view(np.int64)).to("cuda:0")
    work = torch.empty_like(src)
    for inverse in (False, True):
        want = _fast_cpu(curve, raw, w, inverse)
        for tile_log in (0, 12):
            work.copy_(src)
            torch.cuda.synchronize()         # torch's stream wrote it; the context runs on a stream of its own
            ctx.set_tuning("ntt_tile_log", tile_log)
            try:
                ctx.ntt_device(work.data_ptr(), log_n, native.int_to_words(w), inverse, 1)
                ctx.synchronize()
                if tile_log:
                    assert ctx.prof_read("ntt_tile_log")[0] == tile_log
            finally:
                ctx.set_tuning("ntt_tile_log", 0)
            assert_same(work.cpu().numpy().view(np.uint64), want, (log_n, inverse, "tile_log", tile_log))


# ---- 2. batches -----------------------------------------------------------------------------------------------------

BATCHES = (2, 3, 8)
BATCH_LOGS = (1, 6, 12, 13, 14, 16)      # a tile of one butterfly, 64 elements, the single-pass limit, an odd split, even splits


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("inverse", [False, True])
def test_batches_with_a_guard_vector(native, curve, inverse):
    """kzg_ntt_device with batch 2, 3 and 8 on allocations of batch + 1 different vectors: each of the first `batch`
    must equal the oracle's transform of that vector alone (batch_stride, and for two passes the scratch offset of
    vector 1..), the last must come back as it went in.  At 2^13 also under 256- and 4096-element tiles.  All calls
    are queued on one fresh context in the order of growing n * batch, so that ntt_scratch is outgrown again and again
    with transforms still queued, and the context is synchronised once, after the last."""
    import torch
    w_of = {log_n: O.curve(curve).root_of_unity(1 << log_n) for log_n in BATCH_LOGS}
    hosts = {log_n: _vectors(native, curve, log_n, max(BATCHES) + 1) for log_n in BATCH_LOGS}
    wants = {}
    for log_n in BATCH_LOGS:
        n = 1 << log_n
        wants[log_n] = np.concatenate([CO.fft(curve, hosts[log_n][v * n:(v + 1) * n].copy(), w_of[log_n], inverse=inverse)
                                       for v in range(max(BATCHES))])
    calls = [(log_n, batch, 0) for log_n in BATCH_LOGS for batch in BATCHES]
    calls += [(13, batch, tile_log) for batch in BATCHES for tile_log in (8, 12)]
    calls.sort(key=lambda c: (c[1] << c[0], c[2]))
    bufs = [torch.from_numpy(hosts[log_n][:(batch + 1) << log_n].view(np.int64)).to("cuda:0") for log_n, batch, _ in calls]
    torch.cuda.synchronize()                 # torch's stream wrote them; the context runs on a stream of its own
    ctx = native.Context(curve)
    try:
        for (log_n, batch, tile_log), d in zip(calls, bufs):
            ctx.set_tuning("ntt_tile_log", tile_log)
            ctx.ntt_device(d.data_ptr(), log_n, native.int_to_words(w_of[log_n]), inverse, batch)
            if tile_log:
                assert ctx.prof_read("ntt_tile_log")[0] == tile_log
        ctx.synchronize()
        for (log_n, batch, tile_log), d in zip(calls, bufs):
            n = 1 << log_n
            got = d.cpu().numpy().view(np.uint64)
            what = (curve, inverse, "log_n", log_n, "batch", batch, "tile_log", tile_log)
            assert_same(got[:batch * n], wants[log_n][:batch * n], what)
            assert np.array_equal(got[batch * n:], hosts[log_n][batch * n:(batch + 1) * n]), what + ("guard vector",)
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_an_empty_batch_touches_nothing(native, curve):
    """batch = 0: KZG_OK, and neither a single-pass nor a two-pass size writes a byte"""
    ctx = native.get_context(curve)
    for log_n in (6, 13):
        raw = _vectors(native, curve, log_n)
        w = O.curve(curve).root_of_unity(1 << log_n)
        for inverse in (False, True):
            got = transform_on_device(native, ctx, raw, log_n, w, inverse, batch=0)   # raises unless KZG_OK
            assert np.array_equal(got, raw), (log_n, inverse)


def test_the_headline_launch_2_20_batch_4_inverse(native):
    """What the benchmark's headline loop launches -- ntt_device(work, 20, w, True, 4) on BLS12-381 -- with each of the
    four vectors against oracle/fast_cpu.cpp and a fifth vector behind them that must not change."""
    curve, log_n, batch = "bls12_381", 20, 4
    n = 1 << log_n
    w = O.curve(curve).root_of_unity(n)
    raw = _vectors(native, curve, log_n, batch + 1)
    got = transform_on_device(native, native.get_context(curve), raw, log_n, w, True, batch)
    for v in range(batch):
        assert_same(got[v * n:(v + 1) * n], _fast_cpu(curve, raw[v * n:(v + 1) * n], w, True), ("vector", v))
    assert np.array_equal(got[batch * n:], raw[batch * n:]), "guard vector"


# ---- 3. the paths selected by the environment ------------------------------------------------------------------------

def _run_child(body, variable, value):
    """tests/ntt_env_child.<body>() in a fresh interpreter with `variable` set in ITS environment only: the library
    reads KZG_NTT_TWIST_TABLE and KZG_NTT_TILE_LOG once, into statics, so this process cannot switch them"""
    env = {k: v for k, v in os.environ.items() if k not in ("KZG_NTT_TWIST_TABLE", "KZG_NTT_TILE_LOG")}
    env[variable] = value
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import ntt_env_child; ntt_env_child.{body}()"
    done = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=600, capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert done.stdout.strip().endswith(f"{body} ok"), done.stdout[-2000:]


def test_full_twist_table_in_a_child_process():
    """KZG_NTT_TWIST_TABLE=1 (EPI_TABLE, two of the eight instantiations per curve): whole transforms at 2^13 and 2^14,
    the distributed column pass with its col_base term, and the refusal of the rows-twist pass, which needs the factor
    tables.  See ntt_env_child.twist_table."""
    _run_child("twist_table", "KZG_NTT_TWIST_TABLE", "1")


def test_tile_log_from_the_environment_in_a_child_process():
    """KZG_NTT_TILE_LOG=9: taken when nothing is tuned, overridden by set_tuning, back after tuning 0.  See
    ntt_env_child.tile_log_9."""
    _run_child("tile_log_9", "KZG_NTT_TILE_LOG", "9")

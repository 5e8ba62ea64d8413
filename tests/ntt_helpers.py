"""Shared by the at-size NTT tests (test_ntt_gpu.py, test_ntt_plans_gpu.py and its child processes in
ntt_env_child.py, test_fast_cpu.py): inputs of canonical limbs over the whole range [0, r) with the values next to the
modulus planted, one transform through kzg_ntt_device, and the bit-exact comparison that names what differs."""
import numpy as np


def uniform_below_r(rs, n, r):
    """uint64[n,4] limbs of values spread over the WHOLE range [0, r): random 256-bit words with the top limb
    folded below r's top limb (+1 where the lower limbs allow it), so near-r values occur -- the at-size inputs
    of the older tests stop at 2^253."""
    raw = rs.randint(0, 1 << 63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) \
        + rs.randint(0, 2, size=(n, 4)).astype(np.uint64)
    top = r >> 192
    raw[:, 3] %= np.uint64(top)                      # value < top * 2^192 <= r
    return raw


def plant_edge_values(raw, r, native):
    n = raw.shape[0]
    edge = [r - 1, r - 2, 0, 1, r - (1 << 20), (r - 1) // 2, (r + 1) // 2, r - 1]
    pos = [0, 1, 2, 3, n // 2, n // 2 + 1, n - 2, n - 1]
    raw[pos] = native.ints_to_limbs(edge)
    return raw


def edge_vector(rs, n, r, native, turn=0):
    """One input vector of any power-of-two length: uniform_below_r with plant_edge_values; below four elements,
    where the eight positions do not exist, the first element is one of r-1, r-2, 0, 1 (by `turn`)."""
    raw = uniform_below_r(rs, n, r)
    if n >= 4:
        return plant_edge_values(raw, r, native)
    raw[0] = native.ints_to_limbs([[r - 1, r - 2, 0, 1][turn % 4]])[0]
    return raw


def transform_on_device(native, ctx, raw, log_n, w, inverse, batch=1):
    """kzg_ntt_device on a device copy of `raw` (uint64[(batch or more) * n, 4], left unchanged); the whole buffer back"""
    import torch
    d = torch.from_numpy(raw.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()             # torch's stream wrote it; the context runs on a stream of its own
    ctx.ntt_device(d.data_ptr(), log_n, native.int_to_words(w), inverse, batch)
    ctx.synchronize()
    return d.cpu().numpy().view(np.uint64)


def assert_same(got, want, what):
    """np.array_equal on the canonical limbs; a failure says how many elements differ and where, which is what tells
    a wrong vector of a batch from a wrong tile or line"""
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} of {want.shape[0]} elements differ, the first at {bad[:8].tolist()}, "
                             f"the last at {int(bad[-1])}")

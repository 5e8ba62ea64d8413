"""The byte kernels of csrc/blob.hip past one pass of their strided loops: 513 blobs of 4096 elements are 2^21 + 4096
elements, one more blob than 8192 workgroups of 256 lanes take in one pass, so the last blob is the second pass
(tests/lagrange_cases.py, pinned by tests/test_lagrange_cases_host.py).  Device forms between guard words, both orders,
against a reference vectorised in numpy that equals tests/blob_restated.py; non-canonical elements at both ends of
both passes mark their blobs and nothing else.  Equality of integers everywhere."""
import functools
import random

import numpy as np
import pytest

import blob_restated as B
import lagrange_cases as L

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
LOG_N, NB, TOTAL = L.BLOB_LOG_N, L.BLOB_B, L.BLOB_TOTAL
N = 1 << LOG_N
GUARD, GUARD_BYTE = 0x5a5a5a5a5a5a5a5a, 0x5a
ALL_ONES = (1 << 256) - 1


def bitrev_index(log_n):
    i = np.arange(1 << log_n, dtype=np.int64)
    rev = np.zeros_like(i)
    for k in range(log_n):
        rev |= ((i >> k) & 1) << (log_n - 1 - k)
    return rev


def limbs_of(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype="<u8")


def at_least(limbs, r):
    """limbs[..., 4] (little-endian) >= r, element by element"""
    rl = limbs_of(r)
    ge = np.ones(limbs.shape[:-1], dtype=bool)                 # equal so far: >= holds
    for k in range(4):                                         # from the lowest limb up: a higher limb overrides
        ge = np.where(limbs[..., k] == rl[k], ge, limbs[..., k] > rl[k])
    return ge


def np_intake(blobs, log_n, r, bit_reversed):
    """blob_restated.intake over uint8[b, 32 << log_n], vectorised: (uint64[b, n, 4] canonical limbs, uint8[b])"""
    b = blobs.shape[0]
    be = np.ascontiguousarray(blobs).view(">u8").reshape(b, 1 << log_n, 4)
    limbs = be[..., ::-1].astype("<u8")                        # big-endian words, most significant first -> limbs
    bad = at_least(limbs, r)
    limbs[bad] = 0
    if bit_reversed:
        limbs = limbs[:, bitrev_index(log_n)]                  # an involution: out[rev[i]] = in[i]
    return np.ascontiguousarray(limbs), bad.any(axis=1).astype(np.uint8)


def np_output(vals, log_n, r, bit_reversed):
    """the inverse: uint64[b, n, 4] -> (uint8[b, 32 << log_n] big-endian elements, uint8[b]); >= r leaves zero bytes"""
    b = vals.shape[0]
    limbs = vals[:, bitrev_index(log_n)] if bit_reversed else vals.copy()
    bad = at_least(limbs, r)
    limbs[bad] = 0
    out = np.ascontiguousarray(limbs[..., ::-1].astype(">u8")).view(np.uint8).reshape(b, 32 << log_n)
    return out, bad.any(axis=1).astype(np.uint8)


@pytest.mark.parametrize("curve", CURVES)
def test_the_vectorised_reference_is_the_restatement(native, curve):
    """a 3 x 8 batch with 0, r - 1, r, r + 1 and 2^256 - 1 among random elements, both orders, and back"""
    r = B.R[curve]
    rng = random.Random(38)
    rows = [[rng.randrange(r) for _ in range(8)] for _ in range(3)]
    rows[0][0], rows[0][7], rows[1][3], rows[2][1], rows[2][6], rows[2][7] = 0, r - 1, r, r + 1, ALL_ONES, r - 1
    blobs = [b"".join(v.to_bytes(32, "big") for v in row) for row in rows]
    arr = np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(3, 256)
    for bit_reversed in (False, True):
        vals, status = np_intake(arr, 3, r, bit_reversed)
        want = [B.intake(blob, 8, curve, bit_reversed) for blob in blobs]
        assert native.limbs_to_ints(vals.reshape(-1, 4)) == [v for row, _ in want for v in row]
        assert list(status) == [s for _, s in want] == [0, 1, 1]
        back, status = np_output(vals, 3, r, bit_reversed)     # canonical values: the bytes again, bad ones as zeros
        cleaned = [[v if v < r else 0 for v in row] for row in rows]
        assert back.tobytes() == b"".join(v.to_bytes(32, "big") for row in cleaned for v in row)
        assert not status.any()
        raw = np.ascontiguousarray(arr).view(">u8").reshape(3, 8, 4)[..., ::-1].astype("<u8")
        back, status = np_output(raw, 3, r, False)             # limbs >= r on the way out
        assert list(status) == [0, 1, 1] and back.tobytes() == b"".join(
            v.to_bytes(32, "big") for row in cleaned for v in row)
    assert list(bitrev_index(3)) == [B.bitrev(i, 3) for i in range(8)]
    assert list(bitrev_index(LOG_N)[:5]) == [B.bitrev(i, LOG_N) for i in range(5)]


@functools.lru_cache(maxsize=None)
def clean_batch():
    """513 blobs of 4096 random elements below 2^252 (so below both moduli): uint8[513, 131072]"""
    g = np.random.default_rng(513)
    blobs = np.frombuffer(g.bytes(TOTAL * 32), dtype=np.uint8).reshape(NB, 32 * N).copy()
    blobs[:, ::32] &= 0x0f
    return blobs


def upload(arr, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(dtype)).to("cuda:0")


def guarded(words, fill, dtype):
    """a device buffer of `words` items between 32 bytes of guard pattern on either side, and its inner view"""
    import torch
    pad = 32 // np.dtype(dtype).itemsize
    t = torch.from_numpy(np.full(pad + words + pad, fill, dtype=dtype)).to("cuda:0")
    return t, t[pad:pad + words], pad


def guards_intact(t, pad, fill):
    return bool((t[:pad] == fill).all()) and bool((t[-pad:] == fill).all())


def place(idx, bit_reversed, rev):
    """(blob, row) where the kernels keep the value of the byte element with flat index idx"""
    j, i = idx >> LOG_N, idx & (N - 1)
    return j, int(rev[i]) if bit_reversed else i


def plants(curve):
    """the two batches with non-canonical elements: [(flat index, value)] and the blobs they mark"""
    r = B.R[curve]
    four = [(idx, (r, ALL_ONES)[k % 2]) for k, idx in enumerate(L.BLOB_PLANTED)]
    return [(four, list(L.BLOB_PLANTED_BLOBS)), ([(L.BLOB_LONE, r)], [L.BLOB_LONE >> LOG_N])]


@pytest.mark.parametrize("curve", CURVES)
def test_intake_past_one_pass(native, curve):
    """kzg_blob_to_fr_device: the clean batch, r and 2^256 - 1 at the first and last element of either pass, and the
    first element of the second pass alone; then the values back through kzg_fr_to_blob_device"""
    import torch
    r = B.R[curve]
    ctx = native.get_context(curve)
    rev = bitrev_index(LOG_N)
    blobs = clean_batch()
    d_blobs = upload(blobs, np.uint8)
    for bit_reversed in (False, True):
        want, want_status = np_intake(blobs, LOG_N, r, bit_reversed)
        assert not want_status.any()
        d_want = upload(want, np.int64).view(NB, N, 4)
        t_vals, d_vals, pad = guarded(TOTAL * 4, GUARD, np.int64)
        t_status, d_status, spad = guarded(NB, GUARD_BYTE, np.uint8)
        torch.cuda.synchronize()
        ctx.blob_to_fr_device(d_blobs.data_ptr(), LOG_N, NB, bit_reversed, d_vals.data_ptr(), d_status.data_ptr())
        ctx.synchronize()
        assert guards_intact(t_vals, pad, GUARD) and guards_intact(t_status, spad, GUARD_BYTE)
        assert torch.equal(d_vals.view(NB, N, 4), d_want), bit_reversed
        assert not bool(d_status.any())
        # round trip: the bytes again
        t_back, d_back, bpad = guarded(TOTAL * 32, GUARD_BYTE, np.uint8)
        torch.cuda.synchronize()
        ctx.fr_to_blob_device(d_vals.data_ptr(), LOG_N, NB, bit_reversed, d_back.data_ptr(), d_status.data_ptr())
        ctx.synchronize()
        assert guards_intact(t_back, bpad, GUARD_BYTE) and guards_intact(t_status, spad, GUARD_BYTE)
        assert torch.equal(d_back, d_blobs) and not bool(d_status.any()), bit_reversed
        del t_back, d_back
        for planted, marked in plants(curve):
            d_bad = d_blobs.clone().view(TOTAL, 32)
            d_expect = d_want.clone()
            for idx, value in planted:
                d_bad[idx] = torch.from_numpy(np.frombuffer(value.to_bytes(32, "big"), dtype=np.uint8).copy()).to("cuda:0")
                j, row = place(idx, bit_reversed, rev)
                d_expect[j, row] = 0
            d_vals.fill_(GUARD)
            d_status.fill_(GUARD_BYTE)
            torch.cuda.synchronize()
            ctx.blob_to_fr_device(d_bad.data_ptr(), LOG_N, NB, bit_reversed, d_vals.data_ptr(), d_status.data_ptr())
            ctx.synchronize()
            assert guards_intact(t_vals, pad, GUARD) and guards_intact(t_status, spad, GUARD_BYTE)
            assert torch.nonzero(d_status).flatten().tolist() == marked, (bit_reversed, marked)
            assert torch.equal(d_vals.view(NB, N, 4), d_expect), (bit_reversed, marked)
            del d_bad, d_expect


@pytest.mark.parametrize("curve", CURVES)
def test_output_past_one_pass(native, curve):
    """kzg_fr_to_blob_device on the same shape: clean values, and limbs r and 2^256 - 1 where the byte elements at
    both ends of both passes read them"""
    import torch
    r = B.R[curve]
    ctx = native.get_context(curve)
    rev = bitrev_index(LOG_N)
    vals, _ = np_intake(clean_batch(), LOG_N, r, False)        # any canonical values: the blobs' own, in natural order
    d_vals = upload(vals, np.int64).view(NB, N, 4)
    for bit_reversed in (False, True):
        want, want_status = np_output(vals, LOG_N, r, bit_reversed)
        assert not want_status.any()
        d_want = upload(want, np.uint8).view(TOTAL, 32)
        t_out, d_out, pad = guarded(TOTAL * 32, GUARD_BYTE, np.uint8)
        t_status, d_status, spad = guarded(NB, GUARD_BYTE, np.uint8)
        torch.cuda.synchronize()
        ctx.fr_to_blob_device(d_vals.data_ptr(), LOG_N, NB, bit_reversed, d_out.data_ptr(), d_status.data_ptr())
        ctx.synchronize()
        assert guards_intact(t_out, pad, GUARD_BYTE) and guards_intact(t_status, spad, GUARD_BYTE)
        assert torch.equal(d_out.view(TOTAL, 32), d_want) and not bool(d_status.any()), bit_reversed
        for planted, marked in plants(curve):
            d_bad = d_vals.clone()
            d_expect = d_want.clone()
            for idx, value in planted:
                j, row = place(idx, bit_reversed, rev)
                d_bad[j, row] = torch.from_numpy(limbs_of(value).view(np.int64).copy()).to("cuda:0")
                d_expect[idx] = 0
            d_out.fill_(GUARD_BYTE)
            d_status.fill_(GUARD_BYTE)
            torch.cuda.synchronize()
            ctx.fr_to_blob_device(d_bad.data_ptr(), LOG_N, NB, bit_reversed, d_out.data_ptr(), d_status.data_ptr())
            ctx.synchronize()
            assert guards_intact(t_out, pad, GUARD_BYTE) and guards_intact(t_status, spad, GUARD_BYTE)
            assert torch.nonzero(d_status).flatten().tolist() == marked, (bit_reversed, marked)
            assert torch.equal(d_out.view(TOTAL, 32), d_expect), (bit_reversed, marked)
            del d_bad, d_expect

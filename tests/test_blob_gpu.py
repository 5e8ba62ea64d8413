"""GPU tests of EIP-4844 blobs as bytes (csrc/blob.hip through the C ABI and the facade): the intake equals the
restatement (tests/blob_restated.py) element by element, in both orders, with non-canonical elements at the corners of
the batch; the challenges equal hashlib's digest for digest at the wave and workgroup edges of one lane per blob; the
three calls of the specification agree with the existing evaluation-form calls and reject every single change;
pending results of the commit pipeline stay pending and correct.  Equality of integers everywhere."""
import json
import os
import random

import numpy as np
import pytest

import blob_restated as B

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
KZG_ERR_ARG = -1
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


def element_bytes(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def canonical_blobs(rng, b, n, r):
    """b blobs of n random canonical elements, 0 and r - 1 among them"""
    rows = []
    for j in range(b):
        vals = [rng.randrange(r) for _ in range(n)]
        vals[j % n] = 0
        vals[(j + 1) % n] = r - 1
        rows.append(vals)
    return rows


def restated_intake(native, blobs, n, curve, bit_reversed):
    """(uint64[b, n, 4], uint8[b]) from the restatement"""
    vals, status = zip(*(B.intake(blob, n, curve, bit_reversed) for blob in blobs))
    flat = [v for row in vals for v in row]
    return native.ints_to_limbs(flat).reshape(len(blobs), n, 4), np.array(status, dtype=np.uint8)


# ---- 1. intake --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_intake_equals_the_restatement_element_by_element(kzgs, native, curve):
    ctx = kzgs[curve]._context()
    r = B.R[curve]
    rng = random.Random(len(curve))
    for b in (1, 3, 65):
        for n in (2, 8, 256):
            blobs = [element_bytes(row) for row in canonical_blobs(rng, b, n, r)]
            arr = np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(b, 32 * n)
            for bit_reversed in (False, True):
                vals, status = ctx.blob_to_fr(arr, n.bit_length() - 1, bit_reversed)
                want, want_status = restated_intake(native, blobs, n, curve, bit_reversed)
                assert not status.any() and not want_status.any(), (b, n, bit_reversed)
                assert np.array_equal(vals, want), (b, n, bit_reversed)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("b,n", [(1, 2), (3, 8), (65, 256)])
def test_non_canonical_elements_mark_their_blob_and_nothing_else(kzgs, native, curve, b, n):
    """r, r + 1 and 2^256 - 1 at the first and the last element of the first and the last blob"""
    ctx = kzgs[curve]._context()
    r = B.R[curve]
    rng = random.Random(b * n)
    for bad in (r, r + 1, (1 << 256) - 1):
        for blob_at in sorted({0, b - 1}):
            for elem_at in (0, n - 1):
                rows = canonical_blobs(rng, b, n, r)
                rows[blob_at][elem_at] = bad
                blobs = [element_bytes(row) for row in rows]
                arr = np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(b, 32 * n)
                for bit_reversed in (False, True):
                    vals, status = ctx.blob_to_fr(arr, n.bit_length() - 1, bit_reversed)
                    want, want_status = restated_intake(native, blobs, n, curve, bit_reversed)
                    assert list(np.flatnonzero(status)) == [blob_at] == list(np.flatnonzero(want_status))
                    assert status[blob_at] == 1
                    at = B.bitrev(elem_at, n.bit_length() - 1) if bit_reversed else elem_at
                    assert not vals[blob_at, at].any()                       # the bad element is zeros
                    assert np.array_equal(vals, want)                        # every other element still correct


@pytest.mark.parametrize("curve", CURVES)
def test_device_form_writes_between_guard_words(kzgs, native, curve):
    import torch
    ctx = kzgs[curve]._context()
    r = B.R[curve]
    b, n, log_n = 3, 8, 3
    rng = random.Random(17)
    rows = canonical_blobs(rng, b, n, r)
    rows[1][5] = r                                                           # one blob is marked
    blobs = [element_bytes(row) for row in rows]
    arr = np.frombuffer(bytearray(b"".join(blobs)), dtype=np.uint8).reshape(b, 32 * n)
    want, want_status = restated_intake(native, blobs, n, curve, True)
    dev = f"cuda:{ctx.device}"
    GUARD = 0x5a5a5a5a5a5a5a5a
    d_blobs = torch.from_numpy(arr.view(np.int64)).to(dev)
    d_vals = torch.from_numpy(np.full(4 + b * n * 4 + 4, GUARD, dtype=np.int64)).to(dev)   # 32 guard bytes each side
    d_status = torch.from_numpy(np.full(32 + b + 32, 0x5a, dtype=np.uint8)).to(dev)
    torch.cuda.synchronize(ctx.device)
    ctx.blob_to_fr_device(d_blobs.data_ptr(), log_n, b, True, d_vals.data_ptr() + 32, d_status.data_ptr() + 32)
    ctx.synchronize()
    vals, status = d_vals.cpu().numpy(), d_status.cpu().numpy()
    assert (vals[:4] == GUARD).all() and (vals[-4:] == GUARD).all()
    assert (status[:32] == 0x5a).all() and (status[32 + b:] == 0x5a).all()
    assert np.array_equal(vals[4:-4].view(np.uint64).reshape(b, n, 4), want)
    assert list(status[32:32 + b]) == list(want_status) == [0, 1, 0]


# ---- 2. challenges ------------------------------------------------------------------------------------------------------
def challenge_case(native, ctx, curve, n, b, seed):
    G = B.G_BYTES[curve]
    rng = np.random.default_rng(seed)
    blobs = rng.integers(0, 256, size=(b, 32 * n), dtype=np.uint8)
    blobs[0] = 0xff                                                          # bytes that are no field elements
    comms = rng.integers(0, 256, size=(b, G), dtype=np.uint8)
    z = ctx.blob_challenges(blobs, comms, n.bit_length() - 1)
    got = native.limbs_to_ints(z)
    want = [B.challenge(blobs[j].tobytes(), comms[j].tobytes(), n, curve) for j in range(b)]
    return got == want


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("b", [1, 63, 64, 65, 130])
def test_challenges_equal_hashlib_at_the_wave_and_workgroup_edges(kzgs, native, curve, b):
    ctx = kzgs[curve]._context()
    for n in (2, 4, 8):
        assert challenge_case(native, ctx, curve, n, b, seed=n * 1000 + b), n


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("b", [1, 130])
def test_challenges_of_full_size_blobs(kzgs, native, curve, b):
    """n = 4096: 2,050 compressions per lane; b = 130 is 17 MB of blobs, three waves"""
    assert challenge_case(native, kzgs[curve]._context(), curve, 4096, b, seed=b)


@pytest.mark.parametrize("curve", CURVES)
def test_challenges_separate_near_equal_inputs(kzgs, native, curve):
    """two blobs that differ in their last byte only; two equal blobs with different commitments"""
    ctx = kzgs[curve]._context()
    n, G = 8, B.G_BYTES[curve]
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, size=32 * n, dtype=np.uint8)
    x2 = x.copy()
    x2[-1] ^= 1
    c = rng.integers(0, 256, size=(2, G), dtype=np.uint8)
    c[1] = c[0]
    c[1, -1] ^= 0x80
    blobs = np.stack([x, x2, x, x])
    comms = np.stack([c[0], c[0], c[0], c[1]])
    z = native.limbs_to_ints(ctx.blob_challenges(blobs, comms, 3))
    assert z == [B.challenge(blobs[j].tobytes(), comms[j].tobytes(), n, curve) for j in range(4)]
    assert z[0] == z[2] and len({z[0], z[1], z[3]}) == 3


def test_argument_errors_and_empty_batches(kzgs, native):
    ctx = kzgs["bls12_381"]._context()
    lib, vp = native.lib(), native._as_vp
    blob = np.zeros((1, 64), dtype=np.uint8)
    comm = np.zeros((1, 48), dtype=np.uint8)
    vals, status, z = np.zeros((1, 2, 4), dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros((1, 4), dtype=np.uint64)
    assert lib.kzg_blob_to_fr(ctx._h, 1, vp(blob), 1, 1, vp(vals), vp(status)) == 0
    assert lib.kzg_blob_to_fr(ctx._h, 0, vp(blob), 1, 1, vp(vals), vp(status)) == KZG_ERR_ARG          # log_n = 0
    assert lib.kzg_blob_to_fr(ctx._h, 25, vp(blob), 1, 1, vp(vals), vp(status)) == KZG_ERR_ARG         # log_n = 25
    assert lib.kzg_blob_to_fr(ctx._h, 24, vp(blob), 5, 1, vp(vals), vp(status)) == KZG_ERR_ARG         # 5 * 2^24 > 2^26
    assert lib.kzg_blob_challenges(ctx._h, 0, vp(blob), vp(comm), 1, vp(z)) == KZG_ERR_ARG
    assert lib.kzg_blob_challenges(ctx._h, 24, vp(blob), vp(comm), 5, vp(z)) == KZG_ERR_ARG
    assert lib.kzg_blob_to_fr(ctx._h, 1, None, 0, 1, None, None) == 0                                  # b = 0: no work
    assert lib.kzg_blob_challenges(ctx._h, 1, None, None, 0, None) == 0
    assert lib.kzg_blob_to_fr_device(ctx._h, 1, 16, 1, 1, 48, 64) == KZG_ERR_ARG                       # d_vals not 32-aligned
    assert lib.kzg_blob_challenges_device(ctx._h, 1, 16, 8, 1, 64) == KZG_ERR_ARG                      # commitments not 16-aligned
    assert lib.kzg_blob_challenges(ctx._h, 1, vp(blob), vp(comm), 1, vp(z)) == 0                       # still usable
    assert native.limbs_to_ints(z) == [B.challenge(bytes(64), bytes(48), 2, "bls12_381")]


# ---- 3. end to end: the three calls of the specification --------------------------------------------------------------
def outside_subgroup_blob():
    """a BLS12-381 point on the curve and outside the subgroup, compressed, from the golden file"""
    with open(os.path.join(HERE, "golden", "g1_bytes_vectors.json")) as f:
        return bytes.fromhex(json.load(f)["bls12_381"]["status3"][0]["blob"])


@pytest.mark.parametrize("curve,n,b", [("bls12_381", 8, 5), ("bn254", 8, 5), ("bls12_381", 4096, 3)])
def test_the_three_calls_end_to_end(kzgs, native, curve, n, b):
    """n = 8 on both curves, and once at the size of EIP-4844 on its curve (each verdict is two pure-Python pairings)"""
    kzg = kzgs[curve]
    r, G = B.R[curve], B.G_BYTES[curve]
    log_n = n.bit_length() - 1
    rng = random.Random(n + b)
    lk, rk = kzg.setup_lagrange(n, tau=TAU)
    rows = canonical_blobs(rng, b, n, r)
    blobs = [element_bytes(row) for row in rows]
    natural = [B.intake(blob, n, curve)[0] for blob in blobs]

    values = kzg.blob_to_values(blobs, n)
    assert native.limbs_to_ints(values.reshape(-1, 4)) == [v for row in natural for v in row]
    comms = kzg.blob_to_kzg_commitment(lk, blobs)
    assert comms == kzg.compress_g1(kzg.commit_evaluations(lk, natural))
    assert all(isinstance(c, bytes) and len(c) == G for c in comms)
    zs = [B.challenge(blob, c, n, curve) for blob, c in zip(blobs, comms)]
    assert [int(z) for z in kzg.blob_challenges(blobs, comms, n)] == zs
    proofs = kzg.compute_blob_kzg_proof(lk, blobs, comms)
    assert proofs == kzg.compress_g1([kzg.open_evaluations(lk, [natural[j]], zs[j], 1) for j in range(b)])

    assert kzg.verify_blob_kzg_proof_batch(lk, rk, blobs, comms, proofs) is True
    if n == 8:                                                               # the root alone, arrays for lists
        assert kzg.verify_blob_kzg_proof_batch(
            lk.w, rk, np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(b, -1),
            np.frombuffer(b"".join(comms), dtype=np.uint8).reshape(b, G), proofs) is True
    ys = [int(y) for y in kzg.evaluate_evaluations_each(lk, natural, zs)]
    rho = B.rho(n, comms, zs, ys, proofs, curve)
    assert kzg.verify_blobs(lk, rk, kzg.decompress_g1(comms), natural, zs, kzg.decompress_g1(proofs), r=rho) is True

    def verdict(blobs=blobs, comms=comms, proofs=proofs):
        return kzg.verify_blob_kzg_proof_batch(lk, rk, blobs, comms, proofs)

    flipped = list(blobs)
    raw = bytearray(flipped[1])
    raw[32 * (n - 1) + 31] ^= 1                                              # one byte of one blob (still canonical)
    flipped[1] = bytes(raw)
    assert B.intake(flipped[1], n, curve)[1] == 0
    assert verdict(blobs=flipped) is False
    assert proofs[0] != proofs[1]
    assert verdict(proofs=[proofs[1], proofs[0]] + proofs[2:]) is False      # two proofs swapped
    with_r = list(blobs)
    with_r[b - 1] = with_r[b - 1][:32 * 3] + r.to_bytes(32, "big") + with_r[b - 1][32 * 4:]
    assert verdict(blobs=with_r) is False                                    # one element replaced by r
    with pytest.raises(ValueError, match=rf"blob {b - 1}: element 3 "):
        kzg.blob_to_values(with_r, n)
    vals, status = kzg.blob_to_values(with_r, n, strict=False)
    assert list(status) == [0] * (b - 1) + [1] and not vals[b - 1, B.bitrev(3, log_n)].any()
    with pytest.raises(ValueError):
        kzg.blob_to_kzg_commitment(lk, with_r)
    with pytest.raises(ValueError):
        kzg.compute_blob_kzg_proof(lk, with_r, comms)
    cleared = list(comms)
    keep = 0x7f if curve == "bls12_381" else 0x3f                            # ZCash: bit 7; gnark: both top bits
    cleared[0] = bytes([cleared[0][0] & keep]) + cleared[0][1:]              # the compression flag cleared
    assert kzg.decompress_g1(cleared, strict=False)[1][0] == 1
    assert verdict(comms=cleared) is False
    if curve == "bls12_381":
        forged = list(proofs)
        forged[2] = outside_subgroup_blob()
        assert kzg.decompress_g1(forged, strict=False)[1][2] == 3
        assert verdict(proofs=forged) is False

    assert kzg.verify_blob_kzg_proof_batch(lk, rk, [], [], []) is True       # no blobs
    assert kzg.blob_to_kzg_commitment(lk, []) == [] and kzg.compute_blob_kzg_proof(lk, [], []) == []
    for bad in (dict(comms=comms[:-1]), dict(proofs=proofs + proofs[:1]), dict(blobs=blobs[:-1]),
                dict(blobs=[blobs[0][:-1]] + blobs[1:]), dict(comms=[comms[0] + b"\x00"] + comms[1:])):
        with pytest.raises(ValueError):
            verdict(**bad)
    with pytest.raises(ValueError):
        kzg.compute_blob_kzg_proof(lk, blobs, comms[:-1])
    with pytest.raises(ValueError):
        kzg.blob_challenges(blobs, comms[:-1], n)


# ---- 4. the commit pipeline is not touched ---------------------------------------------------------------------------------
def test_pending_commits_stay_pending_and_correct_across_blob_calls(kzgs, native):
    import torch
    curve = "bls12_381"
    kzg = kzgs[curve]
    ctx = kzg._context()
    L, r = ctx.fp_limbs, B.R[curve]
    n = 1 << 12
    ck = kzg.setup(n - 1, tau=TAU)[0]
    rng = np.random.default_rng(6)
    polys = rng.integers(0, 1 << 63, size=(2, n, 4), dtype=np.uint64)
    polys[..., 3] %= np.uint64(r >> 192)
    want_xy, want_inf = ctx.commit(ck.srs, polys, [n, n], n)
    b, bn = 70, 8
    blobs = rng.integers(0, 256, size=(b, 32 * bn), dtype=np.uint8)
    blobs[:, ::32] &= 0x0f                                                   # every element below r
    comms = rng.integers(0, 256, size=(b, 48), dtype=np.uint8)
    d = torch.from_numpy(polys.view(np.int64)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize(ctx.device)
    out_xy = np.zeros((2, 2 * L), dtype=np.uint64)
    out_inf = np.full(2, 9, dtype=np.uint8)
    ctx.commit_device_async(ck.srs, d.data_ptr(), [n, n], n, out_xy, out_inf)
    vals, status = ctx.blob_to_fr(blobs, 3, True)
    z = ctx.blob_challenges(blobs, comms, 3)
    assert len(ctx._inflight) == 1 and (out_inf == 9).all()               # not retired: delivered at the flush
    ctx.commit_flush()
    assert (out_xy == want_xy).all() and (out_inf == want_inf).all()
    rows = [blobs[j].tobytes() for j in range(b)]
    want_vals, want_status = restated_intake(native, rows, bn, curve, True)
    assert np.array_equal(vals, want_vals) and not status.any() and not want_status.any()
    assert native.limbs_to_ints(z) == [B.challenge(rows[j], comms[j].tobytes(), bn, curve) for j in range(b)]


# ---- 5. one profiling span per call -----------------------------------------------------------------------------------
def test_one_span_per_call(kzgs, native):
    ctx = kzgs["bn254"]._context()
    blobs = np.zeros((3, 64), dtype=np.uint8)
    comms = np.zeros((3, 32), dtype=np.uint8)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for _ in range(3):
            ctx.blob_to_fr(blobs, 1)
        for _ in range(2):
            ctx.blob_challenges(blobs, comms, 1)
        ms, count = ctx.prof_read("blob_intake")
        assert count == 3 and ms > 0
        ms, count = ctx.prof_read("blob_challenge")
        assert count == 2 and ms > 0
    finally:
        ctx.prof_enable(False)

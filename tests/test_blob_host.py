"""EIP-4844 blobs as bytes on the CPU: the restatement (tests/blob_restated.py) against public facts, and
csrc/sha256.h / csrc/blob.h -- the text the gfx950 kernels of blob.hip compile -- built for the host
(tests/shim/blob_shim.cpp) against hashlib and the restatement.  The shim runs plain and with -DKZG_AUDIT, and once as
a program of its own under the address and undefined-behaviour sanitizers."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

import blob_restated as B

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "shim")
SRC = os.path.join(SHIM_DIR, "blob_shim.cpp")
CURVE_IDS = {"bn254": 0, "bls12_381": 1}
CURVES = ["bls12_381", "bn254"]
U64x4 = ctypes.c_uint64 * 4


# ---- the restatement --------------------------------------------------------------------------------------------

def test_restatement_is_pinned_to_public_facts():
    assert hashlib.sha256(b"abc").hexdigest() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    assert B.FS_DOMAIN == b"FSBLOBVERIFY_V1_" and B.RHO_DOMAIN == b"RCKZGBATCH___V1_"
    assert len(B.FS_DOMAIN) == len(B.RHO_DOMAIN) == 16
    u = -0xd201000000010000                                           # BLS12-381: r = u^4 - u^2 + 1
    assert B.R["bls12_381"] == u ** 4 - u ** 2 + 1
    assert B.R["bls12_381"] == 52435875175126190479447740508185965837690552500527637822603658699938581184513
    t = 4965661367192848881                                            # BN254: r = 36 t^4 + 36 t^3 + 18 t^2 + 6 t + 1
    assert B.R["bn254"] == 36 * t ** 4 + 36 * t ** 3 + 18 * t ** 2 + 6 * t + 1
    assert B.R["bn254"] == 21888242871839275222246405745257275088548364400416034343698204186575808495617
    assert (1 << 256) // B.R["bls12_381"] == 2 and (1 << 256) // B.R["bn254"] == 5
    from kzg_snark_amd import curve as C
    for name in CURVES:
        assert C.CURVES[name].r == B.R[name] and C.g1_compressed_size(C.CURVES[name]) == B.G_BYTES[name]
    assert [B.bitrev(i, 3) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7] and B.bitrev(0, 0) == 0


def test_restated_intake():
    r = B.R["bn254"]
    elems = [5, r - 1, r, 7]
    blob = b"".join(e.to_bytes(32, "big") for e in elems)
    assert B.intake(blob, 4, "bn254", bit_reversed=False) == ([5, r - 1, 0, 7], 1)
    assert B.intake(blob, 4, "bn254", bit_reversed=True) == ([5, 0, r - 1, 7], 1)
    assert B.intake(blob[:64], 2, "bn254") == ([5, r - 1], 0)


# ---- sha256.h / blob.h on the host -------------------------------------------------------------------------------

def build_shim(audit):
    kind = "audit" if audit else "plain"
    so = os.path.join(SHIM_DIR, f"libblob_shim_{kind}.so")
    subprocess.run(["g++", "-O0" if audit else "-O1", "-std=c++17", *(["-DKZG_AUDIT"] if audit else []), "-shared",
                    "-fPIC", SRC, "-o", so], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module", params=["plain", "audit"])
def shim(request):
    lib = build_shim(request.param == "audit")
    lib.audited = request.param == "audit"
    if lib.audited:
        lib.bs_audit_count.restype = ctypes.c_ulonglong
    return lib


def assert_clean(shim):
    if shim.audited:
        assert shim.bs_audit_count() == 0


def limbs_value(out):
    return sum(int(v) << (64 * i) for i, v in enumerate(out))


def padded(msg):
    """FIPS 180-4 5.1.1, written out here"""
    zeros = (55 - len(msg)) % 64
    return msg + b"\x80" + b"\x00" * zeros + (8 * len(msg)).to_bytes(8, "big")


@pytest.mark.parametrize("length", [0, 3, 55, 56, 63, 64, 65, 119, 120])
def test_compression_function_block_by_block_against_hashlib(shim, length):
    rng = random.Random(length)
    msg = b"abc" if length == 3 else bytes(rng.randrange(256) for _ in range(length))
    data = padded(msg)
    assert len(data) % 64 == 0 and len(data) // 64 == (length + 8) // 64 + 1
    state = (ctypes.c_uint32 * 8)()
    shim.bs_sha256_init(state)
    for k in range(0, len(data), 64):
        shim.bs_sha256_block(state, data[k:k + 64])
    assert b"".join(int(w).to_bytes(4, "big") for w in state) == hashlib.sha256(msg).digest()
    assert_clean(shim)


@pytest.mark.parametrize("curve", CURVES)
def test_digest_reduction_on_chosen_values(shim, curve):
    r, cid = B.R[curve], CURVE_IDS[curve]
    trips = (1 << 256) // r
    assert shim.bs_digest_trips(cid) == trips
    values = [0, r - 1, r, 2 * r - 1, 2 * r, (1 << 256) - 1]
    if curve == "bn254":
        values += [k * r - 1 for k in (3, 4, 5)] + [k * r for k in (3, 4, 5)]
    assert max(v // r for v in values) == trips                       # every trip of the loop runs
    for v in values:
        assert v < 1 << 256
        out = U64x4()
        assert shim.bs_fr_from_digest(cid, v.to_bytes(32, "big"), out) == 0
        assert limbs_value(out) == v % r, hex(v)
    assert_clean(shim)


@pytest.mark.parametrize("curve", CURVES)
def test_element_check(shim, curve):
    r, cid = B.R[curve], CURVE_IDS[curve]
    rng = random.Random(3)
    for v in [0, 1, r - 1, r, r + 1, (1 << 256) - 1, 1 << 255, r ^ 1 << 32, r - (1 << 224)] + \
             [rng.randrange(1 << 256) for _ in range(16)]:
        out = U64x4()
        ok = shim.bs_element(cid, v.to_bytes(32, "big"), out)
        assert ok == (1 if v < r else 0), hex(v)
        assert limbs_value(out) == (v if v < r else 0), hex(v)
    assert_clean(shim)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [2, 4, 8, 64])
def test_challenge_against_the_restatement(shim, curve, n):
    cid, G = CURVE_IDS[curve], B.G_BYTES[curve]
    assert shim.bs_commitment_size(cid) == G
    rng = random.Random(n * 7 + cid)
    blobs = [bytes(rng.randrange(256) for _ in range(32 * n)), b"\x00" * (32 * n), b"\xff" * (32 * n)]
    comms = [bytes(rng.randrange(256) for _ in range(G)), b"\x00" * G, b"\xff" * G]
    seen = set()
    for blob in blobs:
        for comm in comms:
            out, pieces = U64x4(), ctypes.c_uint64(0)
            assert shim.bs_challenge(cid, n.bit_length() - 1, blob, comm, out, ctypes.byref(pieces)) == 0
            assert pieces.value == 2 * n                                # every 16-byte piece exactly once
            assert limbs_value(out) == B.challenge(blob, comm, n, curve)
            seen.add(limbs_value(out))
    assert len(seen) == 9
    # the block count of the layout blob.h describes: n/2 + 2 on both curves (three at n = 2)
    assert len(padded(b"\x00" * (32 + 32 * n + G))) // 64 == n // 2 + 2
    assert_clean(shim)


# ---- rho ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("b", [1, 3])
def test_rho_against_a_byte_string_concatenated_by_hand(curve, b):
    from kzg_snark_amd.kzg import KZG
    kzg = KZG(curve)
    G, r, n = B.G_BYTES[curve], B.R[curve], 4096
    rng = random.Random(b)
    comms = [bytes(rng.randrange(256) for _ in range(G)) for _ in range(b)]
    proofs = [bytes(rng.randrange(256) for _ in range(G)) for _ in range(b)]
    zs = [rng.randrange(r) for _ in range(b)]
    ys = [rng.randrange(r) for _ in range(b)]
    zs[0], ys[-1] = 1, r - 1
    data = b"RCKZGBATCH___V1_" + b"\x00" * 6 + b"\x10\x00" + b"\x00" * 7 + bytes([b])
    for j in range(b):
        data += comms[j] + zs[j].to_bytes(32, "big") + ys[j].to_bytes(32, "big") + proofs[j]
    assert len(data) == 32 + b * (2 * G + 64)
    want = int.from_bytes(hashlib.sha256(data).digest(), "big") % r
    assert B.rho(n, comms, zs, ys, proofs, curve) == want
    assert kzg._blob_batch_rho(n, comms, zs, ys, proofs) == want


# ---- argument checks of the facade that need no device ---------------------------------------------------------------

def test_facade_refuses_sizes_before_any_device_work():
    from kzg_snark_amd.kzg import KZG
    kzg = KZG("bls12_381")
    with pytest.raises(ValueError):
        kzg.blob_to_values([b"\x00" * 96], 3)                           # n is not a power of two
    with pytest.raises(ValueError):
        kzg.blob_to_values([b"\x00" * 64], 1)                           # n below 2
    with pytest.raises(ValueError):
        kzg._byte_rows([b"\x00" * 64, b"\x00" * 63], 64, "blob")
    assert kzg._byte_rows([], 64, "blob").shape == (0, 64)


# ---- sanitizers -----------------------------------------------------------------------------------------------------

def test_shim_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """blob_shim.cpp with its own main(): SHA-256 of "abc" and of the empty message, the digest reduction and the
    element check around r, challenges of blobs of 2 .. 64 elements in buffers of their exact size, on both curves; built
    with -DKZG_AUDIT and -fsanitize=address,undefined (no recovery, static runtimes) and run as a program of its own.
    Exit status 0 = no sanitizer report, no audit violation, every check of the program passed."""
    exe = str(tmp_path / "blob_shim_san")
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-DKZG_AUDIT", "-DBLOB_SHIM_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert "no violations" in res.stdout

"""EIP-4844 blobs as bytes, restated with hashlib and Python integers: the reference of tests/test_blob_host.py and
tests/test_blob_gpu.py.  Nothing here imports the package under test."""
import hashlib

FS_DOMAIN = b"FSBLOBVERIFY_V1_"                # FIAT_SHAMIR_PROTOCOL_DOMAIN of EIP-4844
RHO_DOMAIN = b"RCKZGBATCH___V1_"               # RANDOM_CHALLENGE_KZG_BATCH_DOMAIN
R = {"bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
     "bn254": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
G_BYTES = {"bls12_381": 48, "bn254": 32}       # a compressed G1 point: ZCash's format / gnark's


def bitrev(i, log_n):
    return int(format(i, f"0{log_n}b")[::-1], 2) if log_n else 0


def challenge(blob, commitment, n, curve):
    """z = SHA-256(domain | n as 16 bytes BE | blob | commitment) mod r"""
    assert len(blob) == 32 * n and len(commitment) == G_BYTES[curve]
    digest = hashlib.sha256(FS_DOMAIN + n.to_bytes(16, "big") + bytes(blob) + bytes(commitment)).digest()
    return int.from_bytes(digest, "big") % R[curve]


def rho(n, commitments, zs, ys, proofs, curve):
    """the weight base of the batch: SHA-256(domain | n (8 B) | b (8 B) | per blob: commitment | z | y | proof) mod r"""
    data = RHO_DOMAIN + n.to_bytes(8, "big") + len(zs).to_bytes(8, "big")
    for c, z, y, p in zip(commitments, zs, ys, proofs):
        data += bytes(c) + int(z).to_bytes(32, "big") + int(y).to_bytes(32, "big") + bytes(p)
    return int.from_bytes(hashlib.sha256(data).digest(), "big") % R[curve]


def intake(blob, n, curve, bit_reversed=True):
    """(values in natural order -- element i at bitrev(i) when bit_reversed --, status): an element >= r becomes 0
    and sets status 1"""
    log_n = n.bit_length() - 1
    vals, status = [0] * n, 0
    for i in range(n):
        v = int.from_bytes(blob[32 * i:32 * i + 32], "big")
        if v >= R[curve]:
            v, status = 0, 1
        vals[bitrev(i, log_n) if bit_reversed else i] = v
    return vals, status

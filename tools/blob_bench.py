"""Timing of EIP-4844 blobs as bytes on one GPU, BLS12-381, n = 4096, b = 6, 64 and 1024 blobs.

Per b, alternating in one process:

    upload_ms      the blobs and commitments from host memory to the device (a torch copy, synchronised)
    device_ms      kzg_blob_to_fr_device + kzg_blob_challenges_device on the resident bytes, until z is on the host
    host_hash_ms   hashlib.sha256 over the same blobs, one core: the challenges on the host
    host_intake_ms a numpy intake of the same blobs: byte swap, comparison with r, bit-reversal permutation
    verify_ms      KZG.verify_blob_kzg_proof_batch(pairing="host") end to end from bytes, its two pure-Python pairings
                   included
    verify_device_ms   the same call with pairing="device": the verdict from one kzg_pairing_check
    pairings_ms    those two pairings alone (what verify_ms spends after the device is done)

    python tools/blob_bench.py [--out DIR] [--reps 5] [--blobs 6,64,1024]

Every figure is the median of --reps runs after one warm-up; every repetition's challenges and values are compared
with the host's, and every batch must verify.  Prints one JSON line (and writes DIR/blob_bench.json with --out)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x1d0c_7e5a_9b3f_2468_ace0_1357_9bdf
LOG_N = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blobs", default="6,64,1024")
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG("bls12_381")
    ctx = kzg._context()
    r = kzg.curve_order
    n = 1 << LOG_N
    G = ctx.g1_bytes
    dev = f"cuda:{ctx.device}"
    lk, rk = kzg.setup_lagrange(n, tau=TAU)
    res = {"curve": "bls12_381", "n": n, "reps": a.reps, "blobs": {}}
    r_limbs = _native.int_to_words(r)
    rev = np.array([int(format(i, f"0{LOG_N}b")[::-1], 2) for i in range(n)])

    def timed(fn):
        torch.cuda.synchronize(ctx.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(ctx.device)
        return (time.perf_counter() - t0) * 1e3, out

    def med(samples):
        return {"median": statistics.median(samples), "twice_spread": 2 * (max(samples) - min(samples)),
                "samples": [round(s, 3) for s in samples]}

    def host_hash(blobs, comms):
        head = b"FSBLOBVERIFY_V1_" + n.to_bytes(16, "big")
        return [int.from_bytes(hashlib.sha256(head + blobs[j].tobytes() + comms[j].tobytes()).digest(), "big") % r
                for j in range(blobs.shape[0])]

    def host_intake(blobs):
        limbs = np.ascontiguousarray(blobs.reshape(-1, n, 32)[..., ::-1]).view("<u8")       # [b, n, 4], little-endian
        below = np.zeros(limbs.shape[:2], dtype=bool)
        undecided = np.ones(limbs.shape[:2], dtype=bool)
        for k in (3, 2, 1, 0):
            below |= undecided & (limbs[..., k] < r_limbs[k])
            undecided &= limbs[..., k] == r_limbs[k]
        out = np.empty_like(limbs)
        out[:, rev] = np.where(below[..., None], limbs, 0)
        return out, (~below).any(axis=1)

    for b in [int(s) for s in a.blobs.split(",") if s]:
        rng = np.random.default_rng(b)
        blobs = rng.integers(0, 256, size=(b, 32 * n), dtype=np.uint8)
        blobs[:, ::32] &= 0x3f                                          # every element below 2^254 < r
        comms_b = kzg.blob_to_kzg_commitment(lk, blobs)
        proofs_b = kzg.compute_blob_kzg_proof(lk, blobs, comms_b)
        comms = np.frombuffer(bytearray(b"".join(comms_b)), dtype=np.uint8).reshape(b, G)
        proofs = np.frombuffer(bytearray(b"".join(proofs_b)), dtype=np.uint8).reshape(b, G)
        d_vals = torch.empty((b, n, 4), dtype=torch.int64, device=dev)
        d_z = torch.empty((b, 4), dtype=torch.int64, device=dev)
        d_status = torch.empty(b, dtype=torch.uint8, device=dev)

        def upload():
            return (torch.from_numpy(blobs.view(np.int64)).to(dev), torch.from_numpy(comms.view(np.int64)).to(dev))

        def device(d_blobs, d_comms):
            ctx.blob_to_fr_device(d_blobs.data_ptr(), LOG_N, b, True, d_vals.data_ptr(), d_status.data_ptr())
            ctx.blob_challenges_device(d_blobs.data_ptr(), d_comms.data_ptr(), LOG_N, b, d_z.data_ptr())
            ctx.synchronize()
            return _native.limbs_to_ints(d_z.cpu().numpy().view(np.uint64))

        t = {k: [] for k in ("upload_ms", "device_ms", "host_hash_ms", "host_intake_ms", "verify_ms", "pairings_ms",
                             "verify_device_ms")}
        for rep in range(a.reps + 1):
            ms_u, (d_blobs, d_comms) = timed(upload)
            ms_d, z_dev = timed(lambda: device(d_blobs, d_comms))
            ms_h, z_host = timed(lambda: host_hash(blobs, comms))
            ms_i, (vals_host, bad_host) = timed(lambda: host_intake(blobs))
            ms_v, ok = timed(lambda: kzg.verify_blob_kzg_proof_batch(lk, rk, blobs, comms, proofs, pairing="host"))
            ms_vd, ok_dev = timed(lambda: kzg.verify_blob_kzg_proof_batch(lk, rk, blobs, comms, proofs, pairing="device"))
            ms_p, _ = timed(lambda: (kzg.pairing(kzg.G2, kzg.G1), kzg.pairing(rk, kzg.G1)))
            assert z_dev == z_host, f"{b} blobs: the device's challenges differ from hashlib's"
            assert np.array_equal(d_vals.cpu().numpy().view(np.uint64), vals_host) and not bad_host.any()
            assert not d_status.cpu().numpy().any() and ok is True, f"{b} blobs: the batch does not verify"
            assert ok_dev is True, f"{b} blobs: the batch does not verify with the pairing on the device"
            if rep:
                for k, v in zip(t, (ms_u, ms_d, ms_h, ms_i, ms_v, ms_p, ms_vd)):
                    t[k].append(v)
        m = {k: statistics.median(v) for k, v in t.items()}
        res["blobs"][str(b)] = {
            "blobs": b, **{k: med(v) for k, v in t.items()},
            "device_with_upload_ms": m["upload_ms"] + m["device_ms"],
            "host_ms": m["host_hash_ms"] + m["host_intake_ms"],
            "device_over_host": (m["upload_ms"] + m["device_ms"]) / (m["host_hash_ms"] + m["host_intake_ms"]),
            "verify_without_pairings_ms": m["verify_ms"] - m["pairings_ms"],
        }
        print(f"{b} blobs: upload {m['upload_ms']:.2f} ms, device {m['device_ms']:.2f} ms, hashlib "
              f"{m['host_hash_ms']:.2f} ms, numpy intake {m['host_intake_ms']:.2f} ms, verify {m['verify_ms']:.1f} ms "
              f"(pairings {m['pairings_ms']:.1f} ms), with the device pairing {m['verify_device_ms']:.1f} ms",
              file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "blob_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

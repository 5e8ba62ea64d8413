"""Timing of EIP-7594 cells as bytes on one GPU, BLS12-381, n = 4096, l = 64, N = 8192, b = 1, 6 and
64 blobs.

Per b, the legs alternating in one process, every leg from the same blob bytes to the same cell and proof bytes:

    new_ms         KZG.compute_cells_and_kzg_proofs: intake, both transforms, kzg_fr_to_blob_device and FK20 on the
                   resident coefficients; only bytes cross to the host
    old_ms         the route before it: blob_to_values, the inverse transform per blob, Context.open_cosets with the
                   values as limbs (what open_cosets_each(with_values=True) calls), a numpy encoding of the cells
                   (bit-reversal of both index spaces, byte swap) and compress_g1 with the proofs reordered
    old_encode_ms  the numpy encoding alone
    verify_ms      KZG.verify_cell_kzg_proof_batch(pairing="device") on every cell of the b blobs, and its parts run
                   on their own: hash_ms (the batch challenge, hashlib), decompress_ms (kzg_g1_decompress of the
                   distinct commitments and the proofs), fold_ms (kzg_verify_cosets_bytes), pairing_ms (one
                   kzg_pairing_check)

    python tools/cells_bench.py [--out DIR] [--reps 3] [--blobs 1,6,64]

Every figure is the median of --reps runs after one warm-up.  In every repetition the new route must reproduce the
old one byte for byte, and the batch must verify.  Prints one JSON line (and writes DIR/cells_bench.json with --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x1d0c_7e5a_9b3f_2468_ace0_1357_9bdf
LOG_N, LOG_L, LOG_EXT = 12, 6, 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blobs", default="1,6,64")
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG("bls12_381")
    ctx = kzg._context()
    r = kzg.curve_order
    n, l, N = 1 << LOG_N, 1 << LOG_L, 1 << LOG_EXT
    C = N // l
    G = ctx.g1_bytes
    ck, _ = kzg.setup(n - 1, tau=TAU)
    rk_l = kzg.coset_verification_key(l, TAU)
    table = kzg.coset_table(ck, n, l)
    w = int(kzg.Fq.root_of_unity(N))
    w_n = _native.int_to_words(pow(w, N // n, r))
    rev_c = np.array([kzg._brp(c, LOG_EXT - LOG_L) for c in range(C)])
    rev_l = np.array([kzg._brp(t, LOG_L) for t in range(l)])
    res = {"curve": "bls12_381", "n": n, "l": l, "N": N, "reps": a.reps, "blobs": {}}

    def timed(fn):
        torch.cuda.synchronize(ctx.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(ctx.device)
        return (time.perf_counter() - t0) * 1e3, out

    def med(samples):
        return {"median": statistics.median(samples), "twice_spread": 2 * (max(samples) - min(samples)),
                "samples": [round(s, 3) for s in samples]}

    def encode(ev):
        """uint64[b, C, l, 4] limbs in the library's numbering -> uint8[b, C, 32 l] cells"""
        picked = ev[:, rev_c][:, :, rev_l]
        return np.ascontiguousarray(picked.view(np.uint8).reshape(ev.shape[0], C, l, 32)[..., ::-1]).reshape(
            ev.shape[0], C, 32 * l)

    for b in [int(s) for s in a.blobs.split(",") if s]:
        rng = np.random.default_rng(b)
        blobs = rng.integers(0, 256, size=(b, 32 * n), dtype=np.uint8)
        blobs[:, ::32] &= 0x3f                                          # every element below 2^254 < r
        state = {}

        def new():
            return kzg.compute_cells_and_kzg_proofs(table, blobs, l, N=N)

        def old():
            coeffs = np.ascontiguousarray(kzg.blob_to_values(blobs, n))
            for j in range(b):
                ctx.ntt(coeffs[j], LOG_N, w_n, True)
            xy, inf, ev = ctx.open_cosets(table.table, coeffs, [n] * b, n, LOG_EXT, w, evals=True)
            t0 = time.perf_counter()
            cells = encode(ev)
            state["encode_ms"] = (time.perf_counter() - t0) * 1e3
            comp = ctx.g1_compress(xy.reshape(b * C, -1), inf.reshape(-1)).reshape(b, C, G)[:, rev_c]
            state["coeffs"] = coeffs
            return ([[cells[j, c].tobytes() for c in range(C)] for j in range(b)],
                    [[comp[j, c].tobytes() for c in range(C)] for j in range(b)])

        _, (cells, proofs) = timed(new)
        timed(old)
        commitments = kzg.compress_g1(kzg.commit(ck, [state["coeffs"][j] for j in range(b)]))
        per_cell = [commitments[j] for j in range(b) for _ in range(C)]
        cell_idx = [c for _ in range(b) for c in range(C)]
        flat_cells = np.frombuffer(b"".join(x for row in cells for x in row), dtype=np.uint8).reshape(b * C, 32 * l)
        flat_proofs = np.frombuffer(b"".join(x for row in proofs for x in row), dtype=np.uint8).reshape(b * C, G)
        comm_idx = [j for j in range(b) for _ in range(C)]
        points = np.concatenate([np.frombuffer(b"".join(commitments), dtype=np.uint8).reshape(b, G), flat_proofs])
        coset_idx = np.asarray([kzg._brp(c, LOG_EXT - LOG_L) for c in cell_idx], dtype=np.uint32)
        key = kzg._key(ck)

        def verify():
            return kzg.verify_cell_kzg_proof_batch(ck, rk_l, per_cell, cell_idx, flat_cells, flat_proofs, l, N)

        def hash_only():
            return kzg._cell_batch_rho(n, l, commitments, comm_idx, cell_idx, flat_cells, flat_proofs)

        def decompress():
            return ctx.g1_decompress(points, check_subgroup=True)

        def fold(xy, inf, rho):
            return ctx.verify_cosets_bytes(key.srs, LOG_EXT, LOG_L, w, xy[:b], inf[:b], comm_idx, coset_idx,
                                           flat_cells, xy[b:], inf[b:], rho)

        def pairing(out_xy, out_inf):
            L_pt, R_pt = kzg._points(out_xy, out_inf)
            return kzg.pairing_check([(L_pt, kzg.G2), (kzg.neg(R_pt), rk_l)])

        t = {k: [] for k in ("new_ms", "old_ms", "old_encode_ms", "verify_ms", "hash_ms", "decompress_ms", "fold_ms",
                             "pairing_ms")}
        for rep in range(a.reps + 1):
            ms_new, got = timed(new)
            ms_old, want = timed(old)
            assert got[0] == want[0], f"{b} blobs: the cells of the new route differ from the old route's"
            assert got[1] == want[1], f"{b} blobs: the proofs of the new route differ from the old route's"
            ms_v, ok = timed(verify)
            ms_h, rho = timed(hash_only)
            ms_d, (xy, inf, status) = timed(decompress)
            ms_f, (out_xy, out_inf, bad) = timed(lambda: fold(xy, inf, rho))
            ms_p, ok_parts = timed(lambda: pairing(out_xy, out_inf))
            assert ok is True and ok_parts is True and not status.any() and not bad, f"{b} blobs: no verification"
            if rep:
                for k, v in zip(t, (ms_new, ms_old, state["encode_ms"], ms_v, ms_h, ms_d, ms_f, ms_p)):
                    t[k].append(v)
        m = {k: statistics.median(v) for k, v in t.items()}
        res["blobs"][str(b)] = {"blobs": b, "cells": b * C, **{k: med(v) for k, v in t.items()},
                                "new_over_old": m["new_ms"] / m["old_ms"], "hash_share": m["hash_ms"] / m["verify_ms"]}
        print(f"{b} blobs: new {m['new_ms']:.1f} ms, old {m['old_ms']:.1f} ms (numpy encoding {m['old_encode_ms']:.1f} "
              f"ms); verify {m['verify_ms']:.1f} ms = hash {m['hash_ms']:.1f} + decompression {m['decompress_ms']:.1f} "
              f"+ fold {m['fold_ms']:.1f} + pairing {m['pairing_ms']:.1f} ms", file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "cells_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

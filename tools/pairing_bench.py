"""Timing of pairing-product checks on one GPU, both curves, k = 2 pairs per equation,
m = 1, 64, 1024 and 4096 equations.

Per curve and m, alternating in one process:

    device_ms      kzg_pairing_check end to end from host arrays (copies, one launch, the statuses back)
    host_ms        m = 1 only: the two KZG.pairing calls of kzg_snark_amd/pairing.py and the comparison of their
                   values -- what every verifier ended with before the device call existed

    python tools/pairing_bench.py [--out DIR] [--reps 5] [--sizes 1,64,1024,4096]

The equations are e(a G1, b G2) e(-(a b [+ 1]) G1, G2) with a seeded pattern of true and false ones; every repetition's
statuses are compared with the pattern and the host's verdict with the first equation's.  Every figure is the median
of --reps runs after one warm-up.  Prints one JSON line (and writes DIR/pairing_bench.json with --out)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,64,1024,4096")
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    def med(samples):
        return {"median": statistics.median(samples), "twice_spread": 2 * (max(samples) - min(samples)),
                "samples": [round(s, 3) for s in samples]}

    res = {"k": 2, "reps": a.reps, "curves": {}}
    for curve in ("bls12_381", "bn254"):
        kzg = KZG(curve)
        ctx = kzg._context()
        L, r = ctx.fp_limbs, kzg.curve_order
        rng = random.Random(len(curve))
        sa = [rng.randrange(1, r) for _ in range(POOL)]
        sb = [rng.randrange(1, r) for _ in range(POOL)]
        A = [kzg.multiply(kzg.G1, s) for s in sa]
        B = [kzg.multiply(kzg.G2, s) for s in sb]
        g1_rows, _ = _native.points_to_limbs(A, L)
        g2_rows, _ = _native.g2_points_to_limbs(B + [kzg.G2], L)
        closing = {}

        def close_row(s):
            if s not in closing:
                closing[s] = _native.points_to_limbs([kzg.neg(kzg.multiply(kzg.G1, s % r))], L)[0][0]
            return closing[s]

        def timed(fn):
            torch.cuda.synchronize(ctx.device)
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize(ctx.device)
            return (time.perf_counter() - t0) * 1e3, out

        rows = {}
        for m in [int(s) for s in a.sizes.split(",") if s]:
            holds = [rng.randrange(2) == 0 for _ in range(m)]
            holds[0] = True
            picks = [(rng.randrange(POOL), rng.randrange(POOL)) for _ in range(m)]
            g1 = np.zeros((m, 2, 2 * L), dtype=np.uint64)
            g2 = np.zeros((m, 2, 4 * L), dtype=np.uint64)
            for e, ((i, j), h) in enumerate(zip(picks, holds)):
                g1[e, 0], g2[e, 0] = g1_rows[i], g2_rows[j]
                g1[e, 1], g2[e, 1] = close_row(sa[i] * sb[j] + (0 if h else 1)), g2_rows[POOL]
            want = [0 if h else 1 for h in holds]
            i0, j0 = picks[0]
            closer = kzg.multiply(kzg.G1, sa[i0] * sb[j0] % r)
            t_dev, t_host = [], []
            for rep in range(a.reps + 1):
                ms_d, st = timed(lambda: ctx.pairing_check(g1.reshape(-1, 2 * L), None, g2.reshape(-1, 4 * L), None, 2))
                assert list(st) == want, f"{curve}, m = {m}: the statuses differ from the pattern"
                if m == 1:
                    ms_h, ok = timed(lambda: kzg.pairing(B[j0], A[i0]) == kzg.pairing(kzg.G2, closer))
                    assert ok is True
                if rep:
                    t_dev.append(ms_d)
                    if m == 1:
                        t_host.append(ms_h)
            rows[str(m)] = {"m": m, "device_ms": med(t_dev), **({"host_ms": med(t_host)} if m == 1 else {}),
                            "device_us_per_equation": 1e3 * statistics.median(t_dev) / m}
            print(f"{curve} m = {m}: device {statistics.median(t_dev):.2f} ms"
                  + (f", host {statistics.median(t_host):.1f} ms" if m == 1 else ""), file=sys.stderr, flush=True)
        res["curves"][curve] = rows
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "pairing_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

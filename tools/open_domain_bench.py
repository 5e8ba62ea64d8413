"""Timing of FK20 openings on one GPU: table build, kzg_open_domain for several batch sizes, and the
per-point path it replaces (pipelined kzg_open_device_async at every point of the domain).

    python tools/open_domain_bench.py --out DIR [--curve bls12_381] [--reps 5] [--table-logs 12,16,20]
                                      [--open 12:1,12:8,12:32,12:64,16:1,20:1] [--per-point-logs 12,16,20]

Every figure is the median of --reps runs after one warm-up; each repetition spot-checks proofs against kzg_open.
The per-point path runs all 4096 points at 2^12; above that --sample points, scaled to n (labelled extrapolated).
Writes DIR/open_domain_bench.json and prints it."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--curve", default="bls12_381")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--table-logs", default="12,16,20")
    ap.add_argument("--open", default="12:1,12:8,12:32,12:64,16:1,20:1")
    ap.add_argument("--per-point-logs", default="12,16,20")
    ap.add_argument("--sample", type=int, default=1024)
    a = ap.parse_args()

    import numpy as np
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG(a.curve)
    ctx = kzg._context()
    r = kzg.curve_order
    rng = random.Random(1)
    opens = [tuple(int(x) for x in s.split(":")) for s in a.open.split(",") if s]
    logs = sorted({int(x) for x in a.table_logs.split(",") if x} | {lg for lg, _ in opens}
                  | {int(x) for x in a.per_point_logs.split(",") if x})
    res = {"curve": a.curve, "reps": a.reps, "table_ms": {}, "open_domain_ms": {}, "per_point": {}}
    one = _native.int_to_words(1)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    for lg in logs:
        n = 1 << lg
        ck = kzg.setup(n - 1, tau=rng.randrange(r))[0]
        w = int(kzg.Fq.root_of_unity(n))
        tables = []
        if str(lg) in a.table_logs.split(","):
            samples = []
            for rep in range(a.reps + 1):
                ms, t = timed(lambda: ctx.domain_table(ck.srs, lg))
                if rep:
                    samples.append(ms)
                tables.append(t)
                while len(tables) > 1:
                    tables.pop(0).close()
            res["table_ms"][str(lg)] = {"median": statistics.median(samples), "samples": samples}
        table = tables[-1] if tables else ctx.domain_table(ck.srs, lg)
        for olg, b in opens:
            if olg != lg:
                continue
            arr = _native.ints_to_limbs([rng.randrange(r) for _ in range(b * n)]).reshape(b, n, 4).copy()
            samples = []
            for rep in range(a.reps + 1):
                ms, (xy, inf, _) = timed(lambda: ctx.open_domain(table, arr, [n] * b, n, w, evals=False))
                j, i = rng.randrange(b), rng.randrange(n)          # spot check against kzg_open
                pxy, pinf, _ = ctx.open(ck.srs, arr[j:j + 1], [n], n, _native.int_to_words(pow(w, i, r)), one)
                assert np.array_equal(xy[j, i], pxy) and inf[j, i] == pinf[0], (lg, b, j, i)
                if rep:
                    samples.append(ms)
            med = statistics.median(samples)
            res["open_domain_ms"][f"{lg}:{b}"] = {"median": med, "per_poly": med / b, "samples": samples}
            print(f"open_domain 2^{lg} b={b}: {med:.1f} ms ({med / b:.2f} ms per polynomial)", flush=True)
        if str(lg) in a.per_point_logs.split(","):
            import torch
            arr = _native.ints_to_limbs([rng.randrange(r) for _ in range(n)]).copy()
            d = torch.from_numpy(arr.view(np.int64)).to(f"cuda:{ctx.device}")
            torch.cuda.synchronize(ctx.device)
            m = n if n <= 4096 else min(a.sample, n)
            outs = [(np.zeros(2 * ctx.fp_limbs, np.uint64), np.zeros(1, np.uint8), np.zeros(4, np.uint64))
                    for _ in range(m)]
            samples = []
            for rep in range(a.reps + 1):
                def loop():
                    for i in range(m):
                        ctx.open_device_async(ck.srs, d.data_ptr(), [n], n, _native.int_to_words(pow(w, i, r)), one,
                                              *outs[i])
                    ctx.commit_flush()
                ms, _ = timed(loop)
                if rep:
                    samples.append(ms)
            med = statistics.median(samples)
            res["per_point"][str(lg)] = {"points_run": m, "median_ms": med, "all_points_ms": med * n / m,
                                         "extrapolated": m < n, "samples": samples}
            print(f"per-point 2^{lg}: {m} points {med:.1f} ms -> all {med * n / m:.1f} ms"
                  f"{' (extrapolated)' if m < n else ''}", flush=True)
        for t in tables:
            t.close()
        ck.srs.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "open_domain_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items()}, default=str)[:4000])


if __name__ == "__main__":
    main()

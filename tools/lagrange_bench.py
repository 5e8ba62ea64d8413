"""Timing of evaluation-form KZG on one GPU: Lagrange key build by both routes, and the opening
from values against what a caller without it needs (one inverse NTT per vector, then the coefficient opening).

    python tools/lagrange_bench.py --out DIR [--curve bls12_381] [--reps 20] [--key-reps 20] [--key-logs 16,20]

Writes DIR/lagrange_bench.json (medians in ms, every sample kept) and prints it.  The two openings alternate in one
process, so clock and thermal drift hit both alike."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    return statistics.median(xs) if xs else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--curve", default="bls12_381")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--key-reps", type=int, default=20)
    ap.add_argument("--key-logs", default="16,20")
    ap.add_argument("--open-log", type=int, default=20)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.field import GF
    from kzg_snark_amd import curve as _curve

    r = _curve.CURVES[a.curve].r
    F = GF(r)
    ctx = _native.Context(a.curve)
    tau = 0x1234_5678_9abc_def0_0fed_cba9_8765_4321 % r
    tw = _native.int_to_words(tau)
    res = {"curve": a.curve, "reps": a.reps, "key_reps": a.key_reps, "warmup": a.warmup, "key_build_ms": {},
           "device": torch.cuda.get_device_name(0)}

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for log_n in [int(x) for x in a.key_logs.split(",") if x]:
        n = 1 << log_n
        w = int(F.root_of_unity(n))
        mono = ctx.srs_generate(tw, n)
        samples = {"from_tau": [], "from_monomial": []}
        for rep in range(a.warmup + a.key_reps):
            for route in ("from_tau", "from_monomial"):
                if route == "from_tau":
                    ms, lk = timed(lambda: ctx.srs_generate_lagrange(tw, log_n, w))
                else:
                    ms, lk = timed(lambda: ctx.srs_lagrange(mono, log_n, w))
                lk.close()
                if rep >= a.warmup:
                    samples[route].append(ms)
        mono.close()
        res["key_build_ms"][str(log_n)] = {k: {"median": med(v), "samples": v} for k, v in samples.items()}
        print(f"key 2^{log_n}: from tau {med(samples['from_tau']):.1f} ms, from the monomial key "
              f"{med(samples['from_monomial']):.1f} ms", flush=True)

    log_n, k = a.open_log, a.k
    n = 1 << log_n
    w = int(F.root_of_unity(n))
    ww = _native.int_to_words(w)
    mono = ctx.srs_generate(tw, n)
    lk = ctx.srs_generate_lagrange(tw, log_n, w)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    vals = torch.randint(0, 1 << 62, (k, n, 4), generator=g, dtype=torch.int64, device="cuda:0")
    vals[..., 3] >>= 4
    work = torch.empty_like(vals)
    torch.cuda.synchronize()
    z, xi = _native.int_to_words(0x5a5a5a5a5a % r), _native.int_to_words(0x3c3c3c3c3c % r)

    def evals_open():
        return ctx.open_evals(lk, vals.data_ptr(), [n] * k, n, z, xi, device=True)

    def intt_then_open():                    # the values are copied to `work` before the clock starts
        ctx.ntt_device(work.data_ptr(), log_n, ww, True, batch=k)
        return ctx.open(mono, work.data_ptr(), [n] * k, n, z, xi, device=True)

    samples = {"open_evaluations": [], "intt_plus_open": []}
    for rep in range(a.warmup + a.reps):
        ms_a, pa = timed(evals_open)
        work.copy_(vals)
        torch.cuda.synchronize()
        ms_b, pb = timed(intt_then_open)
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb)), "the two openings differ"
        if rep >= a.warmup:
            samples["open_evaluations"].append(ms_a)
            samples["intt_plus_open"].append(ms_b)
    res["open"] = {"log_n": log_n, "k": k, **{key: {"median": med(v), "samples": v} for key, v in samples.items()}}
    print(f"open 2^{log_n} x {k}: from values {med(samples['open_evaluations']):.3f} ms, {k} INTTs + open "
          f"{med(samples['intt_plus_open']):.3f} ms", flush=True)
    lk.close()
    mono.close()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "lagrange_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "key_build_ms"} | {
        "key_build_ms": {lg: {rt: d["median"] for rt, d in v.items()} for lg, v in res["key_build_ms"].items()}}))


if __name__ == "__main__":
    main()

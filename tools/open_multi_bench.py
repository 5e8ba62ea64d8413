"""Timing of the Shplonk opening on one GPU, BLS12-381, n = 2^20 coefficients per polynomial, the
polynomials resident on the device.  Three legs, every figure the median of --reps runs after one warm-up:

  (a) plonk     the PLONK shape: 6 polynomials opened at {zeta} and 1 at {zeta, zeta g}.
        open_multi_ms  the three device calls KZG.open_multi makes: kzg_fr_poly_eval_batch (7 x 2),
                       kzg_open_points_device (7 polynomials, 2 points, q kept on the device) and
                       kzg_open_points_device (7 polynomials and q, the one point zeta')
        two_opens_ms   what plonk_device.py does today: kzg_open_device of the 7 polynomials at zeta and of the one at
                       zeta g
      The two alternate in one process.  Per repetition the multi proof is checked with check_multi and the first plain
      opening with check (device and host pairings); the warm-up also compares the three calls with KZG.open_multi.
  (b) eval      kzg_fr_poly_eval_batch at k = 9, t = 2 against the 18 kzg_fr_poly_eval calls, alternating, the values
                compared per repetition.
  (c) span      the "open_points_poly" span (HIP events around the polynomial stage) of kzg_open_points_device at
                k = 6 and t = 1, 2, 4, 8, with the "open_poly" span of kzg_open_device at k = 6 beside it.

    python tools/open_multi_bench.py [--out DIR] [--reps 5] [--log-n 20]

Prints one JSON line (and writes DIR/open_multi_bench.json with --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x1d0c_7e5a_9b3f_2468_ace0_1357_9bdf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-n", type=int, default=20)
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG("bls12_381")
    ctx = kzg._context()
    r = kzg.curve_order
    n = 1 << a.log_n
    K = 9                                                            # polynomials on the device, one per row
    res = {"curve": "bls12_381", "n": n, "reps": a.reps}

    def timed(fn):
        torch.cuda.synchronize(ctx.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(ctx.device)
        return (time.perf_counter() - t0) * 1e3, out

    def med(samples):
        return {"median": round(statistics.median(samples), 4), "samples": [round(s, 4) for s in samples]}

    rng = np.random.default_rng(a.log_n)
    rows = rng.integers(0, 1 << 63, size=(K, n, 4), dtype=np.uint64)
    rows[..., 3] %= np.uint64(r >> 192)                              # reduced
    d =kzg._upload(ctx, rows)
    base = d.data_ptr()
    row = lambda i: base + i * n * 32
    ck, rk = kzg.setup(n - 1, tau=TAU)
    words = _native.int_to_words

    # ---- (a) the PLONK shape ----------------------------------------------------------------------------------------
    k = 7
    g = int(kzg.Fq.root_of_unity(n))
    zeta, gamma, zeta2 = (0x9e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251f86c6a11d0c18e95 * s % r for s in (1, 3, 5))
    sets = [[zeta]] * 6 + [[zeta, zeta * g % r]]
    T = [zeta, zeta * g % r]
    gp = [pow(gamma, i + 1, r) for i in range(k)]
    inv = lambda v: pow(v % r, -1, r)
    w1 = [[gp[i], 0] for i in range(6)] + [[gp[6] * inv(T[0] - T[1]) % r, gp[6] * inv(T[1] - T[0]) % r]]
    w2 = [[gp[i] * (zeta2 - T[1]) % r] for i in range(6)] + [[gp[6]], [-(zeta2 - T[0]) * (zeta2 - T[1]) % r]]
    lens = [n] * k

    # the second call takes q as row k of the strided array: the first call leaves it there
    def multi_calls():
        values = ctx.poly_eval_batch(base, lens, n, T)
        W = ctx.open_points(ck.srs, base, lens, n, T, w1, d_quot=row(k), device=True)
        W2 = ctx.open_points(ck.srs, base, lens + [n - 1], n, [zeta2], w2, device=True)
        return values, W, W2

    def two_opens():
        first = ctx.open(ck.srs, base, lens, n, words(zeta), words(gamma), device=True)
        second = ctx.open(ck.srs, row(6), [n], n, words(T[1]), words(gamma), device=True)
        return first, second

    polys = [rows[i] for i in range(k)]
    saved = rows[k].copy()                                           # row k is overwritten by q: restored after the leg
    comms = kzg.commit(ck, polys)
    facade = kzg.open_multi(ck, polys, sets, gamma, zeta2)
    ms_multi, ms_two = [], []
    for rep in range(a.reps + 1):
        t_m, (values, W, W2) = timed(multi_calls)
        t_o, (first, second) = timed(two_opens)
        proof = (kzg._points(*W)[0], kzg._points(*W2)[0])
        evals = [[values[i][0]] for i in range(6)] + [values[6]]
        assert kzg.check_multi(rk, comms, sets, evals, proof, gamma, zeta2) is True, "open_multi: the proof fails"
        pt = kzg._points(first[0], first[1])[0]
        assert kzg.check(rk, comms, zeta, [values[i][0] for i in range(k)], pt, gamma), "kzg_open_device: the proof fails"
        if rep == 0:
            assert proof == (facade.W, facade.W2) and evals == facade.evaluations, "the calls differ from KZG.open_multi"
        else:
            ms_multi.append(t_m)
            ms_two.append(t_o)
    d[k].copy_(torch.from_numpy(saved.view(np.int64)))
    torch.cuda.synchronize(ctx.device)
    res["plonk"] = {"polynomials": k, "points": 2, "open_multi_ms": med(ms_multi), "two_opens_ms": med(ms_two),
                    "multi_over_two_opens": round(statistics.median(ms_multi) / statistics.median(ms_two), 4)}
    print(f"plonk shape: open_multi {statistics.median(ms_multi):.2f} ms, two opens {statistics.median(ms_two):.2f} ms",
          file=sys.stderr, flush=True)

    # ---- (b) batched evaluation -------------------------------------------------------------------------------------
    pts = [zeta, zeta2]
    ms_batch, ms_loop = [], []
    for rep in range(a.reps + 1):
        t_b, got = timed(lambda: ctx.poly_eval_batch(base, [n] * K, n, pts))
        t_l, want = timed(lambda: [[ctx.poly_eval(n, row(i), z) for z in pts] for i in range(K)])
        assert got == want, "kzg_fr_poly_eval_batch differs from kzg_fr_poly_eval"
        if rep:
            ms_batch.append(t_b)
            ms_loop.append(t_l)
    res["eval"] = {"polynomials": K, "points": 2, "batch_ms": med(ms_batch), "loop_ms": med(ms_loop),
                   "batch_over_loop": round(statistics.median(ms_batch) / statistics.median(ms_loop), 4)}
    print(f"evaluation 9 x 2: batch {statistics.median(ms_batch):.3f} ms, 18 calls {statistics.median(ms_loop):.3f} ms",
          file=sys.stderr, flush=True)

    # ---- (c) the polynomial stage by the number of points ------------------------------------------------------------
    k = 6
    ctx.prof_enable(True)
    spans = {}
    wrng = np.random.default_rng(7)
    scalar = lambda: int.from_bytes(wrng.bytes(31), "little")
    for t in (1, 2, 4, 8):
        points = [scalar() for _ in range(t)]
        weights = [[scalar() for _ in range(t)] for _ in range(k)]
        samples = []
        for rep in range(a.reps + 1):
            ctx.prof_reset()
            ctx.open_points(ck.srs, base, [n] * k, n, points, weights, device=True)
            ms, count = ctx.prof_read("open_points_poly")
            assert count == 1
            if rep:
                samples.append(ms)
        spans[str(t)] = med(samples)
    samples = []
    for rep in range(a.reps + 1):
        ctx.prof_reset()
        ctx.open(ck.srs, base, [n] * k, n, words(zeta), words(gamma), device=True)
        ms, count = ctx.prof_read("open_poly")
        assert count == 1
        if rep:
            samples.append(ms)
    ctx.prof_enable(False)
    res["span"] = {"polynomials": k, "open_points_poly_ms": spans, "open_poly_ms": med(samples)}
    print("open_points_poly at k = 6: " + ", ".join(f"t={t} {v['median']:.3f} ms" for t, v in spans.items())
          + f"; open_poly {statistics.median(samples):.3f} ms", file=sys.stderr, flush=True)

    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "open_multi_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Timing of bulk verification at arbitrary points on one GPU, BLS12-381.

Claims leg, K = 64, 4096, 2^16 and 2^20: every proof of kzg_open_domain for one polynomial of K coefficients, so the
claims sit at domain points and three routes see the same input.  Per K, alternating in one process:

    verify_points_ms   kzg_verify_points end to end from host arrays (z_k = w^k handed over as plain scalars)
    verify_cosets_ms   kzg_verify_cosets with l = 1 on the same claims (the slice route of 4.7)
    table_route_ms     tools/verify_bench.py's table route: kzg_srs_load_g1 of the K proofs, kzg_commit of the two
                       K-long scalar vectors r_k and r_k z_k against that key, kzg_srs_free; the values are left out

Blobs leg, 64 and 1024 blobs of 4096 values: commitments against a Lagrange key, one kzg_open_evals proof per blob at
its own random challenge, then

    eval_ms            kzg_fr_eval_lagrange_batch of all blobs from host arrays
    fold_ms            kzg_verify_points of the resulting claims

    python tools/verify_points_bench.py [--out DIR] [--reps 5] [--sizes 64,4096,65536,1048576] [--blobs 64,1024]

Every figure is the median of --reps runs after one warm-up.  Every repetition is checked on the host through the
trapdoor, L == tau R; the two device routes must return the same two points, and the table route's sum_k r_k pi_k must
equal R.  Prints one JSON line (and writes DIR/verify_points_bench.json with --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x1d0c_7e5a_9b3f_2468_ace0_1357_9bdf
BLOB_LOG_N = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64,4096,65536,1048576")
    ap.add_argument("--blobs", default="64,1024")
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG("bls12_381")
    ctx = kzg._context()
    r = kzg.curve_order
    rho = 0x9e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251f86c6a11d0c18e95 % r
    res = {"curve": "bls12_381", "reps": a.reps, "claims": {}, "blobs": {}}

    def timed(fn):
        torch.cuda.synchronize(ctx.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(ctx.device)
        return (time.perf_counter() - t0) * 1e3, out

    def med(samples):
        return {"median": statistics.median(samples), "samples": [round(s, 3) for s in samples]}

    def spread(samples):
        return max(samples) - min(samples)

    def random_elements(rng, shape):
        v = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
        v[..., 3] %= np.uint64(r >> 192)                           # reduced
        return v

    def trapdoor(xy, inf, what):
        L_pt, R_pt = kzg._points(xy, inf)
        assert L_pt == kzg.multiply(R_pt, TAU % r), f"{what}: L != tau R"

    for K in [int(s) for s in a.sizes.split(",") if s]:
        log_n = K.bit_length() - 1
        assert K == 1 << log_n and log_n >= 1
        ck = kzg.setup(K - 1, tau=TAU)[0]
        w = int(kzg.Fq.root_of_unity(K))
        poly = random_elements(np.random.default_rng(log_n), (1, K))
        cxy, cinf = ctx.commit(ck.srs, poly, [K], K)
        table = ctx.domain_table(ck.srs, log_n)
        pxy, pinf, ev = ctx.open_domain(table, poly, [K], K, w, evals=True)
        table.close()
        pxy = np.ascontiguousarray(pxy.reshape(K, -1))
        pinf = np.ascontiguousarray(pinf.reshape(K))
        ys = np.ascontiguousarray(ev.reshape(K, 4))
        ci = np.zeros(K, dtype=np.uint32)
        ki = np.arange(K, dtype=np.uint32)
        zs, rs, ss, x, z = [], [], [], 1, 1                       # the points and the table route's scalars (not timed)
        for k in range(K):
            x = x * rho % r
            zs.append(z)
            rs.append(x)
            ss.append(x * z % r)
            z = z * w % r
        zl = _native.ints_to_limbs(zs)
        scal = np.ascontiguousarray(_native.ints_to_limbs(rs + ss).reshape(2, K, 4))
        del zs, rs, ss

        def table_route():
            key = ctx.srs_load_g1(pxy, pinf)
            out = ctx.commit(key, scal, [K, K], K)
            key.close()
            return out

        pts, cos, tab = [], [], []
        for rep in range(a.reps + 1):
            ms_p, (xy, inf) = timed(lambda: ctx.verify_points(cxy, cinf, ci, zl, ys, pxy, pinf, rho))
            ms_c, (xy_c, inf_c) = timed(lambda: ctx.verify_cosets(ck.srs, log_n, 0, w, cxy, cinf, ci, ki,
                                                                  ys.reshape(K, 1, 4), pxy, pinf, rho))
            ms_t, (txy, tinf) = timed(table_route)
            trapdoor(xy, inf, f"K={K}")
            assert np.array_equal(xy, xy_c) and np.array_equal(inf, inf_c), f"K={K}: the two routes differ"
            assert np.array_equal(txy[0], xy[1]) and tinf[0] == inf[1], f"K={K}: the table route's R differs"
            if rep:
                pts.append(ms_p)
                cos.append(ms_c)
                tab.append(ms_t)
        nbytes, _ = ctx.prof_read("verify_points_device_bytes")
        gain = statistics.median(cos) - statistics.median(pts)
        res["claims"][str(K)] = {
            "K": K, "verify_points_ms": med(pts), "verify_cosets_ms": med(cos), "table_route_ms": med(tab),
            "points_over_cosets": statistics.median(pts) / statistics.median(cos),
            "points_over_table_route": statistics.median(pts) / statistics.median(tab),
            # the comparison DESIGN 4.10 asks for: does verify_points win by more than twice the spread of the samples?
            "cosets_minus_points_ms": gain, "twice_spread_ms": 2 * max(spread(pts), spread(cos)),
            "points_win_beyond_spread": gain > 2 * max(spread(pts), spread(cos)),
            "verify_points_device_bytes": int(nbytes),
        }
        print(f"K={K}: verify_points {statistics.median(pts):.2f} ms, verify_cosets {statistics.median(cos):.2f} ms, "
              f"table route {statistics.median(tab):.2f} ms", file=sys.stderr, flush=True)
        ck.srs.close()

    blob_counts = [int(s) for s in a.blobs.split(",") if s]
    if blob_counts:
        n = 1 << BLOB_LOG_N
        lk, _ = kzg.setup_lagrange(n, tau=TAU)
        w = lk.w
        one = _native.int_to_words(1)
    for b in blob_counts:
        rng = np.random.default_rng(b)
        blobs = random_elements(rng, (b, n))
        zl = random_elements(rng, (b,))
        cxy, cinf = ctx.commit(lk.srs, blobs, [n] * b, n)
        pxy = np.zeros((b, 2 * ctx.fp_limbs), dtype=np.uint64)
        pinf = np.zeros(b, dtype=np.uint8)
        want = np.zeros((b, 4), dtype=np.uint64)
        for j in range(b):
            xy, inf, y = ctx.open_evals(lk.srs, blobs[j:j + 1], [n], n, zl[j], one)
            pxy[j], pinf[j], want[j] = xy, inf[0], y
        ci = np.arange(b, dtype=np.uint32)
        evs, folds = [], []
        for rep in range(a.reps + 1):
            ms_e, ys = timed(lambda: ctx.eval_lagrange_batch(BLOB_LOG_N, w, blobs, [n] * b, n, zl))
            ms_f, (xy, inf) = timed(lambda: ctx.verify_points(cxy, cinf, ci, zl, ys, pxy, pinf, rho))
            assert np.array_equal(ys, want), f"{b} blobs: the batched values differ from kzg_open_evals'"
            trapdoor(xy, inf, f"{b} blobs")
            if rep:
                evs.append(ms_e)
                folds.append(ms_f)
        res["blobs"][str(b)] = {
            "blobs": b, "values_per_blob": n, "eval_ms": med(evs), "fold_ms": med(folds),
            "verify_blobs_ms": statistics.median(evs) + statistics.median(folds),
            "us_per_blob": 1e3 * (statistics.median(evs) + statistics.median(folds)) / b,
        }
        print(f"{b} blobs: evaluation {statistics.median(evs):.2f} ms, fold {statistics.median(folds):.2f} ms",
              file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "verify_points_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

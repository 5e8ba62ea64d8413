"""Timing of bulk verification on one GPU, BLS12-381, at four shapes: the PeerDAS shape (n = 2^12,
N = 2^13, l = 64, 32 blobs), 2^16 with l = 64, 2^20 with N = 2n and l = 16, and every proof of kzg_open_domain at 2^20
(l = 1, K = 2^20).  Per shape, alternating in one process:

    verify_ms       kzg_verify_cosets end to end from host arrays
    table_route_ms  what the library offered before it: kzg_srs_load_g1 of the K proofs, kzg_commit of two K-long scalar
                    vectors (r_k and r_k a_k) against that key, kzg_srs_free; the fold of the values is left out
    prove_ms        kzg_open_cosets / kzg_open_domain (with the values) for the same shape

    python tools/verify_bench.py [--out DIR] [--reps 5] [--shapes peerdas,2^16,2^20,domain]

Every figure is the median of --reps runs after one warm-up.  Every repetition is checked on the host: L == tau^l R
through the trapdoor, and the table route's sum_k r_k pi_k equals R.  Prints one JSON line (and writes
DIR/verify_bench.json with --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {                      # name: (log_n, log_N, log_l, polynomials)
    "peerdas": (12, 13, 6, 32),
    "2^16": (16, 16, 6, 1),
    "2^20": (20, 21, 4, 1),
    "domain": (20, 20, 0, 1),
}
TAU = 0x1d0c_7e5a_9b3f_2468_ace0_1357_9bdf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="peerdas,2^16,2^20,domain")
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG("bls12_381")
    ctx = kzg._context()
    r = kzg.curve_order
    rho = 0x9e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251f86c6a11d0c18e95 % r
    res = {"curve": "bls12_381", "reps": a.reps, "shapes": {}}
    keys = {}

    def timed(fn):
        torch.cuda.synchronize(ctx.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(ctx.device)
        return (time.perf_counter() - t0) * 1e3, out

    def med(samples):
        return {"median": statistics.median(samples), "samples": [round(s, 3) for s in samples]}

    for name in [s for s in a.shapes.split(",") if s]:
        log_n, log_N, log_l, b = SHAPES[name]
        n, N, l = 1 << log_n, 1 << log_N, 1 << log_l
        if log_n not in keys:
            keys[log_n] = kzg.setup(n - 1, tau=TAU)[0]
        ck = keys[log_n]
        w = int(kzg.Fq.root_of_unity(N))
        rng = np.random.default_rng(log_n + log_l)
        polys = rng.integers(0, 1 << 63, size=(b, n, 4), dtype=np.uint64)
        polys[..., 3] %= np.uint64(r >> 192)                       # reduced
        cxy, cinf = ctx.commit(ck.srs, polys, [n] * b, n)
        table = ctx.domain_table(ck.srs, log_n) if l == 1 else ctx.coset_table(ck.srs, log_n, log_l)

        def prove():
            if l == 1:
                return ctx.open_domain(table, polys, [n] * b, n, w, evals=True)
            return ctx.open_cosets(table, polys, [n] * b, n, log_N, w, evals=True)

        C = N // l
        K = b * C
        ci = np.repeat(np.arange(b, dtype=np.uint32), C)
        ki = np.tile(np.arange(C, dtype=np.uint32), b)
        # the table route's scalars r_k = rho^(k+1) and s_k = r_k w^(i_k l), from the host (not timed)
        wl = pow(w, l, r)
        apow = [1] * C
        for i in range(1, C):
            apow[i] = apow[i - 1] * wl % r
        rs, ss, x = [], [], 1
        for k in range(K):
            x = x * rho % r
            rs.append(x)
            ss.append(x * apow[k % C] % r)
        scal = np.ascontiguousarray(_native.ints_to_limbs(rs + ss).reshape(2, K, 4))
        del rs, ss, apow
        tl = pow(TAU, l, r)

        def table_route(pxy, pinf):
            key = ctx.srs_load_g1(pxy, pinf)
            out = ctx.commit(key, scal, [K, K], K)
            key.close()
            return out

        ver, tab, prv = [], [], []
        for rep in range(a.reps + 1):
            ms_p, (pxy, pinf, ev) = timed(prove)
            pxy = np.ascontiguousarray(pxy.reshape(K, -1))
            pinf = np.ascontiguousarray(pinf.reshape(K))
            vals = ev.reshape(K, l, 4)
            ms_v, (xy, inf) = timed(lambda: ctx.verify_cosets(ck.srs, log_N, log_l, w, cxy, cinf, ci, ki, vals, pxy,
                                                              pinf, rho))
            ms_t, (txy, tinf) = timed(lambda: table_route(pxy, pinf))
            L_pt, R_pt = kzg._points(xy, inf)
            assert L_pt == kzg.multiply(R_pt, tl), f"{name}: L != tau^l R"
            assert np.array_equal(txy[0], xy[1]) and tinf[0] == inf[1], f"{name}: the table route's R differs"
            if rep:
                ver.append(ms_v)
                tab.append(ms_t)
                prv.append(ms_p)
        nbytes, _ = ctx.prof_read("verify_device_bytes")
        table.close()
        fp = ctx.fp_limbs
        rec_bytes = 128 if fp == 6 else 96
        win = 13 if K >= (1 << 18) else 16
        res["shapes"][name] = {
            "log_n": log_n, "log_N": log_N, "l": l, "polys": b, "K": K,
            "verify_ms": med(ver), "table_route_ms": med(tab), "prove_ms": med(prv),
            "verify_over_table_route": statistics.median(ver) / statistics.median(tab),
            "verify_over_prove": statistics.median(ver) / statistics.median(prv),
            "verify_device_bytes": int(nbytes), "verify_device_bytes_per_proof": nbytes / K,
            "record_bytes": rec_bytes, "loaded_key_bytes": win * K * rec_bytes,
        }
        print(f"{name}: K={K} verify {statistics.median(ver):.2f} ms, table route {statistics.median(tab):.2f} ms, "
              f"prove {statistics.median(prv):.2f} ms, {nbytes / K:.0f} B of device memory per proof", file=sys.stderr,
              flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "verify_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

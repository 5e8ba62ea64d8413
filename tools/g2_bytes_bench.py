"""Timing of compressed G2 points, subgroup checks on the twist and trusted-setup files on one GPU.
Per curve and per n in 2^12, 2^16 (4096 distinct points of G2, P_i = P_(i-1) + D, repeated to fill n), alternating in
one process, per repetition:

    decompress_ms            kzg_g2_decompress_device, check_subgroup = 0: the decoding kernel (the "g2_decompress" span)
    decompress_checked_ms    the same with check_subgroup = 1: decoding plus the subgroup kernel
    check_affine_ms          kzg_g2_check_subgroup alone (the "g2_subgroup" span: copies in and out included)

and, once per curve, a trusted-setup file of n1 = 4096 G1 points in both bases and n2 = 65 G2 powers:

    load_unchecked_ms        KZG.load_trusted_setup(check=False): parsing, the three decompressions, two key expansions
    load_checked_ms          the same with check=True: plus check_key (one commit, one pairing call, one G1 transform)

    python tools/g2_bytes_bench.py [--out DIR] [--reps 10] [--curves bls12_381,bn254]

Every figure is the median of --reps runs after one warm-up; the variants of a repetition run one after the other, so
drift hits them alike.  Every repetition is checked: all statuses 0 and the points those that were compressed.  Prints
one JSON line (and writes DIR/g2_bytes_bench.json with --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x2b7e_1516_28ae_d2a6_abf7_1588_09cf
DISTINCT = 1 << 12


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": [round(s, 3) for s in v]}


def bench_curve(curve, reps):
    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG(curve)
    ctx = kzg._context()
    L, size = ctx.fp_limbs, ctx.g2_bytes
    G = kzg._g2
    d = G.multiply(kzg.G2, 0x5eed_0bad_cafe)
    pts = [G.multiply(kzg.G2, 0x1234_5678_9abc_def1)]
    for _ in range(DISTINCT - 1):
        pts.append(G.add(pts[-1], d))
    xy0, inf0 = _native.g2_points_to_limbs(pts, L)
    blobs0 = ctx.g2_compress(xy0, inf0)
    dev = f"cuda:{ctx.device}"
    ctx.prof_enable(True)
    out = {}
    for log_n in (12, 16):
        n = 1 << log_n
        xy, inf = np.tile(xy0, (n // DISTINCT, 1)), np.tile(inf0, n // DISTINCT)
        blobs = np.tile(blobs0, (n // DISTINCT, 1))
        d_bytes = torch.from_numpy(blobs.reshape(-1)).to(dev)
        d_xy = torch.zeros(n * 4 * L, dtype=torch.int64, device=dev)
        d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        want_xy = torch.from_numpy(xy.view(np.int64).reshape(-1)).to(dev)

        def device_form(check):
            ctx.prof_reset()
            d_st.fill_(9)
            torch.cuda.synchronize(ctx.device)
            ctx.g2_decompress_device(d_bytes.data_ptr(), n, check, d_xy.data_ptr(), d_inf.data_ptr(), d_st.data_ptr())
            ms, count = ctx.prof_read("g2_decompress")
            assert count == 1
            assert not bool(d_st.any()) and not bool(d_inf.any()) and bool(torch.equal(d_xy, want_xy))
            return ms

        def affine():
            ctx.prof_reset()
            st = ctx.g2_check_subgroup(xy, inf)
            ms, count = ctx.prof_read("g2_subgroup")
            assert count == 1 and not st.any()
            return ms

        names = ["decompress_ms", "decompress_checked_ms", "check_affine_ms"]
        samples = {k: [] for k in names}
        for rep in range(reps + 1):
            row = {"decompress_ms": device_form(False), "decompress_checked_ms": device_form(True),
                   "check_affine_ms": affine()}
            if rep:
                for k in names:
                    samples[k].append(row[k])
        res = {k: summary(v) for k, v in samples.items()}
        res["subgroup_kernel_ms"] = res["decompress_checked_ms"]["median"] - res["decompress_ms"]["median"]
        out[f"n=2^{log_n}"] = res
        for k in names:
            print(f"{curve} n=2^{log_n} {k}: {res[k]['median']:.3f} ms", file=sys.stderr)
    ctx.prof_enable(False)

    # the trusted-setup file
    n1, n2 = 4096, 65
    ck, _ = kzg.setup(n1 - 1, tau=TAU)
    g2 = kzg.setup_g2(n2, TAU)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "setup.txt")
        kzg.save_trusted_setup(path, ck, g2)

        def load(check):
            ctx.synchronize()
            t0 = time.perf_counter()
            ts = kzg.load_trusted_setup(path, check=check)
            ctx.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            assert len(ts.monomial) == n1 and ts.g2 == g2
            ts.monomial.srs.close()
            ts.lagrange.srs.close()
            return ms

        samples = {"load_unchecked_ms": [], "load_checked_ms": []}
        for rep in range(reps + 1):
            row = {"load_unchecked_ms": load(False), "load_checked_ms": load(True)}
            if rep:
                for k in samples:
                    samples[k].append(row[k])
    out["trusted_setup n1=4096 n2=65"] = {k: summary(v) for k, v in samples.items()}
    for k, v in samples.items():
        print(f"{curve} {k}: {statistics.median(v):.1f} ms", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--curves", default="bls12_381,bn254")
    a = ap.parse_args()
    res = {"reps": a.reps, **{c: bench_curve(c, a.reps) for c in a.curves.split(",")}}
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "g2_bytes_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Timing of compressed G1 points and subgroup checks on one GPU, BLS12-381, n = 2^20 points of a
real key ([tau^i] G1).  Alternating in one process, per repetition:

    decompress_ms            kzg_g1_decompress_device, check_subgroup = 0: the kernel alone (the "g1_decompress" span)
    decompress_checked_ms    the same with check_subgroup = 1: decoding plus the subgroup kernel
    decompress_host_ms       kzg_g1_decompress (check_subgroup = 1) end to end from host arrays, copies included
    check_affine_ms          kzg_g1_check_subgroup end to end from host arrays (96 B per point go to the device first)
    load_compressed_ms       kzg_srs_load_g1_compressed (check_subgroup = 1) + kzg_srs_free
    load_affine_ms           kzg_srs_load_g1 of the same key + kzg_srs_free: the route without this feature, which still
                             leaves the caller 2^20 square roots on the host before it

    python tools/g1_bytes_bench.py [--out DIR] [--reps 20] [--log-n 20]

Every figure is the median of --reps runs after one warm-up.  Every repetition is checked: all statuses 0, the points
equal the key's own export, the reloaded key exports the same points.  Prints one JSON line (and writes
DIR/g1_bytes_bench.json with --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x2b7e_1516_28ae_d2a6_abf7_1588_09cf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log-n", type=int, default=20)
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd.kzg import KZG

    kzg = KZG("bls12_381")
    ctx = kzg._context()
    n = 1 << a.log_n
    L, size = ctx.fp_limbs, ctx.g1_bytes
    ck, _ = kzg.setup(n - 1, tau=TAU)
    xy, inf = ck.srs.export()
    blobs = ck.srs.export_compressed()
    ck.srs.close()
    dev = f"cuda:{ctx.device}"
    d_bytes = torch.from_numpy(blobs.reshape(-1)).to(dev)
    d_xy = torch.zeros(n * 2 * L, dtype=torch.int64, device=dev)
    d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    want_xy = torch.from_numpy(xy.view(np.int64).reshape(-1)).to(dev)
    ctx.prof_enable(True)

    def wall(fn):
        torch.cuda.synchronize(ctx.device)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def device_form(check):
        ctx.prof_reset()
        d_st.fill_(9)
        torch.cuda.synchronize(ctx.device)
        ctx.g1_decompress_device(d_bytes.data_ptr(), n, check, d_xy.data_ptr(), d_inf.data_ptr(), d_st.data_ptr())
        ms, count = ctx.prof_read("g1_decompress")
        assert count == 1
        assert not bool(d_st.any()) and not bool(d_inf.any()) and bool(torch.equal(d_xy, want_xy))
        return ms

    def load_compressed():
        key = ctx.srs_load_g1_compressed(blobs, True)
        key.close()

    def load_affine():
        key = ctx.srs_load_g1(xy, inf)
        key.close()

    names = ["decompress_ms", "decompress_checked_ms", "decompress_host_ms", "check_affine_ms", "load_compressed_ms",
             "load_affine_ms"]
    samples = {k: [] for k in names}
    for rep in range(a.reps + 1):
        row = {}
        row["decompress_ms"] = device_form(False)
        row["decompress_checked_ms"] = device_form(True)
        row["decompress_host_ms"], (hxy, hinf, hst) = wall(lambda: ctx.g1_decompress(blobs, True))
        assert not hst.any() and not hinf.any() and np.array_equal(hxy, xy)
        row["check_affine_ms"], st = wall(lambda: ctx.g1_check_subgroup(xy, inf))
        assert not st.any()
        row["load_compressed_ms"], _ = wall(load_compressed)
        row["load_affine_ms"], _ = wall(load_affine)
        if rep:
            for k in names:
                samples[k].append(row[k])
    key = ctx.srs_load_g1_compressed(blobs, True)            # the reloaded key is the key
    bxy, binf = key.export()
    assert np.array_equal(bxy, xy) and np.array_equal(binf, inf)
    key.close()
    ctx.prof_enable(False)
    res = {"curve": "bls12_381", "n": n, "reps": a.reps,
           **{k: {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": [round(s, 3) for s in v]}
              for k, v in samples.items()}}
    res["subgroup_kernel_ms"] = res["decompress_checked_ms"]["median"] - res["decompress_ms"]["median"]
    res["load_compressed_over_load_affine"] = res["load_compressed_ms"]["median"] / res["load_affine_ms"]["median"]
    for k in names:
        print(f"{k}: {res[k]['median']:.2f} ms (min {res[k]['min']:.2f}, max {res[k]['max']:.2f})", file=sys.stderr)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "g1_bytes_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

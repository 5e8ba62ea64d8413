"""Timing of G2 linear combinations and of check_key's folded G2 chain on one GPU.  Per curve, in one
process, after a warm-up, every figure device-synchronised:

    the sum of n = 65, 2^12, 2^16 products (points [tau^j] G2 as arrays, random 256-bit scalars)
        span_ms              the "g2_lincomb" span of kzg_g2_lincomb: copies in, the launches, the fold, the result out
        lincomb_ms           wall time of Context.g2_lincomb, arrays in, one point out
        mul_each_ms          wall time of Context.g2_mul_each on the same arrays: the device part of the route this
                             replaces (multiply_each_g2 followed by a host loop of additions)
        host_adds_extrapolated_ms   the host part of that route: curve.Group.add of two affine points, timed on 16
                             additions and scaled to n - 1 -- extrapolated, not run
    check_key at m = 65 and 4,096 G2 powers (a 16-point G1 key, so the G2 chain is what is timed)
        fold_ms              wall time of check_key(g2_chain="fold")
        links_ms             wall time of check_key(g2_chain="links"), the route this replaces

    python tools/g2_lincomb_bench.py [--out DIR] [--reps 5] [--curves bls12_381,bn254] [--sizes 65,4096,65536]
                                     [--chains 65,4096]

Every figure is given as the median with the minimum and maximum over --reps repetitions.  Prints one JSON line (and
writes DIR/g2_lincomb_bench.json with --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x2b7e_1516_28ae_d2a6_abf7_1588_09cf
HOST_ADDS = 16


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": [round(s, 3) for s in v]}


def wall(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_ms_per_add(group, gen, order):
    import random
    rng = random.Random(16)
    pts = [group.normalize(group.multiply(gen, rng.randrange(1, order))) for _ in range(HOST_ADDS + 1)]
    t0 = time.perf_counter()
    acc = pts[0]
    for pt in pts[1:]:
        acc = group.add(acc, pt)
    return (time.perf_counter() - t0) * 1e3 / HOST_ADDS


def report(curve, what, res, keys):
    for k in keys:
        print(f"{curve} {what} {k}: {res[k]['median']:.3f} ms [{res[k]['min']:.3f}, {res[k]['max']:.3f}]", file=sys.stderr)


def bench_curve(curve, reps, sizes, chains):
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG(curve)
    ctx = kzg._context()
    order = kzg.curve_order
    G = kzg._g2
    add_ms = host_ms_per_add(G, kzg.G2, order)
    out = {"host_g2_ms_per_add": add_ms}
    top = max(sizes + chains)
    xy1, inf1 = kzg._g2_arrays([kzg.G2], "bench")
    p_xy, p_inf = ctx.g2_mul_powers(np.repeat(xy1, top, axis=0), np.repeat(inf1, top), TAU, 1)
    ctx.prof_enable(True)
    for n in sizes:
        xy, inf = p_xy[:n], p_inf[:n]
        k = np.frombuffer(np.random.default_rng(n).bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
        e, t = 0, 1
        for v in _native.limbs_to_ints(k):
            e = (e + int(v) * t) % order
            t = t * TAU % order
        want = G.normalize(G.multiply(kzg.G2, e))
        samples = {"span_ms": [], "lincomb_ms": [], "mul_each_ms": []}
        for rep in range(reps + 1):
            ctx.prof_reset()
            ms, got = wall(ctx, lambda: ctx.g2_lincomb(xy, inf, k))
            span, count = ctx.prof_read("g2_lincomb")
            assert count == 1
            if rep == 0:
                assert _native.limbs_to_g2_points(got[0].reshape(1, -1), got[1])[0] == want
            each_ms, _ = wall(ctx, lambda: ctx.g2_mul_each(xy, inf, k))
            if rep:
                for key, v in (("span_ms", span), ("lincomb_ms", ms), ("mul_each_ms", each_ms)):
                    samples[key].append(v)
        res = {key: summary(v) for key, v in samples.items()}
        res["host_adds_extrapolated_ms"] = add_ms * (n - 1)
        out[f"sum n={n}"] = res
        report(curve, f"n={n}", res, samples)
    ctx.prof_enable(False)

    ck = kzg.setup(15, TAU)[0]
    for m in chains:
        g2 = _native.limbs_to_g2_points(p_xy[:m], p_inf[:m])
        samples = {"fold_ms": [], "links_ms": []}
        for rep in range(reps + 1):
            for key, chain in (("fold_ms", "fold"), ("links_ms", "links")):
                ms, verdict = wall(ctx, lambda: kzg.check_key(ck, g2, r=rep + 3, g2_chain=chain))
                assert verdict is True
                if rep:
                    samples[key].append(ms)
        res = {key: summary(v) for key, v in samples.items()}
        out[f"check_key m={m}"] = res
        report(curve, f"check_key m={m}", res, samples)
    ck.srs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--sizes", default="65,4096,65536")
    ap.add_argument("--chains", default="65,4096")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    chains = [int(s) for s in a.chains.split(",") if s]
    res = {"reps": a.reps, **{c: bench_curve(c, a.reps, sizes, chains) for c in a.curves.split(",")}}
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "g2_lincomb_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

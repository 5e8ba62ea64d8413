"""Timing of the per-point scalar multiplication and of setup contributions on one GPU.  Per curve, in
one process, after a warm-up, every figure device-synchronised:

    scale_key n = 2^12, 2^16, 2^20
        ladder_ms            the "g1_mul_each" span of KZG.scale_key: the launches of g1_mul_each_kernel alone
        scale_key_ms         wall time of KZG.scale_key, key handle to key handle: the ladder plus the expansion of the
                             new key's window multiples (what every key constructor ends with)
        srs_generate_ms      wall time of kzg_srs_generate at the same n: a fixed-base comb doing different work (it
                             knows tau), a FLOOR for a key of n points with its windows, not a target
        host_extrapolated_ms curve.Group.multiply, the host route this replaces, timed on 16 points and scaled to n
    multiply_each_g2 at 65 points
        g2_span_ms           the "g2_mul_each" span (copies in and out included); g2_ms the wall time of the facade call;
                             g2_host_extrapolated_ms as above
    contribute at 4,096 G1 + 65 G2
        contribute_ms        wall time of KZG.contribute end to end (scale_key, the G2 powers, the Lagrange key)

    python tools/mul_each_bench.py [--out DIR] [--reps 5] [--curves bls12_381,bn254] [--sizes 12,16,20]

Every figure is given as the median with the minimum and maximum over --reps repetitions.  Prints one JSON line (and
writes DIR/mul_each_bench.json with --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x2b7e_1516_28ae_d2a6_abf7_1588_09cf
S = 0x243f_6a88_85a3_08d3_1319_8a2e_0370_7344_a409_3822_299f
HOST_POINTS = 16


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": [round(s, 3) for s in v]}


def wall(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_ms_per_point(group, gen, order):
    import random
    rng = random.Random(16)
    pts = [group.multiply(gen, rng.randrange(1, order)) for _ in range(HOST_POINTS)]
    ks = [rng.randrange(order) for _ in range(HOST_POINTS)]
    t0 = time.perf_counter()
    for pt, k in zip(pts, ks):
        group.multiply(pt, k)
    return (time.perf_counter() - t0) * 1e3 / HOST_POINTS


def bench_curve(curve, reps, sizes):
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG(curve)
    ctx = kzg._context()
    order = kzg.curve_order
    host1 = host_ms_per_point(kzg._g1, kzg.G1, order)
    host2 = host_ms_per_point(kzg._g2, kzg.G2, order)
    out = {"host_g1_ms_per_point": host1, "host_g2_ms_per_point": host2}
    ctx.prof_enable(True)
    for log_n in sizes:
        n = 1 << log_n
        ck = kzg.setup(n - 1, TAU)[0]
        want = kzg.setup(n - 1, TAU * S % order)[0]
        samples = {"ladder_ms": [], "scale_key_ms": [], "srs_generate_ms": []}
        for rep in range(reps + 1):
            ctx.prof_reset()
            ms, key = wall(ctx, lambda: kzg.scale_key(ck, S))
            span, count = ctx.prof_read("g1_mul_each")
            assert count == 1
            if rep == 0:
                assert key.srs.export_compressed(n - 64, 64).tobytes() == want.srs.export_compressed(n - 64, 64).tobytes()
            key.srs.close()
            gen_ms, gen = wall(ctx, lambda: ctx.srs_generate(_native.int_to_words(TAU), n))
            gen.close()
            if rep:
                for k, v in (("ladder_ms", span), ("scale_key_ms", ms), ("srs_generate_ms", gen_ms)):
                    samples[k].append(v)
        res = {k: summary(v) for k, v in samples.items()}
        res["host_extrapolated_ms"] = host1 * n
        out[f"scale_key n=2^{log_n}"] = res
        for k in samples:
            print(f"{curve} n=2^{log_n} {k}: {res[k]['median']:.3f} ms [{res[k]['min']:.3f}, {res[k]['max']:.3f}]",
                  file=sys.stderr)
        ck.srs.close()
        want.srs.close()

    n1, n2 = 4096, 65
    setup = kzg.unit_setup(n1, n2)
    setup, _ = kzg.contribute(setup, TAU)
    powers = [pow(S, j, order) for j in range(n2)]
    want_g2 = kzg.setup_g2(n2, TAU * S % order, device=True)
    samples = {"g2_span_ms": [], "g2_ms": [], "contribute_ms": []}
    for rep in range(reps + 1):
        ctx.prof_reset()
        ms, got = wall(ctx, lambda: kzg.multiply_each_g2(setup.g2, powers))
        span, count = ctx.prof_read("g2_mul_each")
        assert count == 1 and got == want_g2
        c_ms, (new, contribution) = wall(ctx, lambda: kzg.contribute(setup, S))
        assert new.g2 == want_g2 and contribution.tau_g1 == new.monomial[1]
        new.monomial.srs.close()
        new.lagrange.srs.close()
        if rep:
            for k, v in (("g2_span_ms", span), ("g2_ms", ms), ("contribute_ms", c_ms)):
                samples[k].append(v)
    ctx.prof_enable(False)
    res = {k: summary(v) for k, v in samples.items()}
    res["g2_host_extrapolated_ms"] = host2 * n2
    res["contribute_host_extrapolated_ms"] = host1 * n1 + host2 * n2
    out[f"setup n1={n1} n2={n2}"] = res
    for k in samples:
        print(f"{curve} {k}: {res[k]['median']:.3f} ms [{res[k]['min']:.3f}, {res[k]['max']:.3f}]", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--sizes", default="12,16,20")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    res = {"reps": a.reps, **{c: bench_curve(c, a.reps, sizes) for c in a.curves.split(",")}}
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "mul_each_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Timing of coset openings on one GPU: coset table builds, kzg_open_cosets against kzg_open_domain
(same process, alternating), the PeerDAS shape, and kzg_open_coset_device against kzg_open_device (k = 1, alternating).

    python tools/open_cosets_bench.py --out DIR [--curve bls12_381] [--reps 5] [--table-logs 12,16,20] [--ls 16,64]
                                      [--log-n 20] [--skip-domain]

Every figure is the median of --reps runs after one warm-up; each repetition spot-checks one proof: a coset proof
against kzg_open_coset, an open_domain proof against kzg_open.  Writes DIR/open_cosets_bench.json and prints it."""
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
    ap.add_argument("--ls", default="16,64")
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--skip-domain", action="store_true", help="leave out open_domain (its table alone takes ~1 s)")
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG(a.curve)
    ctx = kzg._context()
    r = kzg.curve_order
    rng = random.Random(1)
    ls = [int(x) for x in a.ls.split(",") if x]
    res = {"curve": a.curve, "reps": a.reps, "table_ms": {}, "open_cosets_ms": {}, "open_domain_ms": None,
           "peerdas_ms": {}, "open_coset_device_ms": {}, "open_device_ms": None}
    one = _native.int_to_words(1)

    def timed(fn):
        torch.cuda.synchronize(ctx.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(ctx.device)
        return (time.perf_counter() - t0) * 1e3, out

    def med(samples):
        return {"median": statistics.median(samples), "samples": samples}

    def check_coset(ck, arr, n, xy, inf, i, log_N, w, l, b=0):
        C = (1 << log_N) // l
        zeta = pow(w, C, r)
        pxy, pinf, _ = ctx.open_coset(ck.srs, arr[b:b + 1], [n], n, l.bit_length() - 1, pow(w, i, r), zeta, 1)
        assert np.array_equal(xy[b, i], pxy) and inf[b, i] == pinf[0], (n, l, log_N, i)

    # ---- table builds
    keys = {}
    for lg in sorted({int(x) for x in a.table_logs.split(",") if x} | {a.log_n, 12}):
        n = 1 << lg
        keys[lg] = kzg.setup(n - 1, tau=rng.randrange(r))[0]
        if str(lg) not in a.table_logs.split(","):
            continue
        for l in ls:
            if l > n // 2:
                continue
            samples = []
            for rep in range(a.reps + 1):
                ms, t = timed(lambda: ctx.coset_table(keys[lg].srs, lg, l.bit_length() - 1))
                t.close()
                if rep:
                    samples.append(ms)
            res["table_ms"][f"{lg}:{l}"] = med(samples)
            print(f"coset table 2^{lg} l={l}: {statistics.median(samples):.1f} ms", flush=True)

    # ---- open_cosets at 2^log_n, b = 1, alternating with open_domain
    lg = a.log_n
    n = 1 << lg
    ck = keys[lg]
    arr = _native.ints_to_limbs([rng.randrange(r) for _ in range(n)]).reshape(1, n, 4).copy()
    tables = {l: ctx.coset_table(ck.srs, lg, l.bit_length() - 1) for l in ls}
    dtable = None if a.skip_domain else ctx.domain_table(ck.srs, lg)
    w_n = int(kzg.Fq.root_of_unity(n))
    cos = {(l, f): [] for l in ls for f in (1, 2)}
    dom = []
    for rep in range(a.reps + 1):
        for (l, f), samples in cos.items():
            log_N = lg + (f - 1)
            w = int(kzg.Fq.root_of_unity(n * f))
            ms, (xy, inf, _) = timed(lambda: ctx.open_cosets(tables[l], arr, [n], n, log_N, w, evals=False))
            check_coset(ck, arr, n, xy, inf, rng.randrange(n * f // l), log_N, w, l)
            if rep:
                samples.append(ms)
        if dtable is not None:
            ms, (xy, inf, _) = timed(lambda: ctx.open_domain(dtable, arr, [n], n, w_n, evals=False))
            i = rng.randrange(n)
            pxy, pinf, _ = ctx.open(ck.srs, arr, [n], n, _native.int_to_words(pow(w_n, i, r)), one)
            assert np.array_equal(xy[0, i], pxy) and inf[0, i] == pinf[0], i
            if rep:
                dom.append(ms)
    for (l, f), samples in cos.items():
        res["open_cosets_ms"][f"{lg}:l{l}:N{f}n"] = med(samples)
        print(f"open_cosets 2^{lg} l={l} N={f}n: {statistics.median(samples):.1f} ms", flush=True)
    if dom:
        res["open_domain_ms"] = med(dom)
        print(f"open_domain 2^{lg}: {statistics.median(dom):.1f} ms", flush=True)
        res["open_domain_over_open_cosets_l16_Nn"] = statistics.median(dom) / statistics.median(cos[(16, 1)]) \
            if (16, 1) in cos else None
        dtable.close()
    for t in tables.values():
        t.close()

    # ---- PeerDAS shape: n = 2^12, N = 2^13, l = 64
    pn, pl = 1 << 12, 64
    ptable = ctx.coset_table(keys[12].srs, 12, 6)
    w = int(kzg.Fq.root_of_unity(2 * pn))
    for b in (1, 32):
        parr = _native.ints_to_limbs([rng.randrange(r) for _ in range(b * pn)]).reshape(b, pn, 4).copy()
        samples = []
        for rep in range(a.reps + 1):
            ms, (xy, inf, _) = timed(lambda: ctx.open_cosets(ptable, parr, [pn] * b, pn, 13, w, evals=True))
            jb = rng.randrange(b)
            check_coset(keys[12], parr, pn, xy, inf, rng.randrange(2 * pn // pl), 13, w, pl, b=jb)
            if rep:
                samples.append(ms)
        res["peerdas_ms"][f"b{b}"] = dict(med(samples), per_blob=statistics.median(samples) / b)
        print(f"PeerDAS shape b={b}: {statistics.median(samples):.1f} ms", flush=True)
    ptable.close()

    # ---- kzg_open_coset_device vs kzg_open_device (k = 1) at 2^log_n, alternating
    d = torch.from_numpy(arr.reshape(n, 4).view(np.int64)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize(ctx.device)
    cs = {l: [] for l in ls}
    od = []
    z = rng.randrange(1, r)
    for rep in range(a.reps + 1):
        for l in ls:
            zeta = int(kzg.Fq.root_of_unity(l))
            ms, (xy, inf, _) = timed(lambda: ctx.open_coset(ck.srs, d.data_ptr(), [n], n, l.bit_length() - 1, z, zeta,
                                                            1, device=True))
            if rep == 0:
                hxy, hinf, _ = ctx.open_coset(ck.srs, arr, [n], n, l.bit_length() - 1, z, zeta, 1)
                assert np.array_equal(xy, hxy) and inf[0] == hinf[0], l
            if rep:
                cs[l].append(ms)
        ms, _ = timed(lambda: ctx.open(ck.srs, d.data_ptr(), [n], n, _native.int_to_words(z), one, device=True))
        if rep:
            od.append(ms)
    res["open_device_ms"] = med(od)
    for l in ls:
        res["open_coset_device_ms"][str(l)] = dict(med(cs[l]),
                                                   ratio_to_open=statistics.median(cs[l]) / statistics.median(od))
        print(f"open_coset_device 2^{lg} l={l}: {statistics.median(cs[l]):.2f} ms "
              f"(open_device {statistics.median(od):.2f} ms)", flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "open_cosets_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items()}, default=str)[:4000])


if __name__ == "__main__":
    main()

"""Timing of coset recovery on one GPU: kzg_recover_cosets_device at the PeerDAS shape (b = 1, 32) and
at 2^16 / 2^20, against two references timed alternately in the same process -- three batched kzg_ntt_device transforms
of size N (the floor of the per-polynomial part) and kzg_open_cosets_device for the same shape.

    python tools/recover_bench.py --out DIR [--curve bls12_381] [--reps 5] [--shapes peerdas_b1,peerdas_b32,...]
                                  [--no-open NAMES]

Every figure is the median of --reps runs after one warm-up; every repetition (the warm-up too) is verified against
the polynomial it started from, bit for bit.  Writes DIR/recover_bench.json and prints it."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (log_n, log_N, log_l, b); half of the cosets are missing, chosen at random
SHAPES = {
    "peerdas_b1": (12, 13, 6, 1),
    "peerdas_b32": (12, 13, 6, 32),
    "2p16_l64": (16, 17, 6, 1),
    "2p20_l16": (20, 21, 4, 1),
    "2p20_l1": (20, 21, 0, 1),            # 2^20 missing cosets: the product tree at its largest
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--curve", default="bls12_381")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--no-open", default="", help="shapes whose open_cosets reference is left out (key and table "
                                                  "of 2^20 points take seconds to build)")
    a = ap.parse_args()

    import numpy as np
    import torch
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import KZG

    kzg = KZG(a.curve)
    ctx = kzg._context()
    r = kzg.curve_order
    dev = f"cuda:{ctx.device}"
    rng = random.Random(1)
    no_open = {s for s in a.no_open.split(",") if s}
    res = {"curve": a.curve, "reps": a.reps, "leaf": int(ctx.prof_read("recover_leaf")[0]), "shapes": {}}

    def timed(fn):
        torch.cuda.synchronize(ctx.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(ctx.device)
        return (time.perf_counter() - t0) * 1e3, out

    keys = {}
    for name in [s for s in a.shapes.split(",") if s]:
        log_n, log_N, log_l, b = SHAPES[name]
        n, N, l = 1 << log_n, 1 << log_N, 1 << log_l
        C = N // l
        w = int(kzg.Fq.root_of_unity(N))
        w_words = _native.int_to_words(w)
        gen = torch.Generator(device=dev).manual_seed(log_n * 100 + b)
        want = torch.randint(0, 1 << 62, (b, n, 4), dtype=torch.int64, device=dev, generator=gen)
        want[:, :, 3] >>= 3                                               # below 2^251 < r
        ev = torch.zeros((b, N, 4), dtype=torch.int64, device=dev)
        ev[:, :n] = want
        torch.cuda.synchronize(ctx.device)
        ctx.ntt_device(ev.data_ptr(), log_N, w_words, 0, batch=b)
        ctx.synchronize()
        scratch = torch.zeros((b, N, 4), dtype=torch.int64, device=dev)
        d_out = torch.zeros((b, n, 4), dtype=torch.int64, device=dev)
        table = None
        if name not in no_open and log_l < log_n:
            if log_n not in keys:
                keys[log_n] = kzg.setup(n - 1, tau=rng.randrange(r))[0]
            table = ctx.coset_table(keys[log_n].srs, log_n, log_l)
        rec, floor, opn = [], [], []
        for rep in range(a.reps + 1):
            idx = rng.sample(range(C), C // 2)
            rng.shuffle(idx)
            idx_t = torch.tensor(idx, dtype=torch.int64, device=dev)
            d_vals = ev.view(b, l, C, 4)[:, :, idx_t, :].permute(0, 2, 1, 3).contiguous()      # [b][K][l][4]
            d_out.zero_()
            idx_a = np.asarray(idx, dtype=np.uint32)
            ms, (_, ok) = timed(lambda: ctx.recover_cosets(log_n, log_N, log_l, w, idx_a, d_vals.data_ptr(), b,
                                                           d_coeffs=d_out.data_ptr()))
            assert ok.tolist() == [1] * b and torch.equal(d_out, want), (name, rep)
            if rep:
                rec.append(ms)

            def three():
                for inverse in (1, 0, 1):
                    ctx.ntt_device(scratch.data_ptr(), log_N, w_words, inverse, batch=b)
                ctx.synchronize()
            ms, _ = timed(three)
            if rep:
                floor.append(ms)
            if table is not None:
                ms, _ = timed(lambda: ctx.open_cosets(table, d_out.data_ptr(), [n] * b, n, log_N, w, device=True,
                                                      evals=True))
                if rep:
                    opn.append(ms)
        if table is not None:
            table.close()
        m_rec, m_floor = statistics.median(rec), statistics.median(floor)
        row = {"log_n": log_n, "log_N": log_N, "l": l, "b": b, "missing": C - C // 2,
               "recover_ms": {"median": m_rec, "samples": rec},
               "three_ntt_ms": {"median": m_floor, "samples": floor},
               "ratio_to_three_ntt": m_rec / m_floor,
               "open_cosets_ms": {"median": statistics.median(opn), "samples": opn} if opn else None}
        res["shapes"][name] = row
        print(f"{name}: recover {m_rec:.3f} ms, three transforms {m_floor:.3f} ms (x{m_rec / m_floor:.2f}), open_cosets "
              f"{statistics.median(opn) if opn else float('nan'):.1f} ms", flush=True)
        del ev, scratch, d_out, want
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "recover_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""When the waves of msm_accumulate_kernel leave: the kernel ends with its LAST wave, and a SIMD whose other wave has
left runs at half rate, so (last exit - mean exit) is time the kernel's share of the GPU stands partly idle.

    python tools/acc_tail.py [--log-n 20] [--batch 4] [--steps 10]

Two measurements with the library's own probe (kzg_prof_read "msm_accumulate_tail_us", "msm_accumulate_exit_spread_us"; the span of the
kernel beside them):
  alone      one commit in flight (flush after each)
  pipelined  bench.py's loop: an inverse transform of `batch` polynomials and their commits per step, one flush
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x2718281828459045235360287471


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from kzg_snark_amd import _native
    from oracle import py_oracle as O
    cv = O.curve("bls12_381")
    dev = "cuda:0"
    ctx = _native.Context("bls12_381")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.bind_torch_stream(stream)
    n, B, L = 1 << args.log_n, args.batch, ctx.fp_limbs
    srs = ctx.srs_generate(_native.int_to_words(TAU % cv.r), n)
    w_words = _native.int_to_words(cv.root_of_unity(n))
    rs = np.random.RandomState(7)
    host = rs.randint(0, 1 << 62, size=(B, n, 4), dtype=np.int64)
    host[..., 3] >>= 3
    works = [torch.from_numpy(host).to(dev), torch.from_numpy(host).to(dev)]
    torch.cuda.synchronize()
    keep = []

    def step(i):
        work = works[i & 1]
        ctx.ntt_device(work.data_ptr(), args.log_n, w_words, True, B)
        xy, inf = np.zeros((B, 2 * L), dtype=np.uint64), np.zeros(B, dtype=np.uint8)
        keep.append((xy, inf))
        ctx.commit_device_async(srs, work.data_ptr(), [n] * B, n, xy, inf)

    def report(mode):
        span_ms, launches = ctx.prof_read("msm_accumulate")
        tail_us, cnt = ctx.prof_read("msm_accumulate_tail_us")
        spread_us, _ = ctx.prof_read("msm_accumulate_exit_spread_us")
        span_us = 1e3 * span_ms / max(launches, 1)
        print(json.dumps({"mode": mode, "launches": int(cnt), "accumulate_span_us": round(span_us, 1),
                          "tail_us_last_minus_mean": round(tail_us, 1), "exit_spread_us_last_minus_first": round(spread_us, 1),
                          "tail_share_of_span": round(tail_us / span_us, 4) if span_us else None,
                          "shader_mhz": round(ctx.prof_read("msm_accumulate_shader_mhz")[0], 1)}), flush=True)

    for i in range(2):                                      # warm-up: slots, code objects, clocks
        step(i)
    ctx.commit_flush()
    ctx.prof_enable(True)
    ctx.prof_reset()
    for p in range(args.steps):
        xy, inf = np.zeros((1, 2 * L), dtype=np.uint64), np.zeros(1, dtype=np.uint8)
        ctx.commit_device_async(srs, works[0].data_ptr() + (p % B) * n * 32, [n], n, xy, inf)
        ctx.commit_flush()
    report("alone")
    ctx.prof_reset()
    for i in range(args.steps):
        step(i)
    ctx.commit_flush()
    report("pipelined")
    ctx.prof_enable(False)


if __name__ == "__main__":
    main()

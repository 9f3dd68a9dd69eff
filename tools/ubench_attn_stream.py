"""Key-streamed SR-attention microbench (csrc/attention_stream.hip: attn_fwd_stream_kernel / attn_bwd_stream_kernel).

1. The four stage shapes of pvlt_tiny at 512 px, T = 128, batch 32 (every stage sees M = 384 keys): the streamed forward and backward
   through the public entry points, with the fraction of MFMA peak (bf16 2.5 PF dense, fp32 157 TF).
2. Streamed against LDS-resident kernels at M = 192 / 272 / 320 on the same box and the same random data (stage-2 and stage-4 shapes
   of pvlt_tiny at batch 32): the streamed exports against the public entry points, which take the resident kernels at these M.

Usage: python tools/ubench_attn_stream.py [--dtype bf16|fp32] [--reps 20]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvlt_amd import ops  # noqa: E402

PEAK_TF = {torch.bfloat16: 2500.0, torch.float32: 157.3}


def timeit(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def case(B, H, N, M, dt, streamed, reps):
    dev = torch.device("cuda:0")
    C = 64 * H
    g = torch.Generator(device="cpu").manual_seed(B + H + N + M)
    q = torch.randn(B, N, C, generator=g).to(dev, dt)
    kv = torch.randn(B, M, 2 * C, generator=g).to(dev, dt)
    do = torch.randn(B, N, C, generator=g).to(dev, dt)
    o, lse, dq = torch.empty_like(q), torch.empty(B, H, N, device=dev), torch.empty_like(q)
    dkv = torch.zeros(B, M, 2 * C, device=dev)
    f = ops.sr_attention_fwd_streamed if streamed else ops.sr_attention_fwd
    b = ops.sr_attention_bwd_streamed if streamed else ops.sr_attention_bwd
    tf = timeit(lambda: f(q, kv, o, lse, B, H, N, M, C, 2 * C, C, 0, C, 0.125), reps)
    # the zero fill of the fp32 dKV is part of what an atomics-reducing backward costs its caller (trunk.py's pool_zeros)
    tb = timeit(lambda: (dkv.zero_(), b(q, kv, o, do, lse, dq, dkv, B, H, N, M, C, 2 * C, C, 2 * C, 0, C, 0.125)), reps)
    return tf, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    B = 32
    print(f"## streamed kernels, pvlt_tiny at 512 px / T = 128, batch {B}, {a.dtype}")
    print("| stage | H | N | M | fwd us | fwd % MFMA peak | bwd us | bwd % MFMA peak |")
    print("|---|---|---|---|---|---|---|---|")
    for st, (H, N) in enumerate(((1, 16512), (2, 4224), (5, 1152), (8, 384)), 1):
        M = 384
        tf, tb = case(B, H, N, M, dt, False, a.reps)
        fl = 4.0 * B * H * N * M * 64
        pf, pb = fl / tf / 1e6 / PEAK_TF[dt] * 100, 2.5 * fl / tb / 1e6 / PEAK_TF[dt] * 100
        print(f"| {st} | {H} | {N} | {M} | {tf:.1f} | {pf:.1f} | {tb:.1f} | {pb:.1f} |")
    print(f"\n## streamed / resident, batch {B}, {a.dtype}")
    print("| H | N | M | fwd resident us | fwd streamed us | ratio | bwd resident us | bwd streamed us | ratio |")
    print("|---|---|---|---|---|---|---|---|---|")
    for M in (192, 272, 320):
        if dt == torch.float32 and M > 288:
            continue                                   # no fp32 resident kernel at 320 keys
        for H, N in ((2, 4224), (8, M)):
            rf, rb = case(B, H, N, M, dt, False, a.reps)
            sf, sb = case(B, H, N, M, dt, True, a.reps)
            print(f"| {H} | {N} | {M} | {rf:.1f} | {sf:.1f} | {sf / rf:.2f} | {rb:.1f} | {sb:.1f} | {sb / rb:.2f} |")


if __name__ == "__main__":
    main()

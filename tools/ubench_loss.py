"""Times the plain cross-entropy kernels (elementwise.hip) and the label-smoothed / class-weighted ones (loss.hip, docs/loss_options.md) in one process, on
the shapes of the benchmark step: the MLM rows (about 1490 x 30522 logits, ld 30528, bf16 dlogits) and the two CLS heads (256 x 48, 256 x 122, fp32 dlogits).

    python tools/ubench_loss.py [--rows 1490] [--iters 200] [--out FILE]

Every variant is timed with device events around `iters` back-to-back launches, the variants interleaved round by round (five rounds, the median is
reported with the spread), after a warm-up of every variant.  The MLM logits rotate through three buffers (546 MB, more than the 256 MB Infinity Cache), so the
forward reads HBM as it does behind the decoder GEMM of a real step.  Bytes: forward rows x V x 4 read; backward the same read plus rows x ldd x 2 or 4
written (the weights, V x 4 per row, come from L2 and are not counted).  Needs the GPU: there is no CPU path to time."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvlt_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")


def variants(rows, V, ld, out_dtype, nbuf):
    g = torch.Generator().manual_seed(0)
    xs = [(3 * torch.randn(rows, ld, generator=g)).to(DEV) for _ in range(nbuf)]
    labels = torch.randint(0, V, (rows,), generator=g).to(DEV)
    w = (0.5 + 1.5 * torch.rand(V, generator=g)).to(DEV)
    lse, smooth = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    acc2, acc3, gs = torch.zeros(2, device=DEV), torch.empty(3, device=DEV), torch.ones(1, device=DEV)
    dl = torch.empty(rows, ld, device=DEV, dtype=out_dtype)
    state = dict(i=0)

    def x():
        state["i"] = (state["i"] + 1) % nbuf
        return xs[state["i"]]

    def smooth_fwd(e, wt):
        return lambda: ops.ce_smooth_fwd(x(), labels, lse, smooth, acc3, rows, V, ld, label_smoothing=e, weight=wt)

    def smooth_bwd(e, wt):
        return lambda: ops.ce_smooth_bwd(x(), labels, lse, gs, acc3, dl, rows, V, ld, ld, label_smoothing=e, weight=wt)

    fwd = {"plain": lambda: ops.cross_entropy_fwd(x(), labels, lse, acc2[0:1], acc2[1:2], rows, V, ld), "smooth e=0.1": smooth_fwd(0.1, None),
           "weights e=0": smooth_fwd(0.0, w), "smooth e=0.1 + weights": smooth_fwd(0.1, w)}
    ops.ce_smooth_fwd(xs[0], labels, lse, smooth, acc3, rows, V, ld, label_smoothing=0.1, weight=w)        # a valid lse / acc for the backward variants
    ops.cross_entropy_fwd(xs[0], labels, lse, acc2[0:1], acc2[1:2], rows, V, ld)
    bwd = {"plain": lambda: ops.cross_entropy_bwd(x(), labels, lse, gs, acc2[1:2], dl, rows, V, ld, ld), "smooth e=0.1": smooth_bwd(0.1, None),
           "weights e=0": smooth_bwd(0.0, w), "smooth e=0.1 + weights": smooth_bwd(0.1, w)}
    return fwd, bwd


def time_all(fns, iters, rounds=5):
    for f in fns.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1490)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ubench_loss.py needs the GPU"
    lines = [f"ubench_loss: device events around {a.iters} launches, median (min .. max) of 5 interleaved rounds, us per call; forward = row kernel + finish kernel"]
    for name, rows, V, ld, odt, nbuf in (("MLM", a.rows, 30522, 30528, torch.bfloat16, 3), ("CLS sup", 256, 48, 48, torch.float32, 1),
                                         ("CLS sub", 256, 122, 122, torch.float32, 1)):
        fwd, bwd = variants(rows, V, ld, odt, nbuf)
        for tag, fns, nbytes in (("forward", fwd, rows * V * 4), ("backward", bwd, rows * V * 4 + rows * ld * (2 if odt == torch.bfloat16 else 4))):
            res = time_all(fns, a.iters if name == "MLM" else 4 * a.iters)
            base = res["plain"][0]
            lines.append(f"{name} {rows} x {V} (ld {ld}) {tag}, {nbytes / 1e6:.1f} MB:")
            for k, (med, lo, hi) in res.items():
                lines.append(f"    {k:24s} {med:8.2f} us ({lo:.2f} .. {hi:.2f})   {nbytes / med / 1e6:7.2f} TB/s   {med / base:5.2f} x plain")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

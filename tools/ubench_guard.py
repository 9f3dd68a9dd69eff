"""What the non-finite-gradient guard costs per optimizer step (docs/nonfinite_guard.md): flat buffers of PVT-tiny's size (40.0 M floats: P, G, m, v
fp32, the bf16 copy, the one-byte mask), one process, the launches timed with device events --
    ungated    mvlt_adamw_step alone                                          the step without the guard
    ungated'   the same arm a second time                                     its own run-to-run spread, read from two identical arms
    gated      mvlt_adamw_step_gated alone, ok = 1                            the kernel against the kernel
    guard-ok   mvlt_grad_sumsq + mvlt_step_gate + mvlt_adamw_step_gated, ok = 1   what a guarded step runs
    guard-skip the same three launches on a G that holds one Inf, ok = 0      what a skipped step runs
The arms ALTERNATE (one launch group of each per round, every round a new order of the same sequence), each group between two events; reported per
arm: mean, standard deviation, min, median, max in microseconds over --launches rounds after --warmup untimed ones.

    python tools/ubench_guard.py [--n 40000000] [--launches 60] [--warmup 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvlt_amd import ops                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40_000_000)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ubench_guard needs an MI355X"
    assert a.n % 4 == 0 and a.launches >= 50
    dev = torch.device("cuda", 0)
    n = a.n
    gen = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    g_bad = g.clone()
    g_bad[n // 2 + 1] = float("inf")
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    p16 = p.to(torch.bfloat16)
    wd = (torch.arange(n, device=dev) % 8 != 0).to(torch.uint8)                 # weight decay on most elements, none frozen: every vector steps
    norm_mask = torch.ones(n, dtype=torch.uint8, device=dev)
    hp = torch.tensor([1e-5, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9 ** 100, 1 - 0.999 ** 100, 1.0], dtype=torch.float32, device=dev)
    part = torch.empty(1024, device=dev)
    gate = torch.zeros(4, device=dev)
    open_gate = torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)

    def ungated():
        ops.adamw_step(p, g, m, v, p16, n, hp, wd)

    def gated():
        ops.adamw_step_gated(p, g, m, v, p16, n, hp, wd, open_gate)

    def guard(grad):
        ops.grad_sumsq(grad, n, norm_mask, part)
        ops.step_gate(part, 1.0, 0.0, gate, counters)
        ops.adamw_step_gated(p, grad, m, v, p16, n, hp, wd, gate)

    arms = [("ungated", ungated), ("ungated'", ungated), ("gated", gated), ("guard-ok", lambda: guard(g)), ("guard-skip", lambda: guard(g_bad))]
    times = {name: [] for name, _ in arms}
    for r in range(a.warmup + a.launches):
        order = arms[r % len(arms):] + arms[:r % len(arms)]                      # no arm always runs behind the same neighbour
        evs = []
        for name, fn in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((name, e0, e1))
        torch.cuda.synchronize()
        if r >= a.warmup:
            for name, e0, e1 in evs:
                times[name].append(1e3 * e0.elapsed_time(e1))
    applied, skipped = counters.tolist()
    assert applied == skipped == a.warmup + a.launches, (applied, skipped)      # guard-ok stepped every time, guard-skip never
    assert torch.isfinite(p).all().item()

    lines = [f"ubench_guard: {n} elements (P, G, m, v fp32 + bf16 copy + mask byte), {a.launches} alternating rounds after {a.warmup} warm-up rounds, device events, microseconds",
             f"{'arm':11s} {'mean':>9s} {'std':>8s} {'min':>9s} {'median':>9s} {'max':>9s}"]
    for name, _ in arms:
        t = times[name]
        lines.append(f"{name:11s} {statistics.mean(t):9.1f} {statistics.stdev(t):8.1f} {min(t):9.1f} {statistics.median(t):9.1f} {max(t):9.1f}")
    mean = {k: statistics.mean(t) for k, t in times.items()}
    d = {k: mean[k] - mean["ungated"] for k in mean}
    lines.append(f"against ungated (means): ungated' {d[arms[1][0]]:+.1f} us (two identical arms: the run-to-run spread of a mean);  gated {d['gated']:+.1f} us;  "
                 f"guard-ok {d['guard-ok']:+.1f} us;  guard-skip {d['guard-skip']:+.1f} us")
    lines.append(f"bytes moved by the ungated step: {(4 * 7 + 2 + 1) * n / 1e6:.0f} MB -> {(4 * 7 + 2 + 1) * n / mean['ungated'] / 1e3:.0f} GB/s;  "
                 f"the norm pass adds {(4 + 1) * n / 1e6:.0f} MB")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

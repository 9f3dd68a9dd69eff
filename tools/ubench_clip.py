"""What gradient clipping costs per training step: pvlt_tiny at the bench's batch (256 pairs, 256 x 256, 128 tokens, bf16), one process, the step timed
three ways --
    off     scaler(total, opt, clip_grad=None)                                         no clipping
    old     backward; store.apply_pending_scale(); torch.nn.utils.clip_grad_norm_(model.parameters(), c); opt.step()
            (the sequence BF16Scaler ran before the fused path existed, written out here)
    fused   scaler(total, opt, clip_grad=c)          one-pass norm over the flat buffer, coefficient inside the AdamW kernel
The arms ALTERNATE (off, old, fused, off, old, fused, ...) in rounds of STEPS steps each, every round timed with a host clock around work that ends in a
device synchronise; reported are each arm's median ms/step over the rounds, the spread of the rounds (min .. max), and the per-round differences
old - off and fused - off, so a difference can be read against the spread of repeating the same arm.  Also printed: the host time to ENQUEUE the
clip of each arm (no synchronise: what the host pays while the GPU is busy), and the stand-alone kernel times of the norm pass.

    python tools/ubench_clip.py [--rounds 7] [--steps 10] [--clip 1.0] [--batch 256] [--img 256] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                   # noqa: E402
from mvlt_amd import ops, pvlt                 # noqa: E402
from mvlt_amd.engine import BF16Scaler, train_step      # noqa: E402
from mvlt_amd.optim import FusedAdamW          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ubench_clip needs an MI355X"
    dev = torch.device("cuda", 0)
    model = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=128, loss_type=dict(mlm=1, itm=1, t2i=1, cls=0),
                           pretrained_pth=None, drop_path_rate=0.1, drop_rate=0.0, num_classes=1000, in_chans=3).cuda(dev)
    model.train()
    batch = bench.synth_batch(a.batch, a.img, 128, dev, 1)
    batch["mlm_count"] = int((batch["mlm_labels"] != -1).sum())
    opt = FusedAdamW(model, lr=1e-5, weight_decay=0.01)
    scaler = BF16Scaler()
    S = model.store
    params = list(model.parameters())
    enqueue = {"old": [], "fused": []}

    def step_off(i):
        total, _ = train_step(model, batch, i, True)
        opt.zero_grad()
        scaler(total, opt, clip_grad=None, parameters=None)

    def step_old(i):
        total, _ = train_step(model, batch, i, True)
        opt.zero_grad()
        S.scale_in_optimizer = True                    # as BF16Scaler sets it around backward + step
        try:
            total.backward()
            t0 = time.perf_counter()
            S.apply_pending_scale()
            torch.nn.utils.clip_grad_norm_(params, a.clip)
            enqueue["old"].append(time.perf_counter() - t0)
            opt.step()
        finally:
            S.scale_in_optimizer = False
            S.apply_pending_scale()

    def step_fused(i):
        total, _ = train_step(model, batch, i, True)
        opt.zero_grad()
        S.scale_in_optimizer = True
        try:
            total.backward()
            t0 = time.perf_counter()
            S.clip_grad_norm(a.clip)
            enqueue["fused"].append(time.perf_counter() - t0)
            opt.step()
        finally:
            S.scale_in_optimizer = False
            S.apply_pending_scale()

    def step_fused_scaler(i):
        total, _ = train_step(model, batch, i, True)
        opt.zero_grad()
        scaler(total, opt, clip_grad=a.clip, parameters=None)

    arms = [("off", step_off), ("old", step_old), ("fused", step_fused_scaler)]
    for _, fn in arms + [("fused-timed", step_fused)]:             # warm every arm (code objects, ATen's workspaces, the store's clip buffers)
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    norm = float(scaler.last_grad_norm) if scaler.last_grad_norm is not None else float("nan")
    times = {name: [] for name, _ in arms}
    for r in range(a.rounds):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                fn(i)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
    enqueue = {"old": [], "fused": []}
    for i in range(a.steps):                                        # host enqueue time of the clip itself (queue never drained in between)
        step_old(i)
        step_fused(i)
    torch.cuda.synchronize()
    # the norm pass alone, device events, G resident as after a step
    mask, part, out = S._clip_buffers()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for _ in range(5):
        ops.grad_sumsq(S.G, S.total, mask, part)
    k_sumsq, k_coef = [], []
    for _ in range(20):
        ev[0].record()
        ops.grad_sumsq(S.G, S.total, mask, part)
        ev[1].record()
        ops.clip_coef(part, 1.0, a.clip, out)
        ev[2].record()
        torch.cuda.synchronize()
        k_sumsq.append(1e3 * ev[0].elapsed_time(ev[1]))
        k_coef.append(1e3 * ev[1].elapsed_time(ev[2]))

    lines = [f"ubench_clip: pvlt_tiny bf16, batch {a.batch}, {a.img} x {a.img}, 128 tokens, {S.total} gradient elements; clip {a.clip} (last norm {norm:.4g}); "
             f"{a.rounds} alternating rounds x {a.steps} steps per arm, host clock around a device synchronise",
             f"{'arm':8s} {'median ms/step':>15s} {'min':>9s} {'max':>9s}   median of per-round (arm - off), ms   [min .. max]"]
    for name, _ in arms:
        t = times[name]
        d = [x - y for x, y in zip(t, times["off"])]
        lines.append(f"{name:8s} {statistics.median(t):15.3f} {min(t):9.3f} {max(t):9.3f}   {statistics.median(d):+8.3f}   [{min(d):+.3f} .. {max(d):+.3f}]")
    d = [x - y for x, y in zip(times["fused"], times["old"])]
    lines.append(f"fused - old per round: median {statistics.median(d):+.3f} ms/step   [{min(d):+.3f} .. {max(d):+.3f}]")
    lines.append(f"host time to enqueue the clip (median of {a.steps}): old {1e3 * statistics.median(enqueue['old']):.3f} ms, fused {1e3 * statistics.median(enqueue['fused']):.3f} ms")
    lines.append(f"norm pass alone (device events, median of 20): mvlt_grad_sumsq {statistics.median(k_sumsq):.1f} us "
                 f"({(4 + 1) * S.total / statistics.median(k_sumsq) / 1e3:.0f} GB/s over gradients + mask), mvlt_clip_coef {statistics.median(k_coef):.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""What the fused weight EMA costs (docs/ema.md), three measurements in one process:

  kernel   flat buffers of PVT-tiny's size (40.0 M floats), launches timed with device events, arms ALTERNATING (every round a new order):
               adamw       mvlt_adamw_step on P, G, m, v + bf16 copy + mask                  the streaming kernel this one is modelled on, same box
               ema         mvlt_ema_update with the bf16 copy and a mask (nothing frozen)    8 B read + 6 B written + 1 B of mask per element
               ema-nomask  the same without the mask                                         what FusedModelEma passes when no parameter is frozen
               ema'        the `ema` arm a second time                                       run-to-run spread of a mean, from two identical arms
  model    the pvlt_tiny pre-train model (every head of the pre-train task): FusedModelEma.update against timm's per-entry loop
           `ema_v.copy_(ema_v * decay + (1 - decay) * model_v)` over a cloned state_dict -- device time (events around the call) and host time (the
           clock around the call, which only enqueues) per call, alternating
  step     train_one_epoch_vl as bench.py times it (batch 256, 256 px, 128 tokens), blocks of steps without and with model_ema=FusedModelEma(...),
           alternating, host clock around a block that ends in a device synchronise

    python tools/ubench_ema.py [--n 40000000] [--launches 60] [--warmup 10] [--skip-model] [--skip-step] [--out FILE]
"""
import argparse
import contextlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvlt_amd import ops                       # noqa: E402


def _stats(t):
    return f"{statistics.mean(t):9.1f} {statistics.stdev(t):8.1f} {min(t):9.1f} {statistics.median(t):9.1f} {max(t):9.1f}"


def _alternate(arms, rounds, warmup):
    """{arm: ([device us], [host us])}: one call of every arm per round, each between two events and two readings of the host clock"""
    dev_t, host_t = {k: [] for k, _ in arms}, {k: [] for k, _ in arms}
    for r in range(warmup + rounds):
        order = arms[r % len(arms):] + arms[:r % len(arms)]                      # no arm always runs behind the same neighbour
        evs = []
        for name, fn in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h0 = time.perf_counter()
            fn()
            h1 = time.perf_counter()
            e1.record()
            evs.append((name, e0, e1, 1e6 * (h1 - h0)))
        torch.cuda.synchronize()
        if r >= warmup:
            for name, e0, e1, h in evs:
                dev_t[name].append(1e3 * e0.elapsed_time(e1))
                host_t[name].append(h)
    return dev_t, host_t


def kernel_part(a, dev, lines):
    n = a.n
    gen = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    p16 = p.to(torch.bfloat16)
    e = p.clone()
    e16 = p16.clone()
    wd = (torch.arange(n, device=dev) % 8 != 0).to(torch.uint8)                 # 0 / 1 bytes, none frozen: every vector is processed by both kernels
    hp = torch.tensor([1e-5, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9 ** 100, 1 - 0.999 ** 100, 1.0], dtype=torch.float32, device=dev)
    d = 0.9999
    arms = [("adamw", lambda: ops.adamw_step(p, g, m, v, p16, n, hp, wd)),
            ("ema", lambda: ops.ema_update(e, p, e16, n, d, 1.0 - d, wd)),
            ("ema-nomask", lambda: ops.ema_update(e, p, e16, n, d, 1.0 - d)),
            ("ema'", lambda: ops.ema_update(e, p, e16, n, d, 1.0 - d, wd))]
    dev_t, _ = _alternate(arms, a.launches, a.warmup)
    assert torch.isfinite(e).all().item() and torch.isfinite(p).all().item()
    per_el = {"adamw": 4 * 7 + 2 + 1, "ema": 8 + 6 + 1, "ema-nomask": 8 + 6, "ema'": 8 + 6 + 1}      # algorithmic bytes per element
    lines += [f"kernel: {n} elements, {a.launches} alternating rounds after {a.warmup} warm-up rounds, device events, microseconds",
              f"{'arm':11s} {'mean':>9s} {'std':>8s} {'min':>9s} {'median':>9s} {'max':>9s}   bytes/el  GB moved  TB/s (mean)  TB/s (median)"]
    for name, _ in arms:
        t = dev_t[name]
        gb = per_el[name] * n / 1e9
        lines.append(f"{name:11s} {_stats(t)}   {per_el[name]:8d} {gb:9.3f} {gb / statistics.mean(t) * 1e3:12.2f} {gb / statistics.median(t) * 1e3:14.2f}")
    r = (per_el["ema"] * n / statistics.median(dev_t["ema"])) / (per_el["adamw"] * n / statistics.median(dev_t["adamw"]))
    lines.append(f"ema's rate over adamw's on this box (medians): {r:.2f}")


def _pretrain_model(dev):
    from mvlt_amd import pvlt
    torch.manual_seed(1234)
    lt = dict(mlm=1, itm=1, t2i=1, cls=0)
    model = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=128, loss_type=lt, pretrained_pth=None, drop_path_rate=0.1,
                           drop_rate=0.0, num_classes=1000, in_chans=3)
    return model.cuda(dev), lt


def model_part(a, dev, lines):
    from mvlt_amd.optim import FusedModelEma
    model, _ = _pretrain_model(dev)
    model.store.ensure(dev)                                                      # (a forward would do this)
    ema = FusedModelEma(model, decay=0.9999)
    ema.update(model)
    msd = model.state_dict()
    clone = {k: v.detach().clone() for k, v in msd.items()}
    d = 0.9999

    def timm_loop():
        with torch.no_grad():
            for k, model_v in model.state_dict().items():
                ema_v = clone[k]
                ema_v.copy_(ema_v * d + (1. - d) * model_v)

    arms = [("fused", lambda: ema.update(model)), ("timm-loop", timm_loop)]
    dev_t, host_t = _alternate(arms, a.launches, a.warmup)
    lines += ["", f"model: pvlt_tiny pre-train, {model.store.total} elements in the flat store, {len(msd)} state_dict entries ({len(list(model.buffers()))} buffers), "
                  f"{a.launches} alternating rounds, microseconds per call",
              f"{'arm':11s} {'':8s} {'mean':>9s} {'std':>8s} {'min':>9s} {'median':>9s} {'max':>9s}"]
    for name, _ in arms:
        lines.append(f"{name:11s} {'device':8s} {_stats(dev_t[name])}")
        lines.append(f"{name:11s} {'host':8s} {_stats(host_t[name])}")
    lines.append("(device: events around the call -- for the loop this includes the gaps between its launches; host: the clock around the call, which only enqueues)")


def step_part(a, dev, lines):
    import argparse as _ap
    import bench
    from mvlt_amd.engine import BF16Scaler, train_one_epoch_vl
    from mvlt_amd.optim import FusedAdamW, FusedModelEma
    model, lt = _pretrain_model(dev)
    B = 256
    batch = bench.synth_batch(B, 256, 128, dev, 1234)
    opt = FusedAdamW(model, lr=2.5e-4 * B / 512.0, weight_decay=0.01)
    scaler = BF16Scaler()
    eargs = _ap.Namespace(loss_type=lt)
    ema = FusedModelEma(model, decay=0.9999)

    def block(n, model_ema):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr):
            train_one_epoch_vl(model, None, [batch] * n, opt, dev, 0, scaler, None, model_ema, None, True, False, eargs)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    block(5, None)
    block(5, ema)
    t = {"without": [], "with": []}
    for r in range(a.blocks):
        for name in (("without", "with") if r % 2 == 0 else ("with", "without")):
            t[name].append(block(a.block_steps, ema if name == "with" else None))
    lines += ["", f"step: train_one_epoch_vl, pvlt_tiny pre-train, batch {B}, 256 px, 128 tokens; {a.blocks} alternating blocks of {a.block_steps} steps per arm, ms per step"]
    for name in ("without", "with"):
        lines.append(f"{name:8s} model_ema: mean {statistics.mean(t[name]):7.3f}  median {statistics.median(t[name]):7.3f}  min {min(t[name]):7.3f}  max {max(t[name]):7.3f}")
    lines.append(f"difference of the medians: {1e3 * (statistics.median(t['with']) - statistics.median(t['without'])):+.0f} us per step ({ema.updates} updates made)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40_000_000)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ubench_ema needs an MI355X"
    assert a.n % 4 == 0 and a.launches >= 2
    dev = torch.device("cuda", 0)
    lines = [f"ubench_ema on {torch.cuda.get_device_name(0)}"]
    kernel_part(a, dev, lines)
    if not a.skip_model:
        model_part(a, dev, lines)
    if not a.skip_step:
        step_part(a, dev, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

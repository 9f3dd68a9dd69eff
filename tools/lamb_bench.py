"""The measurements of docs/lamb.md, all in one process on one GPU.

1. Kernel time: the three LAMB launches together against one mvlt_adamw_step on the same 40,000,000-element buffers -- rounds in alternating order,
   LAUNCHES launches per timing between device events, medians over the rounds; bytes per element from the kernels' accesses (LAMB: 16 read + 8 written,
   then 12 read + 4 + 2 written = 42; AdamW: 16 + 1 mask byte read, 12 + 2 written = 31).
2. Host time: what the host spends enqueuing FusedLamb.step() on pvlt_tiny (gradients in place, queue never drained) against a per-tensor Python LAMB
   over the same parameters (torch ops, two norms per tensor kept on the device: no host read either).

    python tools/lamb_bench.py [ROUNDS]
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvlt_amd import ops, pvlt                                            # noqa: E402
from mvlt_amd.optim import FusedAdamW, FusedLamb, lamb_tables            # noqa: E402

DEV = torch.device("cuda", 0)
N, LAUNCHES = 40_000_000, 20
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 12


def kernel_time():
    g_ = torch.Generator(device=DEV).manual_seed(3)
    p, g, m = (torch.randn(N, device=DEV, generator=g_) for _ in range(3))
    g, m = g * 1e-2, m * 1e-2
    v = torch.rand(N, device=DEV, generator=g_) * 1e-4
    p16 = torch.empty(N, dtype=torch.bfloat16, device=DEV)
    mask = torch.ones(N, dtype=torch.uint8, device=DEV)
    hp = torch.tensor([1e-5, 0.9, 0.999, 1e-6, 0.01, 1 - 0.9 ** 3, 1 - 0.999 ** 3, 1.0], device=DEV)
    table = torch.tensor([[1e-5, 0.01], [1e-5, 0.0]], device=DEV)
    # a store shaped like pvlt_tiny's, scaled to N: one 23.4 M-element tensor, then matrices and vectors down to 64 elements
    lens, left = [23_440_896], N - 23_440_896
    for n in [2_359_296, 1_048_576, 589_824, 262_144, 65_536, 16_384, 4_096, 512, 320, 128, 64] * 40:
        if left < n + 8:
            continue
        lens.append(n)
        left -= (n + 7) // 8 * 8
    layout, off = [], 0
    for i, n in enumerate(lens):
        layout.append((off, n, 1 if n < 1024 else 0, False))
        off += (n + 7) // 8 * 8
    tensors, chunks = lamb_tables(layout, N, 2)
    td, cd, nc = tensors.to(DEV), chunks.to(DEV), chunks.shape[0]
    partials, ratios = torch.zeros(nc, 2, device=DEV), torch.ones(len(layout), device=DEV)
    print(f"store: {N} elements, {len(layout)} tensors ({off} covered with gaps), {nc} chunks of {ops.LAMB_CHUNK}")

    def lamb():
        ops.lamb_moments(p, g, m, v, N, hp, td, cd, table, 2, partials)
        ops.lamb_fold(partials, td, nc, table, 2, 0, ratios)
        ops.lamb_apply(p, m, v, p16, N, hp, td, cd, table, 2, ratios)

    def moments():
        ops.lamb_moments(p, g, m, v, N, hp, td, cd, table, 2, partials)

    def fold():
        ops.lamb_fold(partials, td, nc, table, 2, 0, ratios)

    def apply():
        ops.lamb_apply(p, m, v, p16, N, hp, td, cd, table, 2, ratios)

    def adamw():
        ops.adamw_step(p, g, m, v, p16, N, hp, mask)

    variants = [("mvlt_adamw_step", adamw, 31), ("LAMB, three launches", lamb, 42), ("  mvlt_lamb_moments", moments, 24), ("  mvlt_lamb_fold", fold, 0),
                ("  mvlt_lamb_apply", apply, 18)]
    times = {name: [] for name, _, _ in variants}
    for _, f, _ in variants:
        f()
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        for name, f, _ in (variants if r % 2 == 0 else variants[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(LAUNCHES):
                f()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / LAUNCHES)
    base = statistics.median(times["mvlt_adamw_step"])
    print("| launch | ms (median) | min .. max | ratio to `mvlt_adamw_step` | TB/s |\n|---|---|---|---|---|")
    for name, _, bytes_per in variants:
        t = statistics.median(times[name])
        rate = f"{bytes_per * N / t / 1e9:.2f}" if bytes_per else "-"
        print(f"| {name} | {t:.4f} | {min(times[name]):.4f} .. {max(times[name]):.4f} | {t / base:.3f} | {rate} |")
    assert torch.isfinite(p).all().item()


class PythonLamb:
    """LAMB tensor by tensor in torch ops, the way a per-tensor optimizer would run it on this backend: no host read (the trust ratio stays on the device)"""

    def __init__(self, params, lr, wd, eps=1e-6, betas=(0.9, 0.999)):
        self.params, self.lr, self.wd, self.eps, self.betas, self.t = params, lr, wd, eps, betas, 0
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]

    @torch.no_grad()
    def step(self):
        self.t += 1
        b1, b2 = self.betas
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        for p, m, v in zip(self.params, self.m, self.v):
            g = p.grad
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            wd = 0.0 if p.dim() == 1 else self.wd
            u = (m / bc1) / ((v / bc2).sqrt_() + self.eps)
            if wd:
                u.add_(p, alpha=wd)
                wn, un = p.norm(), u.norm()
                r = torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn))
                p.sub_(u * (self.lr * r))
            else:
                p.sub_(u, alpha=self.lr)


def host_time():
    import bench
    from mvlt_amd.engine import train_step
    model = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=128, loss_type=dict(mlm=1, itm=1, t2i=1, cls=0), pretrained_pth=None,
                           drop_path_rate=0.1, drop_rate=0.0, num_classes=1000, in_chans=3).cuda(DEV)
    model.train()
    batch = bench.synth_batch(8, 128, 128, DEV, 1)
    batch["mlm_count"] = int((batch["mlm_labels"] != -1).sum())
    total, _ = train_step(model, batch, 0, True)
    total.backward()                                                     # gradients in place; every optimizer below steps from them
    torch.cuda.synchronize()
    params = [p for p in model.store.params.values() if p.grad is not None]
    rows = []
    for name, opt in (("FusedAdamW.step", FusedAdamW(model, lr=1e-5, weight_decay=0.01)), ("FusedLamb.step", FusedLamb(model, lr=1e-5, weight_decay=0.01)),
                      ("per-tensor Python LAMB", PythonLamb(params, 1e-5, 0.01))):
        for _ in range(5):
            opt.step()
        torch.cuda.synchronize()
        per = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(10):
                opt.step()
            per.append((time.perf_counter() - t0) / 10)
            torch.cuda.synchronize()
        rows.append((name, statistics.median(per), min(per), max(per)))
    print(f"host time to enqueue one optimizer step, pvlt_tiny ({len(params)} tensors that train), queue drained between timings of 10 steps:")
    print("| step | host ms (median of 5) | min .. max |\n|---|---|---|")
    for name, t, lo, hi in rows:
        print(f"| {name} | {1e3 * t:.3f} | {1e3 * lo:.3f} .. {1e3 * hi:.3f} |")


if __name__ == "__main__":
    kernel_time()
    host_time()

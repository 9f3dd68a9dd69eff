"""What freezing parameters saves per training step: pvlt_tiny at the bench's batch (256 pairs, 256 x 256, 128 tokens, bf16), one process, the engine's
step (train_step + BF16Scaler + FusedAdamW) under four settings of requires_grad --
    all     everything trainable (the baseline of its own table)
    text    text_embeddings frozen (the 23 M-element tied word table among them)
    lower   stages 1-2 (blocks, patch / text / position embeddings) + text_embeddings frozen
    heads   only the heads trainable (linear probe)
at ONE configuration per call: `--config finetune` (the CLS heads, bench.py's fine-tune entry), `--config pretrain` (MLM + ITM + MIM), or `--config adamw`
(the optimizer launch alone, word table frozen against unfrozen, device events).  One call = one process = one time limit for the caller to set.
The settings ALTERNATE in rounds of STEPS steps (all, text, lower, heads, all, ...), every round timed with a host clock around work that ends in a device
synchronise; reported are each setting's median ms/step over the rounds with min .. max, the per-round difference to `all`, and
torch.cuda.max_memory_allocated of a step of each setting (the peak counter is reset before it, after the warm-up).

    python tools/ubench_freeze.py --config finetune|pretrain|adamw [--rounds 5] [--steps 10] [--batch 256] [--img 256] [--out FILE]
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
from mvlt_amd.plan import backward_plan    # noqa: E402

EMBEDS = ("patch_embed{}", "text_embed{}", "pos_embed{}", "text_pos_embed{}")
SETTINGS = ("all", "text", "lower", "heads")


def stage_prefixes(*stages):
    return tuple(f"block{i}." for i in stages) + tuple(e.format(i) for i in stages for e in EMBEDS)


def apply_setting(model, setting):
    frozen = dict(all=(), text=("text_embeddings.",), lower=stage_prefixes(1, 2) + ("text_embeddings.",),
                  heads=stage_prefixes(1, 2, 3, 4) + ("text_embeddings.",))[setting]
    for n, p in model.named_parameters():
        p.requires_grad_(not (frozen and n.startswith(frozen)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("finetune", "pretrain", "adamw"), required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ubench_freeze needs an MI355X"
    dev = torch.device("cuda", 0)
    lt = dict(mlm=0, itm=0, t2i=0, cls=1) if a.config == "finetune" else dict(mlm=1, itm=1, t2i=1, cls=0)
    torch.manual_seed(4321)
    model = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=128, loss_type=lt, pretrained_pth=None, drop_path_rate=0.1,
                           drop_rate=0.0, num_classes=1000, in_chans=3).cuda(dev)
    model.train()
    batch = bench.synth_batch(a.batch, a.img, 128, dev, 99)
    batch["mlm_count"] = int((batch["mlm_labels"] != -1).sum())
    opt = FusedAdamW(model, lr=1e-5, weight_decay=0.01)
    scaler = BF16Scaler()
    S = model.store
    t2i_on = bool(lt["t2i"])

    def step(i):
        total, _ = train_step(model, batch, i, t2i_on)
        opt.zero_grad()
        scaler(total, opt, clip_grad=None, parameters=None)

    lines = []
    if a.config == "adamw":
        # the optimizer launch alone: same process, same buffers, the word table's mask bytes flipped between 2 and 1
        for i in range(3):
            step(i)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        res = {}
        for rnd in range(a.rounds):
            for setting in ("all", "text"):
                apply_setting(model, setting)
                opt._ensure()
                for _ in range(3):
                    ops.adamw_step(S.P, S.G, opt._m, opt._v, S.C, S.total, opt._hp, opt._wd_mask)
                ts = []
                for _ in range(20):
                    ev[0].record()
                    ops.adamw_step(S.P, S.G, opt._m, opt._v, S.C, S.total, opt._hp, opt._wd_mask)
                    ev[1].record()
                    torch.cuda.synchronize()
                    ts.append(1e3 * ev[0].elapsed_time(ev[1]))
                res.setdefault(setting, []).append(statistics.median(ts))
        n_fz = int((opt._wd_mask == ops.ADAMW_FROZEN).sum())
        lines.append(f"ubench_freeze adamw: mvlt_adamw_step over {S.total} elements (bf16 copy written), device events, {a.rounds} alternating rounds x median of 20 launches")
        for setting in ("all", "text"):
            t = res[setting]
            lines.append(f"{setting:6s} median {statistics.median(t):8.1f} us   [{min(t):.1f} .. {max(t):.1f}]" + (f"   ({n_fz} elements frozen)" if setting == "text" else ""))
    else:
        for setting in SETTINGS:                       # warm every setting (masks, plans, code objects, the pool's size)
            apply_setting(model, setting)
            for i in range(3):
                step(i)
        torch.cuda.synchronize()
        times = {s: [] for s in SETTINGS}
        peak = {}
        for r in range(a.rounds):
            for setting in SETTINGS:
                apply_setting(model, setting)
                step(0)                                # the first step after a flip rebuilds the optimizer's mask: outside the timed region
                torch.cuda.synchronize()
                if r == 0:
                    torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    step(i)
                torch.cuda.synchronize()
                times[setting].append(1e3 * (time.perf_counter() - t0) / a.steps)
                if r == 0:
                    peak[setting] = torch.cuda.max_memory_allocated() / 2 ** 30
        lines.append(f"ubench_freeze {a.config}: pvlt_tiny bf16, batch {a.batch}, {a.img} x {a.img}, 128 tokens, heads {[k for k, v in lt.items() if v]}; "
                     f"{a.rounds} alternating rounds x {a.steps} steps per setting, host clock around a device synchronise")
        lines.append(f"{'setting':8s} {'median ms/step':>15s} {'min':>9s} {'max':>9s}   {'vs all (median of per-round differences)':>42s}   {'peak GiB':>9s}   cut")
        for setting in SETTINGS:
            t = times[setting]
            d = [x - y for x, y in zip(t, times["all"])]
            apply_setting(model, setting)
            cut = backward_plan(model).cut_unit
            lines.append(f"{setting:8s} {statistics.median(t):15.3f} {min(t):9.3f} {max(t):9.3f}   {statistics.median(d):+10.3f} ms ({100 * statistics.median(d) / statistics.median(times['all']):+6.1f} %)"
                         f" [{min(d):+.3f} .. {max(d):+.3f}]   {peak[setting]:9.2f}   {cut.name if cut else '-'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

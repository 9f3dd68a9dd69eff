"""The table of docs/ingest.md: what a batch of images costs between pinned host memory and the (clean, grid-masked) fp32 pair on the device, three ways, on
one stream, interleaved in one process --

  (a) the fp32 path: pinned fp32 (B,3,S,S) -> device, then mvlt_grid_mask_apply
  (b) uint8 at the output size: pinned uint8 (B,S,S,3) -> device, then mvlt_image_ingest (table lookup, both outputs in one pass)
  (c) uint8 slabs of 2S pixels: pinned uint8 (B,2S,2S,3) -> device, then mvlt_image_ingest_resize (rectangle -> S x S, flip, both outputs in one pass)

each as copy + kernel and as the kernel alone (device events around `iters` back-to-back calls), with the bytes each kernel has to move over its time; and, on
the CPU, the cost per image of what (c) takes off the loader workers: PIL resize(BILINEAR) 2S -> S plus ToTensor.

    python tools/ubench_ingest.py [--batch 256] [--size 256] [--iters 20] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3              # us per call


def host_cost(S, n=40):
    """ms per image, one thread: PIL resize of a 2S x 2S RGB image to S x S + ToTensor (uint8 HWC -> fp32 CHW / 255)"""
    try:
        from PIL import Image
    except ImportError:
        return None
    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    imgs = [Image.fromarray(rng.integers(0, 256, size=(2 * S, 2 * S, 3), dtype=np.uint8)) for _ in range(8)]
    for timed in (False, True):
        t0 = time.perf_counter()
        for i in range(n if timed else 4):
            small = imgs[i % 8].resize((S, S), Image.BILINEAR)
            torch.from_numpy(np.array(small)).permute(2, 0, 1).contiguous().float().div(255)
        dt = time.perf_counter() - t0
    return dt / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mvlt_amd import build, ops
    if not torch.cuda.is_available():
        raise SystemExit("ubench_ingest.py measures on the GPU: no device, no number")
    dev, B, S = "cuda:0", args.batch, args.size
    g = torch.Generator().manual_seed(0)
    h_f32 = torch.rand(B, 3, S, S, generator=g).pin_memory()
    h_u8 = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g).pin_memory()
    h_slab = torch.randint(0, 256, (B, 2 * S, 2 * S, 3), dtype=torch.uint8, generator=g).pin_memory()
    rects_host = torch.tensor([[b % 7, b % 5, 2 * S - 8, 2 * S - 6] for b in range(B)], dtype=torch.int32)
    rects = rects_host.to(dev)
    flags = torch.empty(B, (S // 16) ** 2, dtype=torch.uint8, device=dev)
    ops.grid_mask_flags(flags, B, S // 16, S // 16, (S // 16) ** 2 // 2, 0, 1, 0)
    flip = ops.flip_flags(torch.empty(B, dtype=torch.uint8, device=dev), 0.5, 1, 0)
    table = ops.ingest_table().to(dev)
    d_f32, d_u8, d_slab = (torch.empty(t.shape, dtype=t.dtype, device=dev) for t in (h_f32, h_u8, h_slab))
    image, masked = torch.empty(B, 3, S, S, device=dev), torch.empty(B, 3, S, S, device=dev)

    k_a = lambda: ops.grid_mask_apply(d_f32, flags, masked)
    k_b = lambda: ops.image_ingest(d_u8, table, image, masked, flags)
    k_c = lambda: ops.image_ingest_resize(d_slab, rects, rects_host, image, masked, flags, flip)
    out_bytes = 2 * B * 3 * S * S * 4
    rows = {
        "a": ("fp32 H2D + grid_mask_apply", lambda: (d_f32.copy_(h_f32, non_blocking=True), k_a()), k_a, h_f32.numel() * 4, 2 * h_f32.numel() * 4 + flags.numel()),
        "b": ("uint8 H2D + image_ingest", lambda: (d_u8.copy_(h_u8, non_blocking=True), k_b()), k_b, h_u8.numel(), h_u8.numel() + out_bytes + flags.numel()),
        "c": ("uint8 2S slabs H2D + image_ingest_resize", lambda: (d_slab.copy_(h_slab, non_blocking=True), k_c()), k_c, h_slab.numel(),
              int(rects_host[:, 2:].prod(1).sum()) * 3 + out_bytes + flags.numel()),
    }
    for _, full, kern, _, _ in rows.values():             # warm up every shape the timed window uses
        for _ in range(3):
            full(), kern()
    torch.cuda.synchronize()
    t_full, t_kern = {k: [] for k in rows}, {k: [] for k in rows}
    for _ in range(args.rounds):                          # interleaved: a b c a b c ...
        for k, (_, full, kern, _, _) in rows.items():
            t_full[k].append(_timed(full, args.iters))
            t_kern[k].append(_timed(kern, args.iters))
    res = dict(device=torch.cuda.get_device_name(0), source_hash=build.source_hash(), batch=B, size=S, iters=args.iters, rounds=args.rounds, rows={})
    print(f"{res['device']}, batch {B}, {S} px, {args.rounds} rounds of {args.iters} calls, median [min .. max] in us")
    print(f"{'':44s} {'copy + kernel':>26s} {'kernel alone':>26s} {'H2D MB':>8s} {'kernel MB':>10s} {'kernel GB/s':>12s}")
    for k, (name, _, _, h2d, moved) in rows.items():
        f, kn = np.array(t_full[k]), np.array(t_kern[k])
        gbs = moved / np.median(kn) / 1e3
        res["rows"][k] = dict(name=name, full_us=[float(np.median(f)), float(f.min()), float(f.max())], kernel_us=[float(np.median(kn)), float(kn.min()), float(kn.max())],
                              h2d_bytes=int(h2d), kernel_bytes=int(moved), kernel_GBps=float(gbs))
        print(f"({k}) {name:40s} {np.median(f):9.1f} [{f.min():7.1f} .. {f.max():7.1f}] {np.median(kn):9.1f} [{kn.min():7.1f} .. {kn.max():7.1f}] {h2d / 1e6:8.1f} {moved / 1e6:10.1f} {gbs:12.0f}")
    ms = host_cost(S)
    res["host_ms_per_image"] = ms
    print("host, one thread, per image: PIL resize(BILINEAR) %d -> %d + ToTensor: %s" % (2 * S, S, "PIL not installed: not measured" if ms is None else f"{ms:.3f} ms"))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

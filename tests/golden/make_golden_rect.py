#!/usr/bin/env python3
"""Generate tests/golden/rect_tiny256x192.npz: the REAL reference on a rectangular (256 x 192, H x W) input.

Same recipe as tests/golden/make_golden.py (its timm / BertConfig shims, filler weights, injected train-mode masks), for the
shape class that file does not cover: pvlt_tiny with every head, batch 2, T = 128.  `oracle/filler.py:make_batch` makes
square batches, so the batch is made at max(H, W) and `image` / `masked_images` are cropped to [..., :H, :W] -- the grid
mask is built from 16-pixel patches, so a crop at multiples of 32 keeps the clean and the masked image consistent
(`rect_batch` below; the tests import it).

The script first asserts oracle == reference on this input (eval forward incl. the four stage outputs, one train step's
losses, gradients and BatchNorm statistics), then stores the REFERENCE's numbers:
  eval   stats + strided sample of the stage outputs and of every head output, the small heads in full, the MLM top-8 at
         the masked positions, a 16 x 12 grid of the MIM output
  train1 (grid-masked image, injected masks) the losses, every gradient's norm and a 32-value strided sample
tests/test_rect_cpu.py pins the oracle to this fixture, tests/test_rect_gpu.py pins the model to it.

Runs only where the reference checkout is present; the .npz it writes is committed.

usage: python tests/golden/make_golden_rect.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import filler  # noqa: E402
from oracle import pvlt_oracle as O  # noqa: E402

SEED = 20240611
NAME = "rect_tiny256x192"
CASE = dict(variant="pvlt_tiny", H=256, W=192, T=128, B=2, lt=dict(mlm=1, itm=1, t2i=1, cls=1), dp=0.1, step=1)


def rect_batch(seed, B, H, W, T):
    """a filler batch with (B, 3, H, W) images: the square batch at max(H, W), `image` and `masked_images` cropped to the top-left H x W"""
    nb = dict(filler.make_batch(seed, B, max(H, W), T))
    for k in ("image", "masked_images"):
        nb[k] = np.ascontiguousarray(nb[k][..., :H, :W])
    return O.to_torch_batch(nb)


def main():
    from tests.golden import make_golden as MG
    MG.install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from libs import pvlt as ref_pvlt
    from timm.models.layers import DropPath
    c = CASE
    H, W, T, B = c["H"], c["W"], c["T"], c["B"]
    cfg = O.Cfg(c["variant"], c["lt"], 224, 768, T, c["dp"])
    sd = O.filled_state_dict(cfg, SEED)
    ref = getattr(ref_pvlt, c["variant"])(pretrained=True, token_hidden_size=768, num_text_tokens=T, loss_type=c["lt"], pretrained_pth=None,
                                         drop_path_rate=c["dp"], drop_rate=0.0, num_classes=1000, in_chans=3)
    ref.load_state_dict(sd, strict=True)
    batch = rect_batch(SEED, B, H, W, T)
    assert tuple(batch["image"].shape) == (B, 3, H, W)
    G = {"meta": np.array([SEED, B, H, W, T, c["dp"], c["step"]], dtype=np.float64)}

    # ---------------- eval forward
    ref.eval()
    with torch.no_grad():
        img_feats, text_feats = ref.forward_pyramid_features_vl(batch["image"], batch["input_ids"])
        out_ref = ref(batch["image"], batch["input_ids"])
    taps_ref = {}
    for i in range(4):
        assert tuple(img_feats[i].shape[2:]) == (H // (4 * 2 ** i), W // (4 * 2 ** i)), img_feats[i].shape
        taps_ref[f"img_feat{i+1}"], taps_ref[f"text_feat{i+1}"] = img_feats[i], text_feats[i]
    taps = {}
    with torch.no_grad():
        out = O.forward(sd, cfg, batch["image"], batch["input_ids"], train=False, taps=taps)
    worst = 0.0
    for k, v in taps_ref.items():
        assert tuple(taps[k].shape) == tuple(v.shape), (k, taps[k].shape, v.shape)
        worst = max(worst, MG.relerr(taps[k], v))
        G[f"eval/tap/{k}/stats"] = MG.stats(v)
        G[f"eval/tap/{k}/sample"] = MG.sample(v, 1024)
    for k, v in out_ref.items():
        assert v is not None and tuple(out[k].shape) == tuple(v.shape), (k, out[k].shape, v.shape)
        worst = max(worst, MG.relerr(out[k], v))
        G[f"eval/out/{k}/stats"] = MG.stats(v)
        G[f"eval/out/{k}/sample"] = MG.sample(v, 4096)
        G[f"eval/out/{k}/shape"] = np.array(v.shape, dtype=np.int64)
    assert worst < 5e-5, (NAME, "oracle != reference (eval)", worst)
    assert tuple(out_ref["t2i_logits"].shape) == (B, 3, H, W)
    for k in ("itm_logits", "sup_cls_logits", "sub_cls_logits"):
        G[f"eval/full/{k}"] = out_ref[k].numpy().copy()
    pos = O.masked_positions(batch["mlm_labels"])
    G["masked_positions"] = pos.numpy().astype(np.int64)
    rows = out_ref["mlm_logits"].reshape(-1, O.VOCAB)[pos]
    tv, ti = rows.topk(8, dim=-1)
    G["eval/mlm/top8_val"], G["eval/mlm/top8_idx"] = tv.numpy().copy(), ti.numpy().astype(np.int64)
    G["eval/t2i/grid"] = out_ref["t2i_logits"][:, :, ::16, ::16].numpy().copy()
    print(f"[{NAME}] eval oracle-vs-reference worst rel err {worst:.2e}")

    # ---------------- one train-mode step on the grid-masked image, injected masks
    step_idx = c["step"]
    masks = MG.make_masks(cfg, B, T, SEED + step_idx)
    ref.train()
    ref.load_state_dict(sd, strict=True)
    ref.text_embeddings.dropout = MG.FixedDropout(masks["bert"], 0.1)
    q = []
    for k in range(sum(cfg.depths)):
        if cfg.dpr[k] > 0:
            q += [masks["droppath"][k], masks["droppath2"][k]]
    DropPath.QUEUE = q
    ref.zero_grad()
    out_r = ref(batch["masked_images"], batch["input_ids"])
    l_r = O.losses(out_r, batch)
    l_r["total_loss"].backward()
    assert len(q) == 0
    DropPath.QUEUE = None
    g_ref = {k: p.grad for k, p in ref.named_parameters()}
    sdg = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running_" not in k) else v) for k, v in sd.items() if k != O.TIED[0]}
    sdg[O.TIED[0]] = sdg[O.TIED[1]]
    bn_out = {}
    l_o, _ = O.step_loss(sdg, cfg, batch, step_idx, train=True, masks=masks, bn_out=bn_out)
    l_o["total_loss"].backward()
    worst = 0.0
    for k, v in l_r.items():
        worst = max(worst, abs(float(v) - float(l_o[k])) / max(1e-12, abs(float(v))))
        G[f"train{step_idx}/loss/{k}"] = np.array(float(v))
    for k, g in g_ref.items():
        if g is None:
            continue
        worst = max(worst, MG.relerr(sdg[k].grad, g))
        G[f"train{step_idx}/grad/{k}/norm"] = np.array(g.double().norm().item())
        G[f"train{step_idx}/grad/{k}/sample"] = MG.sample(g, 32)
    for k, v in ref.state_dict().items():
        if "running_" in k:
            worst = max(worst, MG.relerr(bn_out[k], v))
    assert worst < 2e-4, (NAME, "oracle != reference (train)", worst)
    print(f"[{NAME}] train step {step_idx} oracle-vs-reference worst rel err {worst:.2e}; losses", {k: round(float(v), 5) for k, v in l_r.items()})
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **G)
    print(f"[{NAME}] wrote {path} ({os.path.getsize(path)/1024:.1f} KiB, {len(G)} arrays)")


if __name__ == "__main__":
    main()

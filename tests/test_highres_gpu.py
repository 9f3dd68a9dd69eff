"""GPU: the whole model where its SR-attention has more keys than the LDS-resident kernels hold (M = (S/32)^2 + T > 320): pvlt_tiny with
every head at 384 px / T = 180 (M = 324), 512 px / T = 128 (M = 384) and 256 px / T = 320 (M = 384), batch 2, both compute dtypes,
against the CPU oracle run live on the same filler weights and inputs (the pattern of tests/test_model_gpu.py); the engine loop
at 512 px through the reference's import path; and 448 px, which the reference itself cannot run (stage 2's 56 x 56 grid has stage 1's
constructor patch count, so reference libs/pvlt.py:292 hands it the unresized 28 x 28 embedding), refused by the model as by the oracle.
Bounds (north_star): eval outputs 1e-3 max-abs / max-abs (fp32) and 2e-2 relative L2 (bf16; the ITM logits through their class
probabilities); gradients of one train step within test_train_step_parity's gates (2e-4 fp32, 8e-2 bf16)."""
import types

import numpy as np
import pytest
import torch

from oracle import filler
from oracle.hostinfo import usable_cores
from oracle import pvlt_oracle as O

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
TOL = {F32: 1e-3, BF: 2e-2}
GTOL = {F32: 2e-4, BF: 8e-2}
LT = dict(mlm=1, itm=1, t2i=1, cls=1)
CASES = {"384px_T180": (384, 180), "512px_T128": (512, 128), "256px_T320": (256, 320)}
B, SEED, DP = 2, 23, 0.1
_ORACLE = {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def setup(img, T, dtype, seed=SEED):
    from mvlt_amd import pvlt
    cfg = O.Cfg("pvlt_tiny", LT, 224, 768, T, DP)
    sd = O.filled_state_dict(cfg, seed)
    model = pvlt.pvlt_tiny(pretrained=True, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None,
                           drop_path_rate=DP, drop_rate=0.0, num_classes=1000, in_chans=3, compute_dtype=dtype)
    model.load_state_dict(sd, strict=True)
    model.cuda(dev())
    return model, cfg, sd


def out_err(k, o, v, dtype):
    o, v = o.detach().double().cpu(), v.detach().double().cpu()
    if dtype == F32:
        return ((o - v).abs().max() / v.abs().max().clamp_min(1e-30)).item()
    if k == "itm_logits":                               # B x 2 numbers near cancellation: their class probabilities (test_model_gpu.py)
        return (o.softmax(-1) - v.softmax(-1)).abs().max().item()
    return ((o - v).norm() / v.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("name", list(CASES))
def test_eval_forward_matches_oracle(parity, name, dtype):
    from mvlt_amd import ops
    img, T = CASES[name]
    model, cfg, sd = setup(img, T, dtype)
    batch = O.to_torch_batch(filler.make_batch(SEED, B, img, T))
    model.eval()
    with torch.no_grad():
        out = model(batch["image"].to(dev()), batch["input_ids"].to(dev()))
    torch.cuda.synchronize()
    if ("eval", name) not in _ORACLE:
        torch.set_num_threads(usable_cores())
        with torch.no_grad():
            _ORACLE[("eval", name)] = O.forward(sd, cfg, batch["image"], batch["input_ids"])
    ref = _ORACLE[("eval", name)]
    bad = {}
    for k, v in ref.items():
        assert v is not None and out[k] is not None, k
        assert tuple(out[k].shape) == tuple(v.shape), (k, out[k].shape, v.shape)
        assert torch.isfinite(out[k].float()).all(), k
        e = out_err(k, out[k], v, dtype)
        if not parity(f"out/{k}", e, TOL[dtype]):
            bad[k] = e
    assert len(ref) == 5 and not bad, (name, str(dtype), bad)
    # masked-index selection, bit-exact
    lab = batch["mlm_labels"].to(dev()).reshape(-1).contiguous()
    idx = torch.empty(lab.numel(), device=dev(), dtype=torch.int32)
    cnt = torch.zeros(1, device=dev(), dtype=torch.int32)
    ops.masked_select(lab, idx, cnt)
    n = int(cnt.item())
    assert np.array_equal(idx[:n].cpu().numpy().astype(np.int64), O.masked_positions(batch["mlm_labels"]).numpy())


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("name", list(CASES))
def test_train_step_matches_oracle(parity, name, dtype):
    """one train-mode step on the grid-masked image (t2i on: engine iteration 1) with injected dropout / DropPath masks, through the
    engine's fused masked-row MLM path: losses and every parameter gradient against the oracle's autograd"""
    from mvlt_amd.engine import compute_losses
    from tests.golden.make_golden import make_masks
    img, T = CASES[name]
    model, cfg, sd = setup(img, T, dtype)
    batch = O.to_torch_batch(filler.make_batch(SEED, B, img, T))
    step_idx = 1
    masks = make_masks(cfg, B, T, SEED + step_idx)
    model.train()
    model.injected_masks = masks
    db = {k: v.to(dev()) for k, v in batch.items()}
    out = model(db["masked_images"], db["input_ids"], mlm_labels=db["mlm_labels"])
    total, parts = compute_losses(out, db["image"], db["mlm_labels"], db["itm_labels"], db["sup_cls_labels"], db["sub_cls_labels"])
    total.backward()
    torch.cuda.synchronize()
    if ("train", name) not in _ORACLE:
        sdg = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running_" not in k) else v)
               for k, v in sd.items() if k != O.TIED[0]}
        sdg[O.TIED[0]] = sdg[O.TIED[1]]
        torch.set_num_threads(usable_cores())
        lo, _ = O.step_loss(sdg, cfg, batch, step_idx, train=True, masks=masks, bn_out={})
        lo["total_loss"].backward()
        _ORACLE[("train", name)] = ({k: float(v) for k, v in lo.items()},
                                    {k: v.grad for k, v in sdg.items() if v.is_floating_point() and v.grad is not None})
    lo, grads = _ORACLE[("train", name)]
    ls = dict(parts, total_loss=total)
    for k, ref in lo.items():
        assert parity(f"loss/{k}", abs(float(ls[k]) - ref) / max(1.0, abs(ref)), TOL[dtype]), (k, float(ls[k]), ref)
    # the ITM head's bias gradients are batch sums of signed per-pair residuals that cancel: on the bf16 path they are gated against the
    # un-cancelled scale, as test_model_gpu.py::test_train_step_parity does
    cancel = {}
    if dtype == BF:
        pr = out["itm_logits"].detach().float().reshape(B, 2).softmax(-1).cpu().numpy().astype(np.float64)
        a_b = pr[:, 0] - (batch["itm_labels"].reshape(-1).numpy() == 0)
        c_itm = max(1.0, float(np.sqrt((a_b ** 2).sum()) / max(1e-12, abs(a_b.sum()))))
        cancel = {"itm_head.linear.bias": c_itm, "itm_head.linear_bias": c_itm, "itm_head_embed.1.bias": c_itm}
    gtol = GTOL[dtype]
    bad, n = {}, 0
    for k, p in model.named_parameters():
        ref = grads.get(k)
        if ref is None or ref.double().norm().item() < 1e-7:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        n += 1
        c_k = cancel.get(k, 1.0)
        refn = ref.double().norm().item()
        en = abs(p.grad.double().norm().item() - refn) / (refn * c_k)
        ef = ((p.grad.detach().double().cpu() - ref.double()).norm() / ref.double().norm()).item() / c_k
        if not (parity("grad-norm/" + k, en, gtol) & parity("grad-full/" + k, ef, gtol)):
            bad[k] = (en, ef)
    assert n > 50
    assert not bad, (name, str(dtype), len(bad), sorted(bad.items(), key=lambda kv: -kv[1][1])[:10])


@pytest.mark.parametrize("dtype", [F32, BF])
def test_448px_is_refused_like_the_reference(dtype):
    """at 448 px the reference's `_get_pos_embed` returns stage 2's 28 x 28 embedding for a 56 x 56 grid and `x + pos_embed` raises; the
    model must raise too (it used to read 3136 rows of a 784-row parameter) -- eval and train mode"""
    img, T = 448, 128
    model, cfg, sd = setup(img, T, dtype)
    batch = O.to_torch_batch(filler.make_batch(SEED, B, img, T))
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            O.forward(sd, cfg, batch["image"], batch["input_ids"])
    model.eval()
    with pytest.raises(RuntimeError, match="unresized"):
        with torch.no_grad():
            model(batch["image"].to(dev()), batch["input_ids"].to(dev()))
    model.train()
    with pytest.raises(RuntimeError, match="unresized"):
        model(batch["image"].to(dev()), batch["input_ids"].to(dev()), mlm_labels=batch["mlm_labels"].to(dev()))
    torch.cuda.synchronize()


class _Loader:
    """list-of-dicts loader that also injects the iteration's dropout / DropPath draws into the model (tests/test_engine_gpu.py)"""

    def __init__(self, model, batches, masks):
        self.model, self.batches, self.masks = model, batches, masks

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for it, b in enumerate(self.batches):
            self.model.injected_masks = self.masks[it]
            yield b


@pytest.mark.parametrize("dtype", [F32, BF])
def test_engine_loop_at_512px(parity, dtype):
    """`train_one_epoch_vl` imported the way reference main_vl.py:198 does, two iterations (clean image, then grid-masked) at 512 px:
    finite losses; on the fp32 path the epoch averages match the oracle's loop (same weights, batches and masks; AdamW steps)"""
    import engine_grid_masking as E
    from mvlt_amd.engine import BF16Scaler
    from mvlt_amd.optim import FusedAdamW
    from tests.golden.make_golden import make_masks
    img, T, iters, lr, wd = 512, 128, 2, 1e-4, 0.05
    model, cfg, sd = setup(img, T, dtype, seed=SEED + 1)
    batches = [O.to_torch_batch(filler.make_batch(SEED + 100 * it, B, img, T)) for it in range(iters)]
    masks = [make_masks(cfg, B, T, SEED + it) for it in range(iters)]
    opt = FusedAdamW(model, lr=lr, weight_decay=wd)
    args = types.SimpleNamespace(loss_type=cfg.loss_type)
    seen = []
    fwd = model.forward
    model.forward = lambda im, ids, **kw: (seen.append(float(im.float().mean())), fwd(im, ids, **kw))[1]
    res = E.train_one_epoch_vl(model, None, _Loader(model, batches, masks), opt, dev(), 0, BF16Scaler(), None, None, None, True, False, args)
    model.forward = fwd
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in res.values()), res
    for it, mean in enumerate(seen):
        want = batches[it]["masked_images" if it % 2 == 1 else "image"].mean().item()
        assert abs(mean - want) < 1e-5, (it, mean, want)
    if dtype != F32:
        return
    torch.set_num_threads(usable_cores())
    hist, _ = O.train_loop(sd, cfg, batches, masks, lr, wd)
    for k in hist[0]:
        ref = sum(h[k] for h in hist) / iters
        assert parity(f"epoch-avg/{k}", abs(res[k] - ref) / max(1.0, abs(ref)), TOL[F32]), (k, res[k], ref)

"""GPU: fused gradient clipping -- the one-pass global norm over the flat gradient buffer (mvlt_grad_sumsq + mvlt_clip_coef), the clip coefficient
riding in the fused AdamW kernel as a device scalar (mvlt_adamw_step's gscale_dev), mvlt_scale_by_dev for readers that need clipped gradients in
memory, and the store / optimizer / scaler plumbing above them (FlatStore.clip_grad_norm, FusedAdamW.step, BF16Scaler, optim.clip_grad_norm_).
The reference is torch.nn.utils.clip_grad_norm_ (what timm's NativeScaler runs at reference engine_grid_masking.py:126) and float64 norms."""
import types

import numpy as np
import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Tolerance of the norm against float64: 1e-5 relative.  Per lane the kernel adds runs of at most 35 vectors into one accumulator and folds the runs
# into a second one; the largest case here (n = 1 << 20 through ONE workgroup: 1024 vectors per lane) makes that 32 + 32 serial additions, followed
# by 2 (components) + 6 (wave butterfly) + 4 (waves) + at most 4 + 6 + 4 (the fold of the partials) tree steps: a worst-case chain of 90 roundings
# of non-negative terms (fma: the squares add no rounding of their own), 90 * 2^-24 = 5.4e-6 on the sum, half of that on its square root, plus one
# rounding each for sqrt and the grad_scale product: < 3e-6.
NORM_TOL = 1e-5


def _randn(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g) * 1e-3).to(DEV)


def _norm(g, n_partials, grad_scale=1.0, max_norm=1.0, mask=None):
    from mvlt_amd import ops
    part = torch.full((n_partials,), float("nan"), device=DEV)          # a workgroup that does not store shows up
    out = torch.full((2,), float("nan"), device=DEV)
    ops.grad_sumsq(g, g.numel(), mask, part)
    ops.clip_coef(part, grad_scale, max_norm, out)
    return part, out


@pytest.mark.parametrize("n_partials", [1, 7, 256, 1024])
@pytest.mark.parametrize("n", [4, 1028, 4 * (256 * 3 + 1), 1 << 20])
def test_norm_matches_float64(parity, n, n_partials):
    g = _randn(n, n + n_partials)
    grad_scale = 0.5
    part, out = _norm(g, n_partials, grad_scale=grad_scale)
    assert torch.isfinite(part).all(), "a workgroup left its partial unwritten"
    ref = grad_scale * float(torch.linalg.vector_norm(g.double()))
    got = float(out[0])
    print(f"n={n} n_partials={n_partials}: norm {got:.9e} ref {ref:.9e} rel {abs(got - ref) / ref:.3e}")
    assert parity(f"clip-norm/{n}/{n_partials}", abs(got - ref) / ref, NORM_TOL)
    if n == 4 and n_partials == 1024:
        assert int((part != 0).sum()) == 1 and float(part[1:].abs().sum()) == 0.0          # idle workgroups store 0


def test_mask_selects_elements(parity):
    n = 4 * (256 * 3 + 1)
    g = _randn(n, 5)
    gen = torch.Generator().manual_seed(6)
    rnd = torch.randint(0, 3, (n,), generator=gen, dtype=torch.uint8)          # (a byte that is neither 0 nor 1 does not select)
    runs = torch.zeros(n, dtype=torch.uint8)
    for lo, hi in ((1, 7), (10, 11), (13, 1030), (2051, 2054), (n - 3, n)):          # runs that start and end off the 4-element vectors
        runs[lo:hi] = 1
    for name, m in (("random", rnd), ("runs", runs)):
        md = m.to(DEV)
        gm = g.clone()
        gm[md != 1] = float("nan")                  # what the mask excludes must not be read into the sum at all
        for n_partials in (1, 7):
            part, out = _norm(gm, n_partials, mask=md)
            ref = float(torch.linalg.vector_norm(g[md == 1].double()))
            got = float(out[0])
            print(f"mask {name} n_partials={n_partials}: norm {got:.9e} ref {ref:.9e}")
            assert parity(f"clip-mask/{name}/{n_partials}", abs(got - ref) / ref, NORM_TOL)
    part, out = _norm(g, 7, max_norm=0.25, mask=torch.zeros(n, dtype=torch.uint8, device=DEV))
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0


def test_norm_is_bit_identical_from_run_to_run():
    g = _randn(1 << 20, 7)
    pa, oa = _norm(g, 1024)
    pb, ob = _norm(g, 1024)
    assert torch.equal(pa, pb) and torch.equal(oa, ob)
    assert pa.data_ptr() != pb.data_ptr()


def test_coefficient_follows_torch():
    g = _randn(1028, 8)
    _, out = _norm(g, 7, max_norm=1.0)
    norm = out[0].cpu()
    assert float(norm) < 1.0 and float(out[1]) == 1.0                    # above the norm: exactly 1
    max_norm = 0.5 * float(norm)
    _, out = _norm(g, 7, max_norm=max_norm)
    want = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (out[0].cpu() + 1e-6), max=1.0)      # clip_grad_norm_'s formula, in fp32 as torch runs it
    got = out[1].cpu()
    ulp = float(np.spacing(np.float32(want.item())))
    print(f"coef {float(got):.9e} want {float(want):.9e} ulp {ulp:.3e}")
    assert abs(float(got) - float(want)) <= ulp
    g[517] = float("inf")
    _, out = _norm(g, 7, max_norm=max_norm)
    assert not torch.isfinite(out[0]).item()
    want = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (out[0].cpu() + 1e-6), max=1.0)
    assert float(out[1]) == float(want) == 0.0


def _adamw_state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p, gr, m = (torch.randn(n, generator=g).to(DEV) for _ in range(3))
    v = torch.rand(n, generator=g).to(DEV)
    return p, gr * 1e-2, m * 1e-2, v * 1e-4


def _adamw(hp7, c, n=4 * (256 * 2 + 3)):
    from mvlt_amd import ops
    p, g, m, v = _adamw_state(n, 21)
    p16 = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    mask = (torch.arange(n, device=DEV) % 3 != 0).to(torch.uint8)
    hp = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05, 1 - 0.9 ** 3, 1 - 0.999 ** 3, hp7], dtype=torch.float32, device=DEV)
    cd = None if c is None else torch.tensor([c], dtype=torch.float32, device=DEV)
    ops.adamw_step(p, g, m, v, p16, n, hp, mask, gscale_dev=cd)
    return p, m, v, p16


def test_adamw_takes_the_clip_coefficient_from_the_device():
    got = _adamw(0.5, 0.37)
    combined = float(torch.tensor(0.5, dtype=torch.float32) * torch.tensor(0.37, dtype=torch.float32))      # the fp32 product the kernel forms
    want = _adamw(combined, None)
    plain = _adamw(0.5, None)
    one = _adamw(0.5, 1.0)
    for a, b, c, d in zip(got, want, plain, one):
        assert torch.equal(a, b)
        assert torch.equal(c, d)
    assert not torch.equal(got[1], plain[1])


def test_scale_by_dev():
    from mvlt_amd import ops
    x = _randn(1028, 9)
    for c in (0.37, 1.0, 0.0):
        y = x.clone()
        cd = torch.tensor([c], dtype=torch.float32, device=DEV)
        ops.scale_by_dev(y, y.numel(), cd)
        assert torch.equal(y, x * cd)


# ------------------------------------------------------------------------------------------------------------------ model level
LT = dict(mlm=1, itm=1, t2i=0, cls=0)
T, B, IMG = 16, 2, 64          # the smallest configuration tests/test_engine_gpu.py builds


def _model(dtype, seed=8, freeze=None):
    from mvlt_amd import pvlt
    cfg = O.Cfg("pvlt_tiny", LT, 224, 768, T, 0.0)
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, drop_path_rate=0.0, compute_dtype=dtype)
    m.load_state_dict(O.filled_state_dict(cfg, seed), strict=True)
    m.cuda().train()
    if freeze is not None:
        for p in getattr(m, freeze).parameters():
            p.requires_grad_(False)
    m.injected_masks = dict(bert=torch.ones(B, T, 768), droppath=[torch.ones(B)] * 8, droppath2=[torch.ones(B)] * 8)
    return m


def _backward(m, seed=8):
    from mvlt_amd.engine import compute_losses
    b = {k: v.to(DEV) for k, v in O.to_torch_batch(filler.make_batch(seed, B, IMG, T)).items()}
    out = m(b["image"], b["input_ids"], mlm_labels=b["mlm_labels"])
    total, _ = compute_losses(out, b["image"], b["mlm_labels"], b["itm_labels"], b["sup_cls_labels"], b["sub_cls_labels"])
    for p in m.parameters():
        p.grad = None
    total.backward()
    torch.cuda.synchronize()
    S = m.store
    holders = []                                          # torch's function on CLONES of the .grad tensors: the model's own stay untouched
    for p in m.parameters():
        if p.grad is not None:
            h = torch.zeros_like(p, requires_grad=True)
            h.grad = p.grad.clone()
            holders.append(h)
    ref_norm = float(torch.nn.utils.clip_grad_norm_(holders, 1e30))
    return S, S.G.clone(), ref_norm


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_clipped_step_matches_torch(parity, dtype):
    from mvlt_amd.optim import FusedAdamW
    m = _model(dtype)
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    S, snap, ref_norm = _backward(m)
    max_norm = 0.5 * ref_norm                            # the clip bites
    norm = S.clip_grad_norm(max_norm)
    assert norm.is_cuda and norm.dim() == 0 and S.pending_clip is not None
    opt.step()
    torch.cuda.synchronize()
    assert S.pending_clip is None
    print(f"{dtype}: norm {float(norm):.9e} torch {ref_norm:.9e}")
    assert parity("clip-model/norm", abs(float(norm) - ref_norm) / ref_norm, 1e-5)
    assert torch.equal(S.G, snap)                        # the clip did not rewrite the gradients
    # The MOMENTS are compared: Adam's first parameter step is m / sqrt(v) = sign(g) whatever the gradient's scale, so the parameters would pass
    # with no clipping at all.  (frozen / gap elements: zero gradient, zero moment on both sides)
    coef_ref = min(1.0, max_norm / (ref_norm + 1e-6))
    b1 = opt.param_groups[0]["betas"][0]
    assert parity("clip-model/moment", _rel(opt._m, (1 - b1) * coef_ref * snap), 2e-5)
    assert _rel(opt._m, (1 - b1) * snap) > 0.4           # ... and an unclipped step is far outside that bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_clip_that_does_not_bite_equals_an_unclipped_step(dtype):
    from mvlt_amd.optim import FusedAdamW
    m = _model(dtype)
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    S, snap, ref_norm = _backward(m)
    p0 = S.P.clone()
    S.clip_grad_norm(2 * ref_norm)
    opt.step()
    got = (S.P.clone(), opt._m.clone(), opt._v.clone())
    # the same step without clipping, from the same parameters and gradients, moments from zero
    S.P.copy_(p0)
    S.G.copy_(snap)
    opt._m.zero_()
    opt._v.zero_()
    opt._step = 0
    opt.step()
    torch.cuda.synchronize()
    for a, b in zip(got, (S.P, opt._m, opt._v)):
        assert torch.equal(a, b)


def test_frozen_parameters_are_left_out_of_the_norm(parity):
    m = _model(torch.float32, freeze="block2")
    S, snap, ref_norm = _backward(m)
    all_norm = float(torch.linalg.vector_norm(snap.double()))
    norm = float(S.clip_grad_norm(1.0))
    S.pending_clip = None
    print(f"frozen block2: norm {norm:.9e} torch {ref_norm:.9e} whole buffer {all_norm:.9e}")
    assert parity("clip-frozen/norm", abs(norm - ref_norm) / ref_norm, 1e-5)


def test_readers_see_final_gradients(parity):
    from mvlt_amd import optim
    m = _model(torch.float32)
    S, snap, ref_norm = _backward(m)
    max_norm = 0.5 * ref_norm
    norm = S.clip_grad_norm(max_norm).clone()
    coef = S.pending_clip.clone()
    S.apply_pending_scale()
    assert S.pending_clip is None
    assert torch.equal(S.G, snap * coef)
    assert abs(float(coef) - max_norm / (float(norm) + 1e-6)) <= 2e-7
    g_store = S.G.clone()
    # the stand-alone function on the same gradients: same norm, same G; through a wrapper and through the store as well
    for handle in (m, types.SimpleNamespace(module=m), S):
        S.G.copy_(snap)
        norm2 = optim.clip_grad_norm_(handle, max_norm)
        assert S.pending_clip is None and S.pending_grad_scale == 1.0
        assert torch.equal(norm2, norm) and torch.equal(S.G, g_store)
    # an owed 1/world is part of the norm and of what is settled
    S.G.copy_(snap)
    S.pending_grad_scale = 0.5
    norm3 = optim.clip_grad_norm_(m, ref_norm)             # the mean gradient's norm is half of ref_norm: no clipping, only the owed factor is settled
    assert parity("clip-readers/half-norm", abs(float(norm3) - 0.5 * ref_norm) / (0.5 * ref_norm), 1e-5)
    assert S.pending_grad_scale == 1.0 and torch.equal(S.G, snap * 0.5)
    torch.cuda.synchronize()


class _Loader:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def test_engine_clips_through_the_fused_path(capsys):
    from mvlt_amd.engine import BF16Scaler, train_one_epoch_vl
    from mvlt_amd.optim import FusedAdamW
    m = _model(torch.bfloat16)
    m.injected_masks = None
    opt = FusedAdamW(m, lr=1e-4, weight_decay=0.05)
    scaler = BF16Scaler()
    batches = [O.to_torch_batch(filler.make_batch(30 + it, B, IMG, T)) for it in range(2)]
    args = types.SimpleNamespace(loss_type=LT)
    dev = torch.device(DEV)
    res = train_one_epoch_vl(m, None, _Loader(batches), opt, dev, 0, scaler, 1e-3, None, None, True, False, args)      # gradient norms here are O(1): 1e-3 bites
    torch.cuda.synchronize()
    assert set(res) == {"lr", "total_loss", "loss_mlm", "loss_itm", "loss_sup_cls", "loss_sub_cls", "loss_t2i"}
    assert all(isinstance(v, float) and np.isfinite(v) for v in res.values())
    n = scaler.last_grad_norm
    assert isinstance(n, torch.Tensor) and n.is_cuda and n.dim() == 0 and float(n) > 1e-3
    S = m.store
    assert S.pending_clip is None and S.pending_grad_scale == 1.0 and not S.scale_in_optimizer
    train_one_epoch_vl(m, None, _Loader(batches), opt, dev, 1, scaler, 0, None, None, True, False, args)
    torch.cuda.synchronize()
    assert scaler.last_grad_norm is None

"""GPU: frozen parameters (requires_grad=False) are honoured at every layer -- the third value of mvlt_adamw_step's mask byte, FusedAdamW leaving frozen
parameters / moments / bf16 copies alone, the backward pruned to the plan of mvlt_amd.plan.backward_plan (same gradients for what stays trainable,
no launches for what does not), freeze -> un-freeze on one optimizer, the engine loop in the fine-tune shape, and two data-parallel ranks.
The yardsticks are torch.optim.AdamW and the build's own all-trainable run on the same batch; shapes are the smallest the suite builds
(tests/test_clip_gpu.py)."""
import contextlib
import hashlib
import os
import socket
import types

import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LT = dict(mlm=1, itm=1, t2i=0, cls=0)
LT_CLS = dict(mlm=0, itm=0, t2i=0, cls=1)
T, B, IMG = 16, 2, 64
EMBEDS = ("patch_embed{}", "text_embed{}", "pos_embed{}", "text_pos_embed{}")
NT = 256                                   # threads per workgroup of the element-wise kernels (csrc/common.h)


def stage_prefixes(*stages):
    return tuple(f"block{i}." for i in stages) + tuple(e.format(i) for i in stages for e in EMBEDS)


def apply_setting(m, setting):
    single = dict(one="block2.1.mlp.fc1.weight",           # the cut in the middle of stage 2, a fused MLP
                  patch1="patch_embed1.proj.weight",       # every block is input-gradient only: the plain gemm_nt stands in for the fused C x C launch of stages 1-2
                  fc2s3="block3.0.mlp.fc2.weight",         # the cut in a stage-3 block (separate MLP GEMMs) that ends after fc2's weight gradient
                  pos3="pos_embed3")                       # the cut in an embedding unit with a position embedding the only trainable tensor
    for p in m.parameters():
        p.requires_grad_(setting not in single)
    if setting in single:
        dict(m.named_parameters())[single[setting]].requires_grad_(True)
        return
    frozen = dict(all=(), heads=stage_prefixes(1, 2, 3, 4) + ("text_embeddings.",), text=("text_embeddings.",),
                  lower=stage_prefixes(1, 2) + ("text_embeddings.",))[setting]
    for n, p in m.named_parameters():
        if frozen and n.startswith(frozen):
            p.requires_grad_(False)


def _model(dtype, lt=LT, seed=8):
    from mvlt_amd import pvlt
    cfg = O.Cfg("pvlt_tiny", lt, 224, 768, T, 0.0)
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=lt, pretrained_pth=None, drop_path_rate=0.0, compute_dtype=dtype)
    m.load_state_dict(O.filled_state_dict(cfg, seed), strict=True)
    m.cuda().train()
    m.injected_masks = dict(bert=torch.ones(B, T, 768), droppath=[torch.ones(B)] * 8, droppath2=[torch.ones(B)] * 8)
    return m


def _batch(seed=8):
    return {k: v.to(DEV) for k, v in O.to_torch_batch(filler.make_batch(seed, B, IMG, T)).items()}


def _backward(m, seed=8):
    from mvlt_amd.engine import compute_losses
    b = _batch(seed)
    out = m(b["image"], b["input_ids"], mlm_labels=b["mlm_labels"]) if m.loss_type["mlm"] else m(b["image"], b["input_ids"])
    total, _ = compute_losses(out, b["image"], b["mlm_labels"], b["itm_labels"], b["sup_cls_labels"], b["sub_cls_labels"])
    for p in m.parameters():
        p.grad = None
    total.backward()
    torch.cuda.synchronize()
    return total.detach().clone()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def maxrel(a, b):            # tests/test_kernels_gpu.py's metric
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------------------------ kernel
def _mask_by_vector(n, seed):
    """all-frozen, frozen-free and mixed 4-element vectors in a fixed random order; the first vector mixed, the last all frozen"""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 3, (n // 4,), generator=g)
    mask = torch.randint(0, 3, (n // 4, 4), generator=g, dtype=torch.uint8)          # kind 2: whatever the draw gives
    mask[kind == 0] = 2
    free = torch.randint(0, 2, (n // 4, 4), generator=g, dtype=torch.uint8)
    mask[kind == 1] = free[kind == 1]
    mask[0] = torch.tensor([2, 0, 1, 2], dtype=torch.uint8)
    mask[-1] = 2
    v = mask.view(-1, 4)
    allf, nonef = (v == 2).all(1), (v != 2).all(1)
    assert int(allf.sum()) > 10 and int(nonef.sum()) > 10 and int((~allf & ~nonef).sum()) > 10
    return mask.reshape(-1).to(DEV)


def _frozen_step(n, mask, with_p16, clip, seed=21):
    """one step with `mask` on poisoned frozen elements, and the same entry on copies whose 2s are 0 and whose g is finite there"""
    from mvlt_amd import ops
    g_ = torch.Generator().manual_seed(seed)
    p, gr, m = (torch.randn(n, generator=g_).to(DEV) for _ in range(3))
    v = torch.rand(n, generator=g_).to(DEV) * 1e-4
    gr, m = gr * 1e-2, m * 1e-2
    fz = mask == 2
    p[fz], m[fz], v[fz] = 7.25, -3.5, 11.0
    p16 = torch.full((n,), -1.5, dtype=torch.bfloat16, device=DEV) if with_p16 else None
    hp = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05, 1 - 0.9 ** 3, 1 - 0.999 ** 3, 0.5], dtype=torch.float32, device=DEV)
    cd = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=DEV)
    before = (p.clone(), m.clone(), v.clone(), None if p16 is None else p16.clone())
    pb, mb, vb, p16b = p.clone(), m.clone(), v.clone(), (None if p16 is None else p16.clone())
    g_bad = gr.clone()
    g_bad[fz] = float("nan")
    ops.adamw_step(p, g_bad, m, v, p16, n, hp, mask, gscale_dev=cd)
    ops.adamw_step(pb, gr, mb, vb, p16b, n, hp, torch.where(fz, torch.zeros_like(mask), mask), gscale_dev=cd)
    torch.cuda.synchronize()
    for got, old, ref in zip((p, m, v, p16), before, (pb, mb, vb, p16b)):
        if got is None:
            continue
        assert torch.equal(got[fz], old[fz]), "a frozen element was written"
        assert torch.equal(got[~fz], ref[~fz]), "a stepped element differs from the run without frozen bytes"
        assert not torch.equal(got[~fz], old[~fz])


@pytest.mark.parametrize("with_p16,clip", [(True, None), (False, None), (True, 0.37)])
def test_kernel_mixed_masks(with_p16, clip):
    n = 4 * (256 * 2 + 3)                                  # as tests/test_clip_gpu.py::_adamw: more than one workgroup, a ragged last one
    _frozen_step(n, _mask_by_vector(n, 5), with_p16, clip)


def test_kernel_frozen_run_across_the_grid_stride_boundary():
    trip = 8192 * NT * 4                                   # elements one trip of the grid-stride loop covers (the launch has at most 8192 workgroups)
    n = trip + 4 * (NT * 3 + 1)
    mask = (torch.arange(n, device=DEV) % 3 != 0).to(torch.uint8)
    mask[trip - 1030:trip + 1030] = 2                      # starts and ends off the vectors
    mask[5:9] = 2
    _frozen_step(n, mask, True, None)


def test_kernel_masks_without_frozen_bytes_match_torch():
    """what tests/test_kernels_gpu.py::test_adamw_matches_torch demands (max-norm relative 1e-6 after three steps), here through masks of 0s and 1s"""
    from mvlt_amd import ops
    n = 4096 + 8
    gen = torch.Generator().manual_seed(3)
    p0, g = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
    for wd_on in (0, 1):
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        p16 = torch.empty(n, device=DEV, dtype=torch.bfloat16)
        ref_p = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([ref_p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01 * wd_on)
        mask = torch.full((n,), wd_on, dtype=torch.uint8, device=DEV)
        for t in range(1, 4):
            ref_p.grad = g.clone()
            opt.step()
            hp = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9 ** t, 1 - 0.999 ** t, 1.0], device=DEV)
            ops.adamw_step(p, g, m, v, p16, n, hp, mask)
        assert maxrel(p, ref_p.detach()) < 1e-6
        assert torch.equal(p16, p.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------------------------ optimizer
def _frozen_state(m, opt):
    S = m.store
    out = {}
    for name, p in S.params.items():
        if not p.requires_grad:
            off, n, _ = S.offsets[name]
            out[name] = (p.detach().clone(), None if S.C is None else S.C[off:off + n].clone(),
                         None if opt._m is None else (opt._m[off:off + n].clone(), opt._v[off:off + n].clone()))
    return out


def _torch_twin(m, lr, wd):
    """torch.optim.AdamW over clones of the trainable parameters, timm's split"""
    named = [(n, torch.nn.Parameter(p.detach().clone())) for n, p in m.store.params.items() if p.requires_grad]
    return dict(named), torch.optim.AdamW(O.adamw_param_groups(named, wd), lr=lr, betas=(0.9, 0.999), eps=1e-8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_leaves_frozen_parameters_alone(parity, dtype):
    from mvlt_amd.optim import FusedAdamW
    m = _model(dtype)
    apply_setting(m, "lower")
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    _backward(m)                                           # (materialises the store; the twin starts from the same values)
    S = m.store
    opt._ensure()
    twin, topt = _torch_twin(m, 1e-3, 0.05)
    start = {n: q.detach().clone() for n, q in twin.items()}
    frozen0 = _frozen_state(m, opt)
    assert len(frozen0) > 60
    for it in range(2):
        if it:
            _backward(m, seed=9)
        for n, q in twin.items():
            q.grad = S.params[n].grad.detach().clone()
        opt.step()
        topt.step()
    torch.cuda.synchronize()
    for name, (p0, c0, mv0) in frozen0.items():
        off, n, _ = S.offsets[name]
        assert S.params[name].grad is None, name
        assert torch.equal(S.params[name].detach(), p0), name
        assert c0 is None or torch.equal(S.C[off:off + n], c0), name
        assert torch.equal(opt._m[off:off + n], mv0[0]) and torch.equal(opt._v[off:off + n], mv0[1]), name
    worst = max(maxrel(S.params[n].detach(), q.detach()) for n, q in twin.items())
    print(f"{dtype}: trainable parameters against torch.optim.AdamW, worst max-norm relative error {worst:.3e}")
    assert parity("freeze-step/trainable-vs-torch", worst, 1e-6)              # the bound of test_adamw_matches_torch
    assert all(not torch.equal(S.params[n].detach(), start[n]) for n in twin)           # ... and they did move


def test_freeze_then_unfreeze_on_one_optimizer():
    from mvlt_amd.optim import FusedAdamW
    m = _model(torch.float32)
    apply_setting(m, "lower")
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    _backward(m)
    S = m.store
    was_frozen = [n for n, p in S.params.items() if not p.requires_grad]
    p0 = {n: S.params[n].detach().clone() for n in was_frozen}
    opt.step()
    assert all(torch.equal(S.params[n].detach(), p0[n]) for n in was_frozen)
    apply_setting(m, "all")
    _backward(m, seed=9)
    assert all(S.params[n].grad is not None for n in was_frozen)
    grads = {n: S.params[n].grad.detach().clone() for n in was_frozen}
    opt.step()
    torch.cuda.synchronize()
    moved = [n for n in was_frozen if not torch.equal(S.params[n].detach(), p0[n])]
    assert len(moved) == len(was_frozen), sorted(set(was_frozen) - set(moved))[:5]
    # their moments started from zero: what a fresh torch.optim.AdamW holds after one step on the same gradients (the optimizer's step counter, and with
    # it the bias correction, is global: the parameters themselves take the second step of the run, docs/freeze.md)
    fresh = {n: torch.nn.Parameter(p0[n].clone()) for n in was_frozen}
    topt = torch.optim.AdamW(O.adamw_param_groups(list(fresh.items()), 0.05), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for n, q in fresh.items():
        q.grad = grads[n]
    topt.step()
    # Bounds from the number formats: from zero, m = (1 - b1) g and v = (1 - b2) g^2.  The kernel forms 1 - beta in fp32 from fp32(beta), torch rounds the
    # double 1 - beta once: fp32(beta) is off by at most 2^-25 (half an ulp below 1), i.e. 2^-25 / (1 - beta) relative to the factor -- 3.0e-7 for
    # b1 = 0.9, 3.0e-5 for b2 = 0.999 -- plus three roundings of 2^-24 for the products.
    tol_m, tol_v = 2 ** -25 / 0.1 + 3 * 2 ** -24, 2 ** -25 / 0.001 + 3 * 2 ** -24
    for n, q in fresh.items():
        off, cnt, shape = S.offsets[n]
        st = topt.state[q]
        assert maxrel(opt._m[off:off + cnt].view(shape), st["exp_avg"]) < tol_m, n
        assert maxrel(opt._v[off:off + cnt].view(shape), st["exp_avg_sq"]) < tol_v, n
    # ... and the parameters took the documented step: moments from zero, the bias correction of the optimizer's step 2, in closed form (float64).  The
    # bound is test_adamw_matches_torch's 1e-6 (max-norm, relative to the parameter) -- the update itself is ~lr = 1e-3 of that scale, so it admits a
    # relative error of 1e-3 in the update, far above the 3e-5 of the fp32 1 - beta2 derived above.
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 0.05
    for n in was_frozen:
        g, p = grads[n].double(), p0[n].double()
        decay = 0.0 if (p.dim() == 1 or n.endswith(".bias")) else wd
        mm, vv = (1 - b1) * g, (1 - b2) * g * g
        want = p * (1 - lr * decay) - (lr / (1 - b1 ** 2)) * mm / (vv.sqrt() / (1 - b2 ** 2) ** 0.5 + eps)
        assert maxrel(S.params[n].detach(), want) < 1e-6, n


# ------------------------------------------------------------------------------------------------------------------ backward
_REF = {}


def _reference(dtype, lt=LT):
    """the all-trainable backward on the shared batch, twice (the second run gives the run-to-run spread); computed once per dtype, never changed"""
    key = (dtype, tuple(sorted(lt.items())))
    if key not in _REF:
        m = _model(dtype, lt)
        loss = _backward(m)
        g1 = {n: p.grad.detach().clone() for n, p in m.store.params.items()}
        _backward(m)
        g2 = {n: p.grad.detach().clone() for n, p in m.store.params.items()}
        _REF[key] = (loss, g1, {n: _rel(g2[n], g1[n]) for n in g1})
    return _REF[key]


LT_MIM = dict(mlm=1, itm=1, t2i=1, cls=0)


@pytest.mark.parametrize("setting", ["heads", "text", "lower", "one", "patch1", "fc2s3", "pos3", "heads+mim"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_trainable_gradients_equal_the_unfrozen_run(parity, dtype, setting):
    lt = LT
    if setting == "heads+mim":                             # the MIM decoder on a frozen trunk: parameter gradients only, no gradient for the stage outputs
        lt, setting = LT_MIM, "heads"
    loss_ref, g_ref, spread = _reference(dtype, lt)
    m = _model(dtype, lt)
    apply_setting(m, setting)
    loss = _backward(m)
    assert torch.equal(loss, loss_ref), (float(loss), float(loss_ref))              # the forward does not change
    bar = 1e-3 if dtype == torch.float32 else 2e-2                                     # the project's bars: relative L2, fp32 / bf16 path
    tag = ("fp32" if dtype == torch.float32 else "bf16") + ("-mim" if lt is LT_MIM else "")
    bad, n_live = {}, 0
    for n, p in m.store.params.items():
        if not p.requires_grad:
            assert p.grad is None, n
            continue
        n_live += 1
        assert p.grad is not None, n
        e = _rel(p.grad, g_ref[n])
        parity(f"freeze-{setting}-{tag}/run-to-run/{n}", spread[n], bar)               # the all-trainable run against itself: recorded beside it, not gated
        if not parity(f"freeze-{setting}-{tag}/grad/{n}", e, bar):
            bad[n] = (e, spread[n])
    assert n_live == dict(one=1, patch1=1, fc2s3=1, pos3=1).get(setting, n_live) and n_live > 0
    assert not bad, (len(bad), sorted(bad.items(), key=lambda kv: -kv[1][0])[:8])


@contextlib.contextmanager
def _counting(m):
    """counting closures around the weight-gradient / attention-backward / embedding-backward entries for the duration of a backward"""
    from mvlt_amd import layers, ops, trunk
    S = m.store
    calls = dict(gemm_tn=0, mlp_bwd_dw=0, sr_attention_bwd=0, bert_embed_bwd=0, conv_wgrad=0)
    in_trunk = [0]
    frozen_targets = []
    g_lo, g_hi = S.G.data_ptr(), S.G.data_ptr() + 4 * S.total

    def wholly_frozen(lo, hi):
        """[lo, hi): byte range inside G -> every parameter it touches is frozen"""
        hit = [p.requires_grad for name, p in S.params.items()
               if g_lo + 4 * S.offsets[name][0] < hi and lo < g_lo + 4 * (S.offsets[name][0] + S.offsets[name][1])]
        return bool(hit) and not any(hit)

    saved = {k: getattr(ops, k) for k in ("gemm_tn", "mlp_bwd_dw", "sr_attention_bwd", "bert_embed_bwd")}
    saved_cw, saved_bw = layers.conv_wgrad, trunk.TrunkStep.backward

    def wrap(key, fn):
        def f(*a, **k):
            if in_trunk[0]:
                calls[key] += 1
            if key == "gemm_tn":
                c = a[2]
                if g_lo <= c.data_ptr() < g_hi and wholly_frozen(c.data_ptr(), c.data_ptr() + 4 * c.numel()):
                    frozen_targets.append(("gemm_tn", tuple(c.shape)))
            return fn(*a, **k)
        return f

    def cw(S_, name, *a, **k):
        if in_trunk[0]:
            calls["conv_wgrad"] += 1
        if not S_.params[name].requires_grad:               # (the arena slot stands for the weight's G slice)
            frozen_targets.append(("conv_wgrad", name))
        return saved_cw(S_, name, *a, **k)

    def bw(self, dxs):
        in_trunk[0] += 1
        try:
            return saved_bw(self, dxs)
        finally:
            in_trunk[0] -= 1

    for k, fn in saved.items():
        setattr(ops, k, wrap(k, fn))
    layers.conv_wgrad, trunk.TrunkStep.backward = cw, bw
    try:
        yield calls, frozen_targets
    finally:
        for k, fn in saved.items():
            setattr(ops, k, fn)
        layers.conv_wgrad, trunk.TrunkStep.backward = saved_cw, saved_bw


@pytest.mark.parametrize("setting", ["all", "heads", "text", "lower", "one", "patch1", "fc2s3", "pos3"])
def test_pruning_really_happens(setting):
    m = _model(torch.bfloat16)
    apply_setting(m, setting)
    _backward(m)                                           # materialise the store (the counters need its addresses)
    with _counting(m) as (calls, frozen_targets):
        _backward(m)
    print(setting, calls, frozen_targets)
    assert not frozen_targets, frozen_targets              # no weight-gradient launch aims at a G slice that lies wholly inside frozen parameters
    d = m.depths
    if setting == "all":
        assert calls["sr_attention_bwd"] == sum(d) and calls["bert_embed_bwd"] == 1 and calls["mlp_bwd_dw"] == d[0] + d[1] and calls["conv_wgrad"] == 3 + d[0] + d[1] + d[2]
    if setting == "heads":
        assert not any(calls.values()), calls
        b = _batch()
        assert torch.is_grad_enabled()
        img_feats, text_feats = m.forward_pyramid_features_vl(b["image"], b["input_ids"])
        assert len(img_feats) == 4 and not any(t.requires_grad for t in img_feats + text_feats)
    if setting == "text":
        assert calls["bert_embed_bwd"] == 0 and calls["sr_attention_bwd"] == sum(d)
    if setting == "lower":
        assert calls["sr_attention_bwd"] == d[2] + d[3] and calls["bert_embed_bwd"] == 0 and calls["mlp_bwd_dw"] == 0
    if setting == "one":
        assert calls["sr_attention_bwd"] == d[2] + d[3] and calls["mlp_bwd_dw"] == 1 and calls["gemm_tn"] == 0 and calls["conv_wgrad"] == 0 and calls["bert_embed_bwd"] == 0
    if setting == "patch1":
        # every block runs for its input gradient alone: no weight-gradient launch in any of them (the fused C x C launch of stages 1-2 is a gemm_tn: it is gone
        # too), the one gemm_tn of the trunk is patch_embed1's
        assert calls == dict(gemm_tn=1, mlp_bwd_dw=0, sr_attention_bwd=sum(d), bert_embed_bwd=0, conv_wgrad=0), calls
    if setting == "fc2s3":
        # stage 4 and block3.1 input-gradient only; block3.0 ends after fc2's weight gradient, before its attention
        assert calls == dict(gemm_tn=1, mlp_bwd_dw=0, sr_attention_bwd=d[3] + d[2] - 1, bert_embed_bwd=0, conv_wgrad=0), calls
    if setting == "pos3":
        assert calls == dict(gemm_tn=0, mlp_bwd_dw=0, sr_attention_bwd=d[3] + d[2], bert_embed_bwd=0, conv_wgrad=0), calls


# ------------------------------------------------------------------------------------------------------------------ engine loop
class _Loader:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_engine_loop_in_the_fine_tune_shape(parity, dtype):
    """CLS heads on a frozen trunk: FusedAdamW + BF16Scaler with a clip that bites against the same loop on stock torch.optim.AdamW + clip_grad_norm_.
    Bounds: tests/test_engine_gpu.py's for its loop (_check_deltas: each tensor's delta norm within 2e-2 fp32 / 0.25 bf16, its values within twice that)."""
    from mvlt_amd.engine import BF16Scaler, train_one_epoch_vl
    from mvlt_amd.optim import FusedAdamW
    batches = [O.to_torch_batch(filler.make_batch(40 + it, B, IMG, T)) for it in range(4)]
    args = types.SimpleNamespace(loss_type=LT_CLS)
    dev = torch.device(DEV)
    max_norm, lr, wd = 1e-3, 1e-4, 0.05
    runs = {}
    for kind in ("fused", "torch"):
        m = _model(dtype, LT_CLS)
        apply_setting(m, "heads")
        p0 = {n: p.detach().clone() for n, p in m.named_parameters()}
        live = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        opt = FusedAdamW(m, lr=lr, weight_decay=wd) if kind == "fused" else \
            torch.optim.AdamW(O.adamw_param_groups(live, wd), lr=lr, betas=(0.9, 0.999), eps=1e-8)
        scaler = BF16Scaler()
        res = train_one_epoch_vl(m, None, _Loader(batches), opt, dev, 0, scaler, max_norm, None, None, True, False, args)
        torch.cuda.synchronize()
        assert all(v == v and abs(v) != float("inf") for v in res.values()), res
        now = dict(m.named_parameters())
        for n, p in p0.items():
            if not now[n].requires_grad:
                assert torch.equal(now[n].detach(), p), (kind, n)
                assert now[n].grad is None
        runs[kind] = {n: (now[n].detach() - p0[n]).double() for n, _ in live}
        if kind == "fused":
            norm = float(scaler.last_grad_norm)
            ref = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.double()) for _, p in live])))
            print(f"{dtype}: clip norm {norm:.9e} torch over the trainable gradients {ref:.9e}")
            assert norm > max_norm                                               # the clip bites
            assert parity("freeze-engine/clip-norm", abs(norm - ref) / ref, 1e-5)
    tol = 2e-2 if dtype == torch.float32 else 0.25
    bad = {}
    for n, d in runs["fused"].items():
        r = runs["torch"][n]
        en = abs(float(d.norm()) - float(r.norm())) / float(r.norm())
        es = float((d - r).norm() / r.norm())
        if not (parity(f"freeze-engine-delta-norm/{n}", en, tol) & parity(f"freeze-engine-delta/{n}", es, 2 * tol)):
            bad[n] = (en, es)
    assert len(runs["fused"]) >= 12 and not bad, bad


# ------------------------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_batch(rank):
    b = O.to_torch_batch(filler.make_batch(70 + rank, B, IMG, T))
    return {k: v.cuda() for k, v in b.items()}


def _rank_grads(model, batch):
    from mvlt_amd.engine import train_step
    total, _ = train_step(model, batch, 0, False)
    for p in model.parameters():
        p.grad = None
    total.backward()
    torch.cuda.synchronize()


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mvlt_amd.dist import DataParallel
        from mvlt_amd.optim import FusedAdamW
        core = _model(torch.float32, seed=9 + rank)           # different start weights: the wrapper broadcasts rank 0's
        apply_setting(core, "lower")
        model = DataParallel(core)
        opt = FusedAdamW(core, lr=1e-3, weight_decay=0.05)
        _rank_grads(model, _rank_batch(rank))
        S = core.store
        S.sync_grads()
        assert S.pending_grad_scale == 1.0
        live = torch.zeros(S.total, dtype=torch.bool, device=S.G.device)
        for n, p in S.params.items():
            if p.requires_grad:
                live[S.offsets[n][0]:S.offsets[n][0] + S.offsets[n][1]] = True
        g_mine = S.G[live].clone()
        opt.step()
        torch.cuda.synchronize()
        ref = _model(torch.float32, seed=9)
        apply_setting(ref, "lower")
        gs = []
        for r in range(world):
            _rank_grads(ref, _rank_batch(r))
            gs.append(ref.store.G[live].clone())
        gmean = sum(gs) / world
        e_g = _rel(g_mine, gmean)
        p_init = ref.store.P
        frozen_same = bool(torch.equal(S.P[~live], p_init[~live]))
        moved = bool(not torch.equal(S.P[live], p_init[live]))
        none_grads = all(p.grad is None for p in core.parameters() if not p.requires_grad)
        q.put(dict(rank=rank, e_g=e_g, frozen_same=frozen_same, moved=moved, none_grads=none_grads,
                   p_sha=hashlib.sha256(S.P.cpu().numpy().tobytes()).hexdigest()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_frozen_lower_stages(parity):
    """the pattern of tests/test_dist_gpu.py: two processes on the one GPU, gloo; its bound on the gradients (1e-5 relative L2 against the mean of the
    single-rank gradients)"""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(world)), key=lambda d: d["rank"])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in res:
        assert parity(f"freeze-dp/grad-rank{r['rank']}", r["e_g"], 1e-5), r
        assert r["frozen_same"] and r["moved"] and r["none_grads"], r
    assert res[0]["p_sha"] == res[1]["p_sha"]               # both ranks hold identical parameters after the step

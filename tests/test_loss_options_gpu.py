"""GPU, model level: `set_loss_options` (docs/loss_options.md) on PVT-tiny at batch 2, 128 px, T = 20, in fp32 and in bf16.  The smoothed MLM loss that
_MLMFusedFn forms inside its node against the unfused route (full logits, F.cross_entropy(label_smoothing=) by ATen, backward through the same model); the CLS
losses with smoothing and class weights against F.cross_entropy on the returned logits; options switched on and off again against a model that never had any;
and the argument checks."""
import pytest
import torch
import torch.nn.functional as F

from oracle import filler
from oracle import pvlt_oracle as O
from tests import rowwise_cases as rc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
B, IMG, T = 2, 128, 20
LT_MLM = dict(mlm=1, itm=0, t2i=0, cls=0)
LT_CLS = dict(mlm=0, itm=0, t2i=0, cls=1)
DT_ID = {torch.float32: "fp32", torch.bfloat16: "bf16"}
DTYPES = [torch.float32, torch.bfloat16]


def _model(dtype, lt, seed=8):
    from mvlt_amd import pvlt
    cfg = O.Cfg("pvlt_tiny", lt, 224, 768, T, 0.0)
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=lt, pretrained_pth=None, drop_path_rate=0.0, compute_dtype=dtype)
    m.load_state_dict(O.filled_state_dict(cfg, seed), strict=True)
    m.cuda().train()
    m.injected_masks = dict(bert=torch.ones(B, T, 768), droppath=[torch.ones(B)] * 8, droppath2=[torch.ones(B)] * 8)        # no dropout: the two routes see one model
    return m


def _batch(seed=8):
    return {k: v.to(DEV) for k, v in O.to_torch_batch(filler.make_batch(seed, B, IMG, T)).items()}


def _grads(m, loss):
    for p in m.parameters():
        p.grad = None
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _compare_routes(m, b, e, dtype, parity):
    """fused step under mlm_label_smoothing = e against full logits + ATen's loss; -> the two MLM losses"""
    from mvlt_amd.engine import train_step
    tag = f"{DT_ID[dtype]} e={e}"
    m.set_loss_options(mlm_label_smoothing=e)
    total, parts = train_step(m, b, 0, False)
    assert m._plan is not None
    fused_loss = parts["loss_mlm"].detach().clone()
    fused = _grads(m, total)                                                   # MLM is the only head: total = 1 x loss_mlm
    out = m(b["image"], b["input_ids"])                                        # the unfused route: (B, T, 30522) logits
    want = F.cross_entropy(out["mlm_logits"].reshape(-1, 30522).float(), b["mlm_labels"].view(-1), ignore_index=-1, label_smoothing=e)
    unfused = _grads(m, want)
    bar = rc.TOL[dtype]
    want = want.detach()
    err = abs(float(fused_loss) - float(want)) / abs(float(want))
    print(f"{tag}: loss_mlm fused {float(fused_loss)!r}, unfused {float(want)!r}, relative difference {err:.3e}")
    assert parity(f"loss_mlm {tag}", err, bar), (tag, float(fused_loss), float(want))
    assert set(fused) == set(unfused)
    worst = ("", 0.0)
    for n, g in unfused.items():
        if float(g.norm()) == 0.0:
            assert float(fused[n].norm()) == 0.0, n
            continue
        r = _rel(fused[n], g)
        worst = max(worst, (n, r), key=lambda t: t[1])
        assert parity(f"grad {tag}/{n}", r, bar), (tag, n, r)
    print(f"{tag}: {len(unfused)} gradient tensors, worst relative L2 {worst[1]:.3e} ({worst[0]})")
    # the fallback below the device path (full logits through engine.cross_entropy) takes the option too
    _, parts_u = train_step(m, b, 0, False, fused=False)
    assert abs(float(parts_u["loss_mlm"]) - float(want)) <= rc.TOL[torch.float32] * abs(float(want))
    return float(fused_loss), float(want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_smoothed_mlm_against_the_unfused_route(dtype, parity):
    """with smoothing OFF the two routes meet the parity bars (fp32 1e-3, bf16 2e-2 relative L2 per tensor) -- so a failure with smoothing ON is the new code's"""
    m, b = _model(dtype, LT_MLM), _batch()
    _, want_plain = _compare_routes(m, b, 0.0, dtype, parity)
    smoothed, want_smoothed = _compare_routes(m, b, 0.1, dtype, parity)
    assert abs(smoothed - want_smoothed) < 0.1 * abs(smoothed - want_plain)     # the option did something: the fused loss follows the smoothed reference


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_cls_options_against_torch(dtype, parity):
    from mvlt_amd.engine import compute_losses, train_step
    m, b = _model(dtype, LT_CLS), _batch()
    g = rc.gen(11)
    w_sup, w_sub = 0.25 + 2 * torch.rand(48, generator=g), 0.25 + 2 * torch.rand(122, generator=g)
    opts = m.set_loss_options(cls_label_smoothing=0.1, sup_cls_weight=w_sup, sub_cls_weight=w_sub.tolist())
    assert opts is m.loss_options and opts.active and opts.sup_cls_weight.is_cuda and opts.sub_cls_weight.dtype == torch.float32
    assert not any("cls_weight" in k for k in m.state_dict()) and not any("cls_weight" in n for n, _ in m.named_buffers())
    out = m(b["image"], b["input_ids"])
    labels = dict(sup=b["sup_cls_labels"].view(-1), sub=b["sub_cls_labels"].view(-1))
    total, parts = compute_losses(out, b["image"], b["mlm_labels"], b["itm_labels"], b["sup_cls_labels"], b["sub_cls_labels"], options=m.loss_options)
    logits = dict(sup=out["sup_cls_logits"], sub=out["sub_cls_logits"])
    got_g = torch.autograd.grad(total, [logits["sup"], logits["sub"]], retain_graph=True)
    for (k, n, w), gg in zip((("sup", 48, w_sup), ("sub", 122, w_sub)), got_g):
        x = logits[k].detach().view(-1, n).double().requires_grad_(True)
        want = F.cross_entropy(x, labels[k], weight=w.double().to(DEV), label_smoothing=0.1)
        want.backward()
        plain = F.cross_entropy(x.detach(), labels[k])
        got = parts[f"loss_{k}_cls"].detach()
        t = rc.TOL[torch.float32]                                              # the loss reads fp32 logits whatever the trunk computes in
        print(f"{DT_ID[dtype]} {k}: loss {float(got)!r}, torch {float(want)!r} (plain {float(plain)!r})")
        assert parity(f"loss_{k}_cls {DT_ID[dtype]}", abs(float(got) - float(want)), t * max(1.0, abs(float(want))))
        assert abs(float(want) - float(plain)) > 10 * t                        # ... and is not the plain loss
        den = float(w.to(DEV)[labels[k]].sum())
        err = (gg.view(-1, n).double() - x.grad).abs()
        bar = rc.bar_dlogits(x.grad, t, 1.0, den, torch.float32)
        assert parity(f"dlogits {k} {DT_ID[dtype]}", float((err / bar).max()), 1.0)
    # train_step hands the model's options over by itself: the same two numbers
    _, parts_t = train_step(m, b, 0, False)
    assert torch.equal(parts_t["loss_sup_cls"], parts["loss_sup_cls"]) and torch.equal(parts_t["loss_sub_cls"], parts["loss_sub_cls"])


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("lt", [LT_MLM, LT_CLS], ids=["mlm", "cls"])
def test_off_is_off(dtype, lt, monkeypatch):
    """options on, a step, options back to their defaults: the next step is the step of a model that never had options set.  Bit for bit: the six losses and
    the gradient every loss node hands to the rest of the backward (dlogits of the plain kernels), and no kernel of csrc/loss.hip is launched.  The flat
    gradient buffer behind them is NOT bit-reproducible in this project -- the weight-gradient and embedding kernels add with fp32 atomics, so two backward
    passes of ONE untouched model differ in their last bits (measured here: 2.1 M of 37.9 M elements in fp32, ~10 k in bf16; tests/test_lamb_gpu.py and
    tests/test_param_groups_gpu.py note the same) -- so the buffer is held to the parity bar against the untouched model, and both counts are printed."""
    from mvlt_amd import ops
    from mvlt_amd.engine import train_step
    b = _batch()
    plain_bwd = ops.cross_entropy_bwd
    handed = []

    def recording_bwd(logits, labels, lse, gscale, count, dlogits, *a, **k):
        plain_bwd(logits, labels, lse, gscale, count, dlogits, *a, **k)
        handed.append(dlogits.clone())

    monkeypatch.setattr(ops, "cross_entropy_bwd", recording_bwd)

    def step(m):
        del handed[:]
        total, parts = train_step(m, b, 0, False)
        for p in m.parameters():
            p.grad = None
        total.backward()
        torch.cuda.synchronize()
        return total._packed.detach().clone(), m.store.G.clone(), list(handed)

    twin = _model(dtype, lt)
    loss_a, g_a, dl_a = step(twin)
    loss_a2, g_a2, dl_a2 = step(twin)
    assert len(dl_a) == (1 if lt is LT_MLM else 2)
    m = _model(dtype, lt)
    if lt is LT_MLM:
        m.set_loss_options(mlm_label_smoothing=0.1)
    else:
        m.set_loss_options(cls_label_smoothing=0.2, sup_cls_weight=torch.full((48,), 2.0), sub_cls_weight=torch.full((122,), 0.5))
    loss_on, _, dl_on = step(m)
    assert not torch.equal(loss_on, loss_a) and not dl_on                       # the options were on: no plain loss backward ran
    m.set_loss_options()
    assert not m.loss_options.active
    calls = []
    monkeypatch.setattr(ops, "ce_smooth_fwd", lambda *a, **k: calls.append("fwd"))
    monkeypatch.setattr(ops, "ce_smooth_bwd", lambda *a, **k: calls.append("bwd"))
    loss_b, g_b, dl_b = step(m)
    assert not calls
    assert torch.equal(_bits(loss_b), _bits(loss_a)) and torch.equal(_bits(loss_a2), _bits(loss_a))
    assert len(dl_b) == len(dl_a) and all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(dl_a, dl_b, dl_a2))
    own, reset = _rel(g_a2, g_a), _rel(g_b, g_a)
    print(f"{DT_ID[dtype]}: gradient elements that differ between the untouched model's own two passes: {int((_bits(g_a) != _bits(g_a2)).sum())} "
          f"(relative L2 {own:.3e}); between it and the model whose options were reset: {int((_bits(g_a) != _bits(g_b)).sum())} of {g_a.numel()} "
          f"(relative L2 {reset:.3e})")
    assert reset <= rc.TOL[dtype], (reset, own)


def test_set_loss_options_validates():
    from mvlt_amd import pvlt
    from mvlt_amd._lib import MVLTError
    m = _model(torch.bfloat16, dict(mlm=1, itm=0, t2i=0, cls=1))
    for kw in (dict(mlm_label_smoothing=1.0), dict(mlm_label_smoothing=-0.1), dict(cls_label_smoothing=1.5), dict(cls_label_smoothing=float("nan"))):
        with pytest.raises(MVLTError, match=r"must be in \[0, 1\)"):
            m.set_loss_options(**kw)
    for kw in (dict(sup_cls_weight=torch.ones(47)), dict(sup_cls_weight=torch.ones(122)), dict(sub_cls_weight=torch.ones(48)), dict(sub_cls_weight=torch.ones(1, 122))):
        with pytest.raises(MVLTError, match="entries"):
            m.set_loss_options(**kw)
    bad = torch.ones(48)
    for v in (0.0, -1.0, float("inf"), float("nan")):
        bad[7] = v
        with pytest.raises(MVLTError, match="positive and finite"):
            m.set_loss_options(sup_cls_weight=bad)
    assert not m.loss_options.active                                           # a refused call changes nothing
    m.set_loss_options(mlm_label_smoothing=0.1, sub_cls_weight=torch.ones(122))
    assert m.loss_options.active and m.loss_options.sup_cls_weight is None
    m.set_loss_options()
    assert not m.loss_options.active and isinstance(m.loss_options, pvlt.LossOptions)
    # weights given before the model moves follow it to the device
    early = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT_CLS, pretrained_pth=None)
    early.set_loss_options(sup_cls_weight=torch.full((48,), 3.0))
    assert not early.loss_options.sup_cls_weight.is_cuda
    early.cuda()
    w = early.loss_options.sup_cls_weight
    assert w.is_cuda and w.dtype == torch.float32 and bool((w == 3.0).all())
    no_cls = _model(torch.bfloat16, LT_MLM)
    with pytest.raises(MVLTError, match="no CLS heads"):
        no_cls.set_loss_options(cls_label_smoothing=0.1)
    no_mlm = _model(torch.bfloat16, LT_CLS)
    with pytest.raises(MVLTError, match="no MLM head"):
        no_mlm.set_loss_options(mlm_label_smoothing=0.1)

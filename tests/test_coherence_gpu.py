"""GPU: every writer of the parameters in front of every copy the forward reads (docs/coherence.md has the writer x copy table).

The forward never reads a Parameter: it reads the bf16 copy C, the W^T / conv-layout copies of FlatStore.extra and the BatchNorm folds of the eval-mode MIM
decoder, and FlatStore.refresh() decides from version counters and three flags whether they are current.  Each case here runs one writer AFTER an earlier
forward (the copies exist and are current), then an eval forward, and hands the model to two judges:

  audit               tests/coherence_cases.py: every copy against its definition from the fp32 masters and the buffers, bit for bit
  the fresh model     a model built from state_dict() of the written one must give the same outputs -- bit for bit for every output the premise test
                      (two fresh models agree) holds that way, else by err_metric / TOL of tests/test_model_gpu.py (BY_TOLERANCE: none today)

and carries a control: the outputs the case names must have moved by at least 10x that tolerance between the forward before the write and the one after.
pvlt_tiny at 64 x 64 pixels (stage grids 16 / 8 / 4 / 2), T = 16, B = 2, all four losses on: the smallest model that has every kind of copy; every
staleness mechanism is independent of size."""
import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O
from oracle.hostinfo import usable_cores
from tests import coherence_cases as CC
from tests.test_model_gpu import TOL, err_metric

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LT = dict(mlm=1, itm=1, t2i=1, cls=1)
T, B, IMG = 16, 2, 64
DTYPES = [torch.float32, torch.bfloat16]
OUTS = ("mlm_logits", "itm_logits", "sup_cls_logits", "sub_cls_logits", "t2i_logits")
TEXT_OUTS = OUTS[:4]
BY_TOLERANCE = frozenset()          # outputs two fresh models do NOT reproduce bit for bit (test_two_fresh_models_agree_bit_for_bit): compared by TOL instead
FACTOR = -4.0                       # the in-place writes: large and sign-flipping, so that a LayerNorm behind the written tensor does not hide it
LR, LAMB_LR = 2e-2, 0.2             # step sizes of the optimizer cases: every weight moves by a sizeable part of itself in ONE step (the controls need it)
CFG = O.Cfg("pvlt_tiny", LT, 224, 768, T, 0.0)

_SD, _BATCH = {}, {}


def filled(seed):
    if seed not in _SD:
        _SD[seed] = O.filled_state_dict(CFG, seed)
    return _SD[seed]


def batch():
    if not _BATCH:
        _BATCH.update({k: v.to(DEV) for k, v in O.to_torch_batch(filler.make_batch(1, B, IMG, T)).items()})
    return _BATCH


def build(dtype, sd):
    from mvlt_amd import pvlt
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, drop_path_rate=0.0, drop_rate=0.0,
                       num_classes=1000, in_chans=3, compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m.cuda().eval()
    m.injected_masks = dict(bert=torch.ones(B, T, 768), droppath=[torch.ones(B)] * 8, droppath2=[torch.ones(B)] * 8)
    return m


def fresh_of(m, dtype):
    return build(dtype, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})


def forward(m):
    """an eval, no-grad forward with every head -> {output: clone}; the copies are current (or should be) afterwards"""
    was = m.training
    m.eval()
    b = batch()
    with torch.no_grad():
        out = m(b["image"], b["input_ids"])
    torch.cuda.synchronize()
    m.train(was)
    return {k: out[k].detach().float().clone() for k in OUTS}


def distance(a, b, dtype):
    return float(err_metric(a.cpu().numpy(), b.cpu().numpy(), dtype))


def same(parity, tag, got, want, dtype):
    """the second judge's comparison: torch.equal, or TOL for the outputs of BY_TOLERANCE"""
    for k in OUTS:
        assert torch.isfinite(got[k]).all(), (tag, k)
        if k in BY_TOLERANCE:
            assert parity(f"{tag}/{k}", distance(got[k], want[k], dtype), TOL[dtype]), (tag, k)
        else:
            assert torch.equal(got[k], want[k]), (tag, k, distance(got[k], want[k], dtype))


def judge(parity, tag, m, dtype, before, moved=OUTS, unmoved=False):
    """forward of the written model -> audit -> fresh-model comparison -> control against `before`.  moved: the outputs that must differ from `before` by
    10 x TOL; unmoved=True: the writer must have changed NO parameter (a closed gate) -- the four text-side outputs equal `before` bit for bit.  Returns
    the outputs."""
    got = forward(m)
    CC.audit(m)
    same(parity, tag, got, forward(fresh_of(m, dtype)), dtype)
    moves = {k: distance(got[k], before[k], dtype) for k in OUTS}
    print(f"{tag}: moved by " + ", ".join(f"{k} {v:.3g}" for k, v in moves.items()))
    if unmoved:                         # (the MIM output is left out: the train-mode forward of the skipped step has moved the running statistics)
        for k in TEXT_OUTS:
            assert torch.equal(got[k], before[k]), (tag, k)
    else:
        for k in moved:
            assert moves[k] >= 10 * TOL[dtype], (tag, k, moves[k])
    return got


def started(dtype, seed=1):
    """a model that has run a forward: copies exist and are current.  -> (model, its outputs)"""
    m = build(dtype, filled(seed))
    out = forward(m)
    CC.audit(m)
    return m, out


def backward(m):
    """train-mode forward + backward of the full loss on the store's gradient buffer; the model is left in train mode"""
    from mvlt_amd.engine import compute_losses
    m.train()
    b = batch()
    out = m(b["image"], b["input_ids"], mlm_labels=b["mlm_labels"])
    total, _ = compute_losses(out, b["image"], b["mlm_labels"], b["itm_labels"], b["sup_cls_labels"], b["sub_cls_labels"])
    for p in m.parameters():
        p.grad = None
    total.backward()
    return total


def freeze_lower(m):
    """stages 1-2 and the BERT embeddings frozen (the `lower` setting of tests/test_freeze_gpu.py)"""
    pre = tuple(f"block{i}." for i in (1, 2)) + tuple(e.format(i) for i in (1, 2) for e in ("patch_embed{}", "text_embed{}", "pos_embed{}", "text_pos_embed{}"))
    for n, p in m.named_parameters():
        p.requires_grad_(not n.startswith(pre + ("text_embeddings.",)))


# ================================================================================================ premises
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_fresh_models_agree_bit_for_bit(dtype, parity):
    a, b = forward(build(dtype, filled(1))), forward(build(dtype, filled(1)))
    for k in OUTS:
        assert a[k].numel() > 0 and torch.isfinite(a[k]).all(), k
        if k not in BY_TOLERANCE:
            assert torch.equal(a[k], b[k]), (k, distance(a[k], b[k], dtype))
    same(parity, "premise", a, b, dtype)
    c = forward(build(dtype, filled(2)))                   # and the other filler seed is a write the controls can see
    for k in OUTS:
        assert distance(c[k], a[k], dtype) >= 10 * TOL[dtype], (k, distance(c[k], a[k], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_audit_sees_every_kind_of_copy_and_a_planted_stale_one(dtype):
    m, _ = started(dtype)
    S = m.store
    kinds = {k.rsplit("::", 1)[1] for k in S.extra if "::" in k}
    assert kinds == {"T", "K", "KT", "F", "W"} and CC.SCORE + "::T" in S.extra
    assert len(m._mim_fold) == 11 and (S.C is not None) == (dtype == torch.bfloat16)
    assert CC.audit(m) == (len(S.offsets) if S.C is not None else 0) + sum("::" in k for k in S.extra) + 22
    with torch.no_grad():
        S.extra["block3.0.mlp.fc1.weight::T"][5, 7] += 1.0          # planted on the device: the judge works here as on the CPU
    assert CC.first_stale(m) == ("block3.0.mlp.fc1.weight::T", 5 * S.extra["block3.0.mlp.fc1.weight::T"].shape[1] + 7)


# ================================================================================================ writers 1-4, 8, 9: torch-side writes
@pytest.mark.parametrize("dtype", DTYPES)
def test_load_state_dict_sgd_and_the_oracle(dtype, parity):
    """writers 1 and 2 as one sequence, whose last state also meets the CPU oracle"""
    m, out = started(dtype)
    m.load_state_dict(filled(2), strict=True)
    out = judge(parity, "load_state_dict", m, dtype, out)
    # only the BatchNorm buffers: the fold must follow
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = sd[k] + 1.0
        elif k.endswith("running_var"):
            sd[k] = sd[k] * 4.0
    m.load_state_dict(sd, strict=True)
    out = judge(parity, "load_state_dict-buffers", m, dtype, out, moved=("t2i_logits",))
    # a stock optimizer step: every parameter halves (p.grad = p on the store's own gradient views, lr 0.5)
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    backward(m)
    with torch.no_grad():
        for p in m.parameters():
            p.grad.copy_(p)
    opt.step()
    out = judge(parity, "sgd", m, dtype, out)
    torch.set_num_threads(usable_cores())
    b = batch()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.forward(sd, CFG, b["image"].cpu(), b["input_ids"].cpu())
    for k in OUTS:
        assert parity(f"oracle/{k}", err_metric(out[k].cpu().numpy(), ref[k].float().numpy(), dtype), TOL[dtype]), k


IN_PLACE = [         # (parameter, the outputs that must move)
    ("text_embed1.0.weight", TEXT_OUTS),                    # a 2-D weight with a ::T copy (a LayerNorm follows: the sign carries the write)
    ("patch_embed2.proj.weight", ("t2i_logits",)),          # ::K / ::KT
    ("t2i_head.conv4.0.weight", ("t2i_logits",)),           # ::K / ::F and the fold
    (CC.SCORE, ("t2i_logits",)),                            # ::W / ::T of the score conv
    ("text_embeddings.LayerNorm.weight", TEXT_OUTS),        # a 1-D tensor
]


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_writes_one_tensor_at_a_time(dtype, parity):
    """writers 3 and 4: p.mul_() under no_grad bumps the Parameter's counter, writes through the flat buffer bump P's"""
    m, out = started(dtype)
    S = m.store
    params = dict(m.named_parameters())
    for name, moved in IN_PLACE:
        with torch.no_grad():
            params[name].mul_(FACTOR)
        out = judge(parity, f"mul_/{name}", m, dtype, out, moved=moved)
    lo, hi = S.prefix_range(("block4.",))
    with torch.no_grad():
        S.P[lo:hi].mul_(FACTOR)
    out = judge(parity, "P[lo:hi].mul_", m, dtype, out, moved=TEXT_OUTS)
    with torch.no_grad():
        S.master("patch_embed3.proj.weight").mul_(FACTOR)
    judge(parity, "master().mul_", m, dtype, out, moved=("t2i_logits",))


@pytest.mark.parametrize("dtype", DTYPES)
def test_train_forward_alone_and_rematerialisation(dtype, parity):
    """writers 8 and 9: a train-mode forward writes the running statistics through raw pointers; .cpu() / .cuda() replace every tensor"""
    from mvlt_amd.optim import FusedAdamW
    m, out = started(dtype)
    m.train()
    b = batch()
    with torch.no_grad():
        for _ in range(6):                                 # (one forward moves the statistics by a tenth of the way: 0.15 on the bf16 output, short of the control)
            m(b["image"], b["input_ids"])
    m.eval()
    out = judge(parity, "train-forward", m, dtype, out, moved=("t2i_logits",))
    P = m.store.P
    m.cpu()
    m.cuda()
    again = forward(m)
    CC.audit(m)
    assert m.store.P is not P
    same(parity, "cpu-cuda", again, out, dtype)            # nothing was written: the same outputs from the re-materialised store
    opt = FusedAdamW(m, lr=LR, weight_decay=0.05)
    backward(m)
    opt.step()
    judge(parity, "cpu-cuda-step", m, dtype, again)


# ================================================================================================ writers 5 and 6: the fused optimizers
def _opt(kind, m):
    from mvlt_amd.optim import FusedAdamW, FusedLamb
    if kind.startswith("lamb"):
        return FusedLamb(m, lr=LAMB_LR, weight_decay=0.05)
    if kind == "adamw-groups-frozen":
        head = [p for n, p in m.named_parameters() if "head" in n.split(".")[0]]
        rest = [p for n, p in m.named_parameters() if "head" not in n.split(".")[0]]
        return FusedAdamW(m, param_groups=[dict(params=rest, lr=LR, weight_decay=0.05), dict(params=head, lr=2 * LR, weight_decay=0.01)])
    return FusedAdamW(m, lr=LR, weight_decay=0.05, skip_nonfinite="gate" in kind)


STEPS = ["adamw-all", "adamw-frozen", "adamw-groups-frozen", "adamw-gate-closed", "adamw-gate-open", "lamb-all", "lamb-frozen"]
BETWEEN = [None, "load-frozen", "mul-frozen", "mul-trainable"]
FROZEN_T, FROZEN_1D, TRAINABLE_T = "block1.0.mlp.fc1.weight", "block2.1.norm2.weight", "block4.0.mlp.fc2.weight"


def _step(kind, m, opt, between=None):
    """backward -> [a parameter write] -> step, the gate variants through what BF16Scaler(skip_nonfinite=True) runs after its backward (tests/test_guard_gpu.py)"""
    S = m.store
    backward(m)
    if between is not None:
        between()
    if "gate" in kind:
        if kind.endswith("closed"):
            name = max((n for n, p in S.params.items() if p.requires_grad), key=lambda n: S.offsets[n][1])
            S.G[S.offsets[name][0] + 3] = float("inf")
        S.scale_in_optimizer = True
        try:
            norm = S.gate_grads(None)
            opt.step()
        finally:
            S.scale_in_optimizer = False
            S.apply_pending_scale()
        assert bool(torch.isfinite(norm)) == kind.endswith("open")
    else:
        opt.step()


@pytest.mark.parametrize("between", BETWEEN, ids=[b or "plain" for b in BETWEEN])
@pytest.mark.parametrize("kind", STEPS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_fused_step(dtype, kind, between, parity, monkeypatch):
    """writer 5 (between=None) and writer 6 = hypothesis 1: a parameter write between the backward and the step.  A step that leaves elements alone
    (frozen ones, everything behind a closed gate) leaves THEIR bf16 copies alone: declaring C fresh afterwards is right only if it was current before."""
    from mvlt_amd import ops
    m, out = started(dtype)
    S = m.store
    frozen = "frozen" in kind
    if frozen:
        freeze_lower(m)
    opt = _opt(kind, m)
    params = dict(m.named_parameters())
    assert params[FROZEN_T].requires_grad == (not frozen) and params[TRAINABLE_T].requires_grad
    sd2 = filled(2)

    def write():
        with torch.no_grad():
            if between == "load-frozen":               # other weights for what this setting freezes (for everything of stages 1-2 when nothing is frozen)
                names = [n for n, p in params.items() if n.startswith(("block1.", "block2.", "patch_embed1.", "patch_embed2.", "text_embed1.", "text_embed2."))]
                sd = {k: v.clone() for k, v in m.state_dict().items()}
                sd.update({n: sd2[n] for n in names})
                m.load_state_dict(sd, strict=True)
            elif between == "mul-frozen":
                params[FROZEN_T].mul_(FACTOR)
                params[FROZEN_1D].mul_(FACTOR)
            else:
                params[TRAINABLE_T].mul_(FACTOR)

    _step(kind, m, opt, write if between else None)
    casts = []
    real = ops.cast_bf16
    monkeypatch.setattr(ops, "cast_bf16", lambda *a, **k: (casts.append(1), real(*a, **k))[1])
    closed = kind.endswith("closed")
    # what must have moved: everything after a step that was applied; behind a closed gate only what the between-write reaches for sure
    moved = OUTS if not closed or between != "mul-trainable" else TEXT_OUTS
    got = judge(parity, f"{kind}/{between}", m, dtype, out, moved=moved, unmoved=closed and between is None)
    monkeypatch.undo()
    if dtype == torch.bfloat16 and between is None:
        # the shortcut itself is under test, not the cast: the kernel wrote C (or left a current C alone), and the forward made no cast.  (The fresh judge
        # model inside `judge` casts once for itself.)
        assert len(casts) == 1, casts
    if dtype == torch.float32:
        assert not casts and S.C is None
    if closed:                                          # nothing but the between-write may have changed
        want = {k: v.clone() for k, v in filled(1).items()}
        if between == "load-frozen":
            want.update({n: sd2[n] for n in want if n.startswith(("block1.", "block2.", "patch_embed1.", "patch_embed2.", "text_embed1.", "text_embed2."))})
        elif between == "mul-frozen":
            want[FROZEN_T], want[FROZEN_1D] = want[FROZEN_T] * FACTOR, want[FROZEN_1D] * FACTOR
        elif between == "mul-trainable":
            want[TRAINABLE_T] = want[TRAINABLE_T] * FACTOR
        for n, p in params.items():
            assert torch.equal(p.detach().cpu(), want[n]), n
    if between is None:                                 # a second step from the state the first one left: the shortcut's bookkeeping survives being used
        _step(kind.replace("closed", "open"), m, opt)
        judge(parity, f"{kind}/second", m, dtype, got)


# ================================================================================================ writer 7: the averaged model
@pytest.mark.parametrize("frozen", [False, True], ids=["all", "frozen"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_model_ema(dtype, frozen, parity):
    from mvlt_amd.optim import FusedAdamW, FusedModelEma
    m, _ = started(dtype)
    if frozen:
        freeze_lower(m)
    opt = FusedAdamW(m, lr=LR, weight_decay=0.05)
    ema = FusedModelEma(m, decay=0.1)
    e = ema.ema
    e.injected_masks = m.injected_masks
    out = forward(e)
    CC.audit(e)
    _step("adamw", m, opt)
    ema.update(m)
    out = judge(parity, "ema-update", e, dtype, out)
    # a write to the averaged model's own parameters between its forward and the next update (what c_current guards)
    with torch.no_grad():
        dict(e.named_parameters())[FROZEN_T].mul_(FACTOR)
    _step("adamw", m, opt)
    ema.update(m)
    out = judge(parity, "ema-write-update", e, dtype, out)
    m.load_state_dict(filled(3), strict=True)
    ema.set(m)
    out = judge(parity, "ema-set", e, dtype, out)
    want = forward(m)
    same(parity, "ema-set-is-the-model", out, want, dtype)
    ema.load_state_dict(dict(filled(2), _ema_updates=5))
    out = judge(parity, "ema-load_state_dict", e, dtype, out)
    assert ema.updates == 5
    ema.load_state_dict(filled(1))                         # ... and an update right behind a load, no forward between: the copy is NOT current for
    ema.update(m)                                          # the loaded parameters, and with frozen ones the launch leaves their elements alone
    judge(parity, "ema-load-update", e, dtype, out)


# ================================================================================================ hypothesis 2: a replaced Parameter in the middle of the model
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_replaced_parameters_are_noticed(dtype, parity):
    """pinned: the store re-materialises (is_current() compares every slot of the module tree), the forward computes with the new values, and an optimizer
    built before follows a `p.data = ...` (same Parameter) but refuses a new Parameter by name"""
    from mvlt_amd.optim import FusedAdamW
    from mvlt_amd.params import Holder
    m, out = started(dtype)
    opt = FusedAdamW(m, lr=LR, weight_decay=0.05)
    _step("adamw", m, opt)
    out = judge(parity, "step", m, dtype, out)
    P = m.store.P
    p = dict(m.named_parameters())["block3.1.mlp.fc2.weight"]
    p.data = (p.detach() * FACTOR).clone()
    out = judge(parity, "p.data=", m, dtype, out, moved=TEXT_OUTS)
    assert m.store.P is not P and p.data_ptr() == m.store.master("block3.1.mlp.fc2.weight").data_ptr()
    moments = opt._m.clone()
    before = {n: q.detach().clone() for n, q in m.named_parameters()}
    _step("adamw", m, opt)                                 # the old optimizer: same Parameters, same layout -> it steps the new store, moments kept
    out = judge(parity, "p.data=/step", m, dtype, out)
    assert opt._mask_key[0] == m.store.P.data_ptr() and not torch.equal(opt._m, moments) and bool((moments != 0).any())
    for n in ("block3.1.mlp.fc2.weight", "patch_embed1.proj.weight", "block3.1.mlp.fc2.bias", "sub_cls_head.linear.weight"):       # the re-pointed tensor, its neighbours, both ends
        assert not torch.equal(dict(m.named_parameters())[n].detach(), before[n]), n
    # a whole head replaced, as a fine-tune does
    head = type(m.sup_cls_head)(768, 48)
    with torch.no_grad():
        head.linear.weight.copy_(filled(3)["sup_cls_head.linear.weight"])
        head.linear.bias.copy_(filled(3)["sup_cls_head.linear.bias"])
        head.linear_bias.copy_(filled(3)["sup_cls_head.linear_bias"])
    m.sup_cls_head = head.cuda()
    out = judge(parity, "new-head", m, dtype, out, moved=("sup_cls_logits",))
    assert m.store.params["sup_cls_head.linear.weight"] is m.sup_cls_head.linear.weight
    assert m.sup_cls_head.linear.weight.data_ptr() == m.store.master("sup_cls_head.linear.weight").data_ptr()
    backward(m)
    with pytest.raises(RuntimeError, match=r"sup_cls_head\.\w+.*replaced"):
        opt.step()
    opt = FusedAdamW(m, lr=LR, weight_decay=0.05)          # a new optimizer steps the new head
    w = m.sup_cls_head.linear.weight.detach().clone()
    _step("adamw", m, opt)
    judge(parity, "new-head/step", m, dtype, out)
    assert not torch.equal(m.sup_cls_head.linear.weight.detach(), w)


# ================================================================================================ hypothesis 3: writes through .data
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_data_writes_need_invalidate(dtype, parity):
    from mvlt_amd.optim import FusedAdamW
    m, out = started(dtype)
    S = m.store
    opt = FusedAdamW(m, lr=LR, weight_decay=0.05)
    _step("adamw", m, opt)
    p = dict(m.named_parameters())["block3.0.attn.proj.weight"]
    v = S.versions()
    p.data.mul_(FACTOR)
    assert S.versions() == v                               # the premise: no counter the store reads has moved
    S.invalidate()
    out = judge(parity, "data-invalidate", m, dtype, out)
    # the controls: without invalidate() the write is NOT seen (the documented limit, docs/coherence.md), and after a fused step force_dirty alone
    # rebuilds the derived copies from a bf16 copy the step declared fresh
    p.data.mul_(0.5)
    forward(m)
    stale = CC.first_stale(m)
    assert stale is not None and stale[0] == ("C[block3.0.attn.proj.weight]" if dtype == torch.bfloat16 else "block3.0.attn.proj.weight::T"), stale
    S.invalidate()
    out = judge(parity, "data-invalidate-2", m, dtype, out, moved=())
    _step("adamw", m, opt)
    p.data.mul_(FACTOR)
    S.force_dirty = True
    forward(m)
    stale = CC.first_stale(m)
    if dtype == torch.bfloat16:
        assert stale is not None and stale[0] == "C[block3.0.attn.proj.weight]", stale
    else:
        assert stale is None                               # (no bf16 copy: the derived copies are rebuilt from P)
    S.invalidate()
    judge(parity, "data-invalidate-3", m, dtype, out)

"""GPU: AdamW with a learning rate and a weight decay per parameter group (docs/param_groups.md) -- mvlt_adamw_step_groups against the kernel it is modelled on
(one mvlt_adamw_step call per group slice: bit for bit), against float64 where groups change inside a 16-byte vector, its frozen byte, its gate and its clip
coefficient; then FusedAdamW(param_groups=layer_decay_groups(...)) through BF16Scaler against torch.optim.AdamW over the same groups, with a frozen stage, a
clip that bites and the non-finite guard, the launch choice, and a checkpoint in the middle of a run.  The argument refusals need no GPU: tests/test_param_groups_cpu.py."""
import io

import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NT = 256                                   # threads per workgroup of the element-wise kernels
TRIP = 8192 * NT * 4                       # elements one trip of the grid-stride loop covers: the launch has at most 8192 workgroups (csrc/adamw_groups.hip)
SIZES = [4, 8, 1028, 4 * (256 * 3 + 1), TRIP + 4 * (NT + 1)]          # the last: just past a full grid, the loop takes a second trip
NAN = float("nan")
STEP_T = 3


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _hp(gs=0.5, lr=NAN, wd=NAN):
    """the row of mvlt_adamw_step; the grouped kernel ignores slots 0 and 4 -- NaN there reaches nothing"""
    return torch.tensor([lr, 0.9, 0.999, 1e-8, wd, 1 - 0.9 ** STEP_T, 1 - 0.999 ** STEP_T, gs], dtype=torch.float32, device=DEV)


def _table(k):
    """k groups: no two learning rates alike, every third group without weight decay, values with full mantissas (a product rounded twice instead of once shows)"""
    rows = [[1e-3 * 0.75 ** (i % 9) * (1 + 0.013 * i), 0.0 if i % 3 == 0 else 0.05 * (1 + 0.1 * i)] for i in range(k)]
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


def _state(n, seed=21):
    g_ = torch.Generator().manual_seed(seed + n % 1000)
    p, gr, m = (torch.randn(n, generator=g_).to(DEV) for _ in range(3))
    v = torch.rand(n, generator=g_).to(DEV) * 1e-4
    p16 = torch.full((n,), -1.5, dtype=torch.bfloat16, device=DEV)
    return [p, gr * 1e-2, m * 1e-2, v, p16]


def _clone(st):
    return [t.clone() for t in st]


def _slices(n, k, seed=3):
    """k contiguous slices of [0, n) with 4-aligned boundaries, ragged lengths"""
    k = min(k, n // 4)
    g_ = torch.Generator().manual_seed(seed)
    cuts = sorted((torch.randperm(n // 4 - 1, generator=g_)[:k - 1] + 1).tolist()) if k > 1 else []
    edges = [0] + [4 * c for c in cuts] + [n]
    return list(zip(edges[:-1], edges[1:]))


def _groups(st, hp, group_of, table, **kw):
    from mvlt_amd import ops
    p, g, m, v, p16 = st
    ops.adamw_step_groups(p, g, m, v, p16, p.numel(), hp, group_of, table, table.shape[0], **kw)


def _slice_oracle(st, slices, bytes_, table, gs, cd):
    """one launch of the existing kernel per slice: the slice's lr in hp[0], its weight decay in hp[4], a mask of all 1 (zero-decay groups too: 1 - lr * 0)"""
    from mvlt_amd import ops
    p, g, m, v, p16 = st
    ones = torch.ones(p.numel(), dtype=torch.uint8, device=DEV)
    tab = table.tolist()
    for (lo, hi), b in zip(slices, bytes_):
        if b >= len(tab):
            continue                                       # a frozen slice: no launch
        hp = _hp(gs, tab[b][0], tab[b][1])
        ops.adamw_step(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], p16[lo:hi], hi - lo, hp, ones[lo:hi], gscale_dev=cd)


# ------------------------------------------------------------------------------------------------------------------ kernel: bit identity with mvlt_adamw_step
@pytest.mark.parametrize("clip", [None, 0.37])
@pytest.mark.parametrize("n", SIZES)
def test_group_slices_equal_one_launch_of_the_old_kernel_per_slice(n, clip):
    table = _table(7)
    slices = _slices(n, 6)
    bytes_ = [[5, 2, 255, 0, 6, 3][j % 6] for j in range(len(slices))]           # groups in no particular order, one slice frozen, group 0 (no decay) and decayed ones
    group_of = torch.empty(n, dtype=torch.uint8, device=DEV)
    for (lo, hi), b in zip(slices, bytes_):
        group_of[lo:hi] = b
    cd = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=DEV)
    st0 = _state(n)
    got, want = _clone(st0), _clone(st0)
    _groups(got, _hp(0.5), group_of, table, gscale_dev=cd)
    _slice_oracle(want, slices, bytes_, table, 0.5, cd)
    torch.cuda.synchronize()
    for name, a, b, old in zip("p g m v p16".split(), got, want, st0):
        assert _same(a, b), (name, int((_bits(a) != _bits(b)).sum()), n)
        if name != "g":
            live = group_of != 255
            assert not torch.equal(a[live], old[live]), name                       # ... and the step happened
            assert _same(a[~live], old[~live]), name
    if clip is not None:                                                           # the coefficient reached the moments
        plain = _clone(st0)
        _groups(plain, _hp(0.5), group_of, table)
        assert not _same(plain[2], got[2])


# ------------------------------------------------------------------------------------------------------------------ kernel: any four bytes in a vector
def _float64_step(st0, group_of, table, gs):
    """AdamW per element in float64 from the fp32 hyper-parameters the kernel reads (1 - beta is exact in fp32 for beta in [0.5, 1])"""
    p, g, m, v = (t.double() for t in st0[:4])
    hp = _hp(gs).double().tolist()
    _, b1, b2, eps, _, bc1, bc2, gsc = hp
    k = table.shape[0]
    idx = group_of.long().clamp(max=k - 1)
    lr, wd = table.double()[idx, 0], table.double()[idx, 1]
    gr = g * gsc
    m2 = b1 * m + (1 - b1) * gr
    v2 = b2 * v + (1 - b2) * gr * gr
    p2 = p * (1 - lr * wd) - (lr / bc1) * m2 / (v2.sqrt() / bc2 ** 0.5 + eps)
    return p2, m2, v2


@pytest.mark.parametrize("k", [7, 254])
def test_groups_that_change_inside_a_vector_match_float64(parity, k):
    """No slice oracle exists here.  The bound is the one tests/test_clip_gpu.py::test_clipped_step_matches_torch holds the stepped moments to, with its
    metric: relative L2 error 2e-5."""
    from tests.test_clip_gpu import _rel
    n = 4 * (256 * 3 + 1)
    table = _table(k)
    g_ = torch.Generator().manual_seed(k)
    group_of = torch.randint(0, k, (n,), generator=g_, dtype=torch.uint8)          # a new group at (almost) every element
    kind = torch.randint(0, 4, (n // 4,), generator=g_)
    frozen = torch.rand(n // 4, 4, generator=g_) < 0.4                             # lone frozen lanes in a quarter of the vectors ...
    frozen[kind != 0] = False
    frozen[kind == 1] = True                                                       # ... a quarter of the vectors frozen whole
    frozen[0] = torch.tensor([True, False, False, True])
    frozen[-1] = True
    frozen = frozen.reshape(-1)
    oob = frozen & (torch.arange(n) % 2 == 0) if k < 254 else torch.zeros(n, dtype=torch.bool)
    group_of[frozen] = 255
    group_of[oob] = k + 1                                                          # a byte past the table that is not 255: frozen as well
    group_of, fz = group_of.to(DEV), frozen.to(DEV)
    mixed = (frozen.view(-1, 4).any(1) & ~frozen.view(-1, 4).all(1)).sum()
    assert int(mixed) > 50 and int(frozen.view(-1, 4).all(1).sum()) > 50
    st0 = _state(n)
    for t in st0[1:4]:
        t[fz] = NAN                                                                # g, m, v of a frozen lane reach nothing
    got = _clone(st0)
    _groups(got, _hp(0.5), group_of, table)
    torch.cuda.synchronize()
    for name, a, old in zip("p g m v p16".split(), got, st0):
        assert _same(a[fz], old[fz]), f"a frozen lane's {name} was written"
    live = ~fz
    for name, a, ref in zip("p m v".split(), (got[0], got[2], got[3]), _float64_step(st0, group_of, table, 0.5)):
        err = _rel(a[live], ref[live])
        print(f"k={k}: {name} relative L2 error against float64 {err:.3e}")
        assert parity(f"groups-mixed/{name}/{k}", err, 2e-5)
    assert _same(got[4][live], got[0][live].to(torch.bfloat16))
    # the learning rates did reach their elements: one rate for all would be far outside the bound
    flat = _float64_step(st0, torch.zeros_like(group_of), table, 0.5)
    assert _rel((got[0] - st0[0])[live], (flat[0] - st0[0].double())[live]) > 0.1


def test_an_all_frozen_buffer_is_untouched():
    n = 1028
    table = _table(3)
    st0 = _state(n)
    st0[1].fill_(NAN)
    for byte in (255, 3, 200):                                                     # the frozen byte, the first byte past the table, one far past it
        got = _clone(st0)
        _groups(got, _hp(0.5), torch.full((n,), byte, dtype=torch.uint8, device=DEV), table)
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(got, st0)), byte


# ------------------------------------------------------------------------------------------------------------------ kernel: gate, slices of a launch
def _any_map(n, k, seed=11):
    g_ = torch.Generator().manual_seed(seed)
    group_of = torch.randint(0, k, (n,), generator=g_, dtype=torch.uint8)
    group_of[torch.rand(n, generator=g_) < 0.2] = 255
    return group_of.to(DEV)


def test_a_closed_gate_leaves_everything_alone():
    n = 4 * (256 * 3 + 1)
    table = _table(5)
    st0 = _state(n)
    got = _clone(st0)
    poisoned = torch.full((n,), 200, dtype=torch.uint8, device=DEV)                # bytes past the table: the closed gate returns before it reads them
    poisoned[::3] = 4
    gate = torch.tensor([float("inf"), 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    _groups(got, _hp(0.5), poisoned, table, gate=gate)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(got, st0))


def test_an_open_gate_is_the_clip_coefficient():
    n = 4 * (256 * 3 + 1)
    table, group_of = _table(5), _any_map(n, 5)
    st0 = _state(n)
    gated, clipped = _clone(st0), _clone(st0)
    gate = torch.tensor([2.5, 0.37, 1.0, 0.0], dtype=torch.float32, device=DEV)
    _groups(gated, _hp(0.5), group_of, table, gate=gate)
    _groups(clipped, _hp(0.5), group_of, table, gscale_dev=gate[1:2])
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(gated, clipped))
    assert not _same(gated[0], st0[0])
    from mvlt_amd import _lib as L
    assert L.last_kernel().startswith("adamw_groups_kernel<")


def test_a_sliced_launch_equals_that_range_of_a_whole_launch():
    from mvlt_amd import ops
    n = 4 * (256 * 3 + 1)
    lo, hi = 516, n - 8
    table, group_of = _table(5), _any_map(n, 5)
    st0 = _state(n)
    whole, part = _clone(st0), _clone(st0)
    _groups(whole, _hp(0.5), group_of, table)
    p, g, m, v, p16 = part
    ops.adamw_step_groups(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], p16[lo:hi], hi - lo, _hp(0.5), group_of[lo:hi], table, 5)
    torch.cuda.synchronize()
    for a, b, old in zip(part, whole, st0):
        assert _same(a[lo:hi], b[lo:hi]) and _same(a[:lo], old[:lo]) and _same(a[hi:], old[hi:])


# ------------------------------------------------------------------------------------------------------------------ model level
LT = dict(mlm=1, itm=1, t2i=0, cls=0)
T, B, IMG = 16, 4, 128                      # pvlt_tiny at 128 px with a 16-token caption, batch 4
LR, WD, DECAY = 1e-3, 0.05, 0.75
_BATCH = {}


def _model(dtype, seed=8, freeze=None):
    from mvlt_amd import pvlt
    cfg = O.Cfg("pvlt_tiny", LT, 224, 768, T, 0.0)
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, drop_path_rate=0.0, compute_dtype=dtype)
    m.load_state_dict(O.filled_state_dict(cfg, seed), strict=True)
    m.cuda().train()
    for prefix in freeze or ():
        for n, p in m.named_parameters():
            if n.startswith(prefix):
                p.requires_grad_(False)
    m.injected_masks = dict(bert=torch.ones(B, T, 768), droppath=[torch.ones(B)] * 8, droppath2=[torch.ones(B)] * 8)
    return m


def _loss(m, seed):
    from mvlt_amd.engine import compute_losses
    if seed not in _BATCH:
        _BATCH[seed] = {k: v.to(DEV) for k, v in O.to_torch_batch(filler.make_batch(seed, B, IMG, T)).items()}
    b = _BATCH[seed]
    out = m(b["image"], b["input_ids"], mlm_labels=b["mlm_labels"])
    total, _ = compute_losses(out, b["image"], b["mlm_labels"], b["itm_labels"], b["sup_cls_labels"], b["sub_cls_labels"])
    return total


def _twin(m, groups):
    """torch.optim.AdamW over clones of the fp32 masters, in the same groups"""
    names = {id(p): n for n, p in m.named_parameters()}
    clones = {n: torch.nn.Parameter(p.detach().clone()) for n, p in m.named_parameters()}
    tg = [dict(params=[clones[names[id(p)]] for p in g["params"]], lr=g["lr"], weight_decay=g["weight_decay"]) for g in groups]
    return clones, torch.optim.AdamW(tg, lr=LR, betas=(0.9, 0.999), eps=1e-8)


def _count_group_launches(monkeypatch):
    from mvlt_amd import ops
    calls, orig = [], ops.adamw_step_groups
    monkeypatch.setattr(ops, "adamw_step_groups", lambda *a, **kw: (calls.append(kw), orig(*a, **kw))[1])
    return calls


def _opt_state(m, opt):
    S = m.store
    return [t.clone() for t in (S.P, opt._m, opt._v)] + ([S.C.clone()] if S.C is not None else [])


@pytest.mark.parametrize("case", ["plain-fp32", "plain-bf16", "frozen-stage", "clip", "guard"])
def test_layer_decay_steps_match_torch_adamw_over_the_same_groups(parity, monkeypatch, case):
    """Two steps through BF16Scaler + FusedAdamW against stock AdamW on clones of the fp32 masters with the same .grad.  The bar is the one
    tests/test_freeze_gpu.py::test_step_leaves_frozen_parameters_alone holds the fused optimizer to against torch.optim.AdamW: every tensor within 1e-6 of
    its largest element (tests/test_kernels_gpu.py's max-norm metric)."""
    from mvlt_amd.engine import BF16Scaler
    from mvlt_amd.optim import FusedAdamW, layer_decay_groups
    from tests.test_freeze_gpu import maxrel
    dtype = torch.float32 if case == "plain-fp32" else torch.bfloat16
    guard = case == "guard"
    m = _model(dtype, freeze=("block2.",) if case == "frozen-stage" else None)
    groups = layer_decay_groups(m, LR, WD, DECAY)
    assert len(groups) == 2 * (sum(m.depths) + 2) and len({g["lr"] for g in groups}) == sum(m.depths) + 2
    clones, topt = _twin(m, groups)
    start = {n: q.detach().clone() for n, q in clones.items()}
    opt = FusedAdamW(m, param_groups=groups, skip_nonfinite=guard)
    scaler = BF16Scaler(skip_nonfinite=guard)
    calls = _count_group_launches(monkeypatch)
    max_norm = 1e-3 if case == "clip" else None                                    # (as tests/test_freeze_gpu.py's engine loop: far below the norm, the clip bites)
    for it in range(2):
        total = _loss(m, 8 + it)
        opt.zero_grad()
        scaler(total, opt, clip_grad=max_norm, parameters=m.parameters())
        S = m.store
        for n, q in clones.items():
            gr = S.params[n].grad
            q.grad = None if gr is None else gr.detach().clone()
        if max_norm:
            ref_norm = float(torch.nn.utils.clip_grad_norm_([q for q in clones.values() if q.grad is not None], max_norm))
            assert ref_norm > max_norm
            assert parity("groups-model/clip-norm", abs(float(scaler.last_grad_norm) - ref_norm) / ref_norm, 1e-5)       # tests/test_clip_gpu.py NORM_TOL
        topt.step()
    torch.cuda.synchronize()
    assert len(calls) == 2 and all((kw["gate"] is not None) == guard and (kw["gscale_dev"] is not None) == (case == "clip") for kw in calls)
    live = [n for n, p in S.params.items() if p.requires_grad]
    worst = max(maxrel(S.params[n].detach(), clones[n].detach()) for n in live)
    print(f"{case}: trainable parameters against torch.optim.AdamW over {len(groups)} groups, worst max-norm relative error {worst:.3e}")
    assert parity(f"groups-model/{case}", worst, 1e-6)
    assert all(not torch.equal(S.params[n].detach(), start[n]) for n in live)
    # a control: the groups matter -- one lr for all is far outside the bar for the lowest layer
    lowest = "patch_embed1.proj.weight"
    step_taken = (S.params[lowest].detach() - start[lowest]).abs().max()
    assert float(step_taken) < 2.5 * 2 * LR * DECAY ** (sum(m.depths) + 1) and float(step_taken) > 0
    for n, p in S.params.items():
        if not p.requires_grad:
            off, cnt, _ = S.offsets[n]
            assert torch.equal(p.detach(), start[n]) and p.grad is None, n
            assert not opt._m[off:off + cnt].any() and not opt._v[off:off + cnt].any(), n
    if case == "frozen-stage":
        assert sum(not p.requires_grad for p in S.params.values()) > 30
    if guard:
        # a third step whose gradients hold an Inf: what BF16Scaler runs after the backward, on the poisoned buffer -- nothing moves, one skip is counted
        assert (opt.applied_steps, opt.skipped_steps) == (2, 0)
        before = _opt_state(m, opt)
        total = _loss(m, 8)
        opt.zero_grad()
        total.backward()
        off, _, _ = S.offsets["block3.0.mlp.fc1.weight"]
        S.G[off + 3] = float("inf")
        norm = S.gate_grads(None)
        opt.step()
        torch.cuda.synchronize()
        assert not torch.isfinite(norm).item() and len(calls) == 3 and calls[-1]["gate"] is not None
        for name, a, b in zip("P m v C".split(), _opt_state(m, opt), before):
            assert _same(a, b), name
        assert (opt.applied_steps, opt.skipped_steps) == (2, 1) and opt.skipped_steps == 1


def test_groups_with_one_lr_and_one_decay_take_the_old_launches(monkeypatch):
    from mvlt_amd import _lib as L, ops
    from mvlt_amd.optim import FusedAdamW
    A, Bm = _model(torch.bfloat16), _model(torch.bfloat16)
    named = list(A.named_parameters())
    nd = [p for n, p in named if p.dim() == 1 or n.endswith(".bias")]
    dec = [(n, p) for n, p in named if not (p.dim() == 1 or n.endswith(".bias"))]
    groups = [dict(params=[p for n, p in dec if "head" in n], weight_decay=WD, name="heads"), dict(params=nd, weight_decay=0.0, name="no_decay"),
              dict(params=[p for n, p in dec if "head" not in n], weight_decay=WD, name="trunk")]
    optA = FusedAdamW(A, lr=LR, weight_decay=0.3, param_groups=groups)            # (the optimizer-wide default decay is not used: every group names its own)
    optB = FusedAdamW(Bm, lr=LR, weight_decay=WD)

    def refuse(*a, **kw):
        raise AssertionError("the grouped kernel was launched for groups that share one lr and one weight decay")
    with monkeypatch.context() as mp:
        mp.setattr(ops, "adamw_step_groups", refuse)
        for it in range(2):
            for m_, o in ((A, optA), (Bm, optB)):
                o.zero_grad()
                _loss(m_, 8 + it).backward()
            Bm.store.G.copy_(A.store.G)                     # the same gradients: two backward passes differ in their last bits (fp32 atomics)
            optA.step()
            assert L.last_kernel().startswith("adamw_kernel<")
            optB.step()
            torch.cuda.synchronize()
            for name, a, b in zip("P m v C".split(), _opt_state(A, optA), _opt_state(Bm, optB)):
                assert _same(a, b), (name, it)
    # the choice is taken per step: a scheduler (or a user) that gives one group a rate of its own switches the launch
    optA.param_groups[0]["lr"] = 2 * LR
    optA.zero_grad()
    _loss(A, 8).backward()
    optA.step()
    torch.cuda.synchronize()
    assert L.last_kernel().startswith("adamw_groups_kernel<")
    assert not _same(A.store.P, Bm.store.P) and torch.isfinite(A.store.P).all().item()


def test_state_dict_round_trip_in_the_middle_of_a_run():
    from mvlt_amd.optim import FusedAdamW, layer_decay_groups
    m = _model(torch.bfloat16)
    opt = FusedAdamW(m, param_groups=layer_decay_groups(m, LR, WD, DECAY))
    opt.zero_grad()
    _loss(m, 8).backward()
    opt.step()
    S = m.store
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    p1 = S.P.clone()
    opt.zero_grad()
    _loss(m, 9).backward()                                  # (the fused step never rewrites G: both continuations below consume these gradients)
    opt.step()
    torch.cuda.synchronize()
    want = _opt_state(m, opt)
    # back to the state after step 1, into a NEW optimizer built the way a resumed run builds it
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu", weights_only=False)
    assert set(sd["fused"]) == {"step", "m", "v"} and sd["fused"]["step"] == 1
    assert [g["name"] for g in sd["param_groups"]] == [g["name"] for g in opt.param_groups] and all("lr_scale" in g for g in sd["param_groups"])
    S.P.copy_(p1)
    opt2 = FusedAdamW(m, param_groups=layer_decay_groups(m, 7.0, 0.5, 0.5))        # (the checkpoint's rates replace these)
    opt2.load_state_dict(sd)
    assert [g["lr"] for g in opt2.param_groups] == [g["lr"] for g in opt.param_groups] and opt2._step == 1
    opt2.step()
    torch.cuda.synchronize()
    for name, a, b in zip("P m v C".split(), _opt_state(m, opt2), want):
        assert _same(a, b), name

"""GPU: the non-finite-gradient guard (docs/nonfinite_guard.md) -- mvlt_step_gate decides on the device whether the optimizer may step (the norm of
mvlt_clip_coef in the same bits, ok = norm is finite, the clip coefficient or exactly 1 / exactly 0), mvlt_adamw_step_gated obeys it (ok = 0: not one
byte of p / m / v / the bf16 copy changes; ok = 1: mvlt_adamw_step bit for bit), and FlatStore.gate_grads / FusedAdamW(skip_nonfinite=True) /
BF16Scaler(skip_nonfinite=True) carry it through a training step: a poisoned step changes nothing, and training goes on as if it had not happened.
Everything here is compared in bits (integer views): the guard adds no arithmetic of its own."""
import numpy as np
import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _randn(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g) * 1e-3).to(DEV)


# ------------------------------------------------------------------------------------------------------------------ the gate kernel
N = 8192


def _gate(g, n_partials, grad_scale=1.0, max_norm=1.0, mask=None, counters=None):
    """-> (gate [4], mvlt_clip_coef's [norm, coef] on the same partials, counters)"""
    from mvlt_amd import ops
    part = torch.full((n_partials,), NAN, device=DEV)
    ops.grad_sumsq(g, g.numel(), mask, part)
    clip = torch.full((2,), NAN, device=DEV)
    ops.clip_coef(part, grad_scale, max_norm, clip)
    gate = torch.full((4,), NAN, device=DEV)
    if counters is None:
        counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.step_gate(part, grad_scale, max_norm, gate, counters)
    return gate, clip, counters


@pytest.mark.parametrize("n_partials", [1, 7, 1024])
def test_gate_on_finite_gradients(n_partials):
    g = _randn(N, 40 + n_partials)
    norms = []
    for max_norm in (0.0, 1e-3, 1e9):
        gate, clip, counters = _gate(g, n_partials, grad_scale=0.5, max_norm=max_norm)
        gate, clip = gate.cpu(), clip.cpu()
        print(f"n_partials={n_partials} max_norm={max_norm}: gate {gate.tolist()} clip {clip.tolist()}")
        assert _same(gate[0:1], clip[0:1])                                   # the norm, in mvlt_clip_coef's bits
        assert float(gate[2]) == 1.0 and float(gate[3]) == 0.0
        assert counters.tolist() == [1, 0]
        if max_norm > 0:
            # min(1, max_norm / (norm + 1e-6)) in fp32, each operation rounded once: torch's own arithmetic on the same fp32 norm
            want = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (gate[0] + torch.tensor(1e-6, dtype=torch.float32)), max=1.0)
            assert _same(gate[1:2], want.reshape(1)) and _same(gate[1:2], clip[1:2])
        else:
            assert float(gate[1]) == 1.0                                     # no clipping asked for: exactly 1
        norms.append(float(gate[0]))
    assert 1e-3 < 0.5 * float(torch.linalg.vector_norm(g.double())) < 1e9    # 1e-3 bites, 1e9 does not
    assert norms[0] == norms[1] == norms[2] and norms[0] > 0


@pytest.mark.parametrize("n_partials", [1, 7, 1024])
def test_gate_closes_on_nonfinite_gradients(n_partials):
    g0 = _randn(N, 50)
    for pos in (0, N - 1, N // 2 + 1):
        for bad in (NAN, INF, -INF):
            g = g0.clone()
            g[pos] = bad
            for max_norm in (0.0, 1.0):
                gate, clip, counters = _gate(g, n_partials, max_norm=max_norm)
                gate = gate.cpu()
                assert not np.isfinite(float(gate[0])), (pos, bad, max_norm)
                assert _same(gate[0:1], clip[0:1].cpu())
                assert _same(gate[1:4], torch.zeros(3)), (pos, bad, max_norm, gate.tolist())      # coefficient exactly +0, ok 0, reserved 0
                assert counters.tolist() == [0, 1]


@pytest.mark.parametrize("n_partials", [1, 7, 1024])
def test_gate_ignores_what_the_mask_leaves_out(n_partials):
    g = _randn(N, 51)
    mask = torch.ones(N, dtype=torch.uint8)
    mask[0] = 0
    mask[5:9] = 2
    mask[N // 2] = 0
    mask[N - 1] = 2
    g[0], g[5], g[7], g[N // 2], g[N - 1] = NAN, INF, -INF, NAN, INF
    md = mask.to(DEV)
    gate, clip, counters = _gate(g, n_partials, mask=md)
    assert float(gate[2]) == 1.0 and np.isfinite(float(gate[0])) and counters.tolist() == [1, 0]
    ref = float(torch.linalg.vector_norm(g[md == 1].double()))
    assert abs(float(gate[0]) - ref) / ref < 1e-5                            # (tests/test_clip_gpu.py derives this bound for the norm kernel)
    g[6] = NAN                                                               # ... and one bad value under a mask byte of 1 closes it
    mask[6] = 1
    gate, _, _ = _gate(g, n_partials, mask=mask.to(DEV))
    assert float(gate[2]) == 0.0 and float(gate[1]) == 0.0


def test_gate_counts_applied_and_skipped_steps():
    good, bad = _randn(N, 52), _randn(N, 53)
    bad[4097] = INF
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    for g in (good, bad, bad, good):
        _gate(g, 7, counters=counters)
    assert counters.tolist() == [2, 2]


# ------------------------------------------------------------------------------------------------------------------ the gated AdamW kernel
GRID_CAP_ELEMS = 8192 * 256 * 4          # mvlt_adamw_step launches grid_for(n / 4, 8192) workgroups of 256 lanes, 4 elements each: one trip covers this many


def _adamw_state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p, g, m = (torch.randn(n, generator=gen).to(DEV) for _ in range(3))
    v = torch.rand(n, generator=gen).to(DEV)
    p16 = torch.randn(n, generator=gen).to(DEV).to(torch.bfloat16)           # (NOT the cast of p: an untouched copy must keep these bits)
    mask = torch.randint(0, 3, (n,), generator=gen, dtype=torch.uint8)       # 0 / 1 / 2 mixed inside the 4-element vectors
    if n >= 64:
        mask[16:48] = 2                                                      # whole vectors frozen: the kernel's early `continue`
        mask[n - 8:n - 4] = 2
    return p, g * 1e-2, m * 1e-2, v * 1e-4, p16, mask.to(DEV)


HP = [1e-3, 0.9, 0.999, 1e-8, 0.05, 1 - 0.9 ** 3, 1 - 0.999 ** 3, 0.5]


@pytest.mark.parametrize("n", [4, 1020, 8196, GRID_CAP_ELEMS + 1028])
def test_gated_adamw_open_equals_the_ungated_kernel(n):
    from mvlt_amd import ops
    hp = torch.tensor(HP, dtype=torch.float32, device=DEV)
    for coef in (1.0, 0.37):
        p, g, m, v, p16, mask = _adamw_state(n, n % 1000)
        g[n - 2] = NAN                                                       # under a frozen byte or not, both kernels must treat it alike
        ref = [t.clone() for t in (p, m, v, p16)]
        gate = torch.tensor([3.0, coef, 1.0, 0.0], dtype=torch.float32, device=DEV)
        ops.adamw_step(ref[0], g, ref[1], ref[2], ref[3], n, hp, mask, gscale_dev=gate[1:2].clone())
        ops.adamw_step_gated(p, g, m, v, p16, n, hp, mask, gate)
        torch.cuda.synchronize()
        for name, a, b in zip("p m v p16".split(), (p, m, v, p16), ref):
            assert _same(a, b), (n, coef, name)
        if n > GRID_CAP_ELEMS:                                               # the second trip of the grid-stride loop did step
            live = mask[GRID_CAP_ELEMS:] != 2
            assert not _same(m[GRID_CAP_ELEMS:][live], _adamw_state(n, n % 1000)[2][GRID_CAP_ELEMS:][live])


@pytest.mark.parametrize("n", [4, 1020, 8196, GRID_CAP_ELEMS + 1028])
def test_gated_adamw_closed_touches_nothing(n):
    from mvlt_amd import ops
    hp = torch.tensor(HP, dtype=torch.float32, device=DEV)
    p, g, m, v, p16, mask = _adamw_state(n, 7 + n % 1000)
    g[0::3], g[1::3], g[2::3] = NAN, INF, -INF
    before = [t.clone() for t in (p, m, v, p16)]
    gate = torch.tensor([INF, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    ops.adamw_step_gated(p, g, m, v, p16, n, hp, mask, gate)
    ops.adamw_step_gated(p, g, m, v, None, n, hp, None, gate)               # without a bf16 copy and without a mask as well
    torch.cuda.synchronize()
    for name, a, b in zip("p m v p16".split(), (p, m, v, p16), before):
        assert _same(a, b), (n, name)


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


_BATCH = {}


def _batch(seed=8):
    if seed not in _BATCH:
        _BATCH[seed] = {k: v.to(DEV) for k, v in O.to_torch_batch(filler.make_batch(seed, B, IMG, T)).items()}
    return _BATCH[seed]


def _loss(m, seed=8):
    from mvlt_amd.engine import compute_losses
    b = _batch(seed)
    out = m(b["image"], b["input_ids"], mlm_labels=b["mlm_labels"])
    total, _ = compute_losses(out, b["image"], b["mlm_labels"], b["itm_labels"], b["sup_cls_labels"], b["sub_cls_labels"])
    return total


def _state(m, opt):
    S = m.store
    return [t.clone() for t in (S.P, opt._m, opt._v)] + ([S.C.clone()] if S.C is not None else [])


def _trainable_offset(S, k=3):
    """flat index of element k of the largest trainable parameter"""
    name = max((n for n, p in S.params.items() if p.requires_grad), key=lambda n: S.offsets[n][1])
    return S.offsets[name][0] + k


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_poisoned_step_is_skipped_and_training_goes_on(dtype, clip):
    from mvlt_amd.engine import BF16Scaler
    from mvlt_amd.optim import FusedAdamW
    A, Bm = _model(dtype), _model(dtype)
    optA = FusedAdamW(A, lr=1e-3, weight_decay=0.05, skip_nonfinite=True)
    optB = FusedAdamW(Bm, lr=1e-3, weight_decay=0.05)
    scA = BF16Scaler(skip_nonfinite=True)
    SA = A.store

    def clean_step():
        """A: the guarded scaler, whole.  B: its own forward and backward, then the sequence BF16Scaler() runs without the guard -- on A's gradients:
        the backward pass accumulates with fp32 atomics (word-embedding scatter, split weight-gradient GEMMs; tools/repeat_step.py measures that noise),
        so two passes over the same batch differ in their last bits whatever the optimizer does.  The guard's promise is about the step: the same
        gradients give the same bits.  (The fused path never rewrites G, so A's buffer still holds what its step consumed.)"""
        total = _loss(A)
        optA.zero_grad()
        scA(total, optA, clip_grad=clip, parameters=A.parameters())
        total = _loss(Bm)
        optB.zero_grad()
        total.backward()
        print(f"gradient elements that differ between the twins' own backward passes: {int((_bits(SA.G) != _bits(Bm.store.G)).sum())} of {SA.total}")
        Bm.store.G.copy_(SA.G)
        normB = Bm.store.clip_grad_norm(clip) if clip else None
        optB.step()
        torch.cuda.synchronize()
        for name, a, b in zip("P m v C".split(), _state(A, optA), _state(Bm, optB)):
            assert _same(a, b), name
        assert SA.pending_gate is None and SA.pending_clip is None and SA.pending_grad_scale == 1.0
        assert torch.isfinite(scA.last_grad_norm).item() and (normB is None or _same(scA.last_grad_norm.reshape(1), normB.reshape(1)))

    clean_step()                                           # step 1: the guard changes no bit of a clean step
    assert (optA.applied_steps, optA.skipped_steps) == (1, 0)
    # step 2: A's backward, then Inf in ONE trainable gradient element; what BF16Scaler runs after the backward follows
    before = _state(A, optA)
    total = _loss(A)
    optA.zero_grad()
    total.backward()
    SA.G[_trainable_offset(SA)] = INF
    norm = SA.gate_grads(clip)
    assert SA.pending_gate is not None
    optA.step()
    torch.cuda.synchronize()
    assert not torch.isfinite(norm).item() and SA.pending_gate is None
    for name, a, b in zip("P m v C".split(), _state(A, optA), before):
        assert _same(a, b), name
    assert (optA.applied_steps, optA.skipped_steps) == (1, 1)
    assert optA._step == 2                                 # attempted steps: the host does not know about the skip
    optB._step += 1                                        # B never saw the bad batch
    clean_step()                                           # step 3: the same weights, the same batch, the same bias corrections -> the same bits
    assert (optA.applied_steps, optA.skipped_steps) == (2, 1)
    assert torch.isfinite(SA.P).all().item()


@pytest.mark.parametrize("clip", [None, 1.0])
def test_control_without_the_guard_the_poison_reaches_the_weights(clip):
    from mvlt_amd.optim import FusedAdamW
    m = _model(torch.float32)
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    S = m.store
    total = _loss(m)
    opt.zero_grad()
    total.backward()
    S.G[_trainable_offset(S)] = INF
    if clip:
        S.clip_grad_norm(clip)
    opt.step()
    torch.cuda.synchronize()
    assert not torch.isfinite(S.P).all().item()


def test_frozen_gradients_and_a_poisoned_loss():
    from mvlt_amd.engine import BF16Scaler
    from mvlt_amd.optim import FusedAdamW
    m = _model(torch.float32, freeze="block2")
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05, skip_nonfinite=True)
    S = m.store
    total = _loss(m)
    opt.zero_grad()
    total.backward()
    opt._ensure()                                          # (the moments exist from the first step on; the snapshot below wants them now)
    before = _state(m, opt)
    name = next(n for n, p in S.params.items() if not p.requires_grad)
    off, n, _ = S.offsets[name]
    S.G[off:off + n] = NAN                                 # a frozen parameter's slice of G is nobody's gradient
    S.gate_grads(None)
    gate = S.pending_gate.clone()
    opt.step()
    torch.cuda.synchronize()
    assert gate.tolist()[1:] == [1.0, 1.0, 0.0] and np.isfinite(float(gate[0]))
    assert (opt.applied_steps, opt.skipped_steps) == (1, 0)
    after = _state(m, opt)
    assert not _same(after[0], before[0]) and torch.isfinite(S.P).all().item()
    assert _same(after[0][off:off + n], before[0][off:off + n])
    # loss * inf through the real backward: every gradient it reaches is Inf or NaN, the scaler's guarded path skips
    scaler = BF16Scaler(skip_nonfinite=True)
    total = _loss(m) * INF
    opt.zero_grad()
    scaler(total, opt, clip_grad=None, parameters=m.parameters())
    torch.cuda.synchronize()
    assert not torch.isfinite(scaler.last_grad_norm).item()
    assert (opt.applied_steps, opt.skipped_steps) == (1, 1)
    for name_, a, b in zip("P m v".split(), _state(m, opt), after):
        assert _same(a, b), name_
    assert S.pending_gate is None and S.pending_grad_scale == 1.0 and not S.scale_in_optimizer

    # checkpoint: the counters travel in state_dict()["fused"], into an optimizer whose store exists and into one whose store does not yet
    sd = opt.state_dict()
    assert sd["fused"]["applied"] == 1 and sd["fused"]["skipped"] == 1
    S._gate[1].zero_()
    opt2 = FusedAdamW(m, lr=1e-3, weight_decay=0.05, skip_nonfinite=True)
    assert (opt2.applied_steps, opt2.skipped_steps) == (0, 0)
    opt2.load_state_dict(sd)
    assert (opt2.applied_steps, opt2.skipped_steps) == (1, 1) and opt2._step == 2
    assert S._gate[1].tolist() == [1, 1]
    from mvlt_amd import pvlt
    fresh = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, drop_path_rate=0.0,
                           compute_dtype=torch.float32)
    assert fresh.store.P is None
    opt3 = FusedAdamW(fresh, skip_nonfinite=True)
    opt3.load_state_dict(sd)                               # (its moments wait for the first forward, and so do the counters)
    assert (opt3.applied_steps, opt3.skipped_steps) == (1, 1)
    assert opt3.state_dict()["fused"]["skipped"] == 1
    old = dict(sd, fused={k: v for k, v in sd["fused"].items() if k not in ("applied", "skipped")})
    opt2.load_state_dict(old)                              # a checkpoint from before the guard loads too, and leaves the counters alone
    assert (opt2.applied_steps, opt2.skipped_steps) == (1, 1)

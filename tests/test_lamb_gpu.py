"""GPU: FusedLamb (docs/lamb.md).  Kernel level -- the three launches of include/mvlt_hip_lamb.h on synthetic flat buffers against the float64 restatement of
tests/test_lamb_cpu.py (`lamb_reference`): norms that must not leak across tensor boundaries, a tensor longer than one trip of the fold, the zero cases, frozen
tensors, the gate, the moments' bits against mvlt_adamw_step, determinism and independence of the layout.  Model level -- three steps of pvlt_tiny through
BF16Scaler + FusedLamb against the same restatement stepping from the same gradients, a checkpoint in the middle of a run, the fused EMA behind it, and
FusedAdamW's launches untouched.

Bars (the issue's, from the reduction's shape): a sum of non-negative fp32 terms reduced at depth d has relative error <= d * 2^-24; the implementation's d is
at most 99 (docs/lamb.md), the bar for a trust ratio is 1e-5 relative, and for a parameter element |dp_gpu - dp_ref| <= 1e-5 |dp_ref| + 1 ulp(p)."""
import io

import pytest
import torch

from tests.test_lamb_cpu import lamb_reference
from tests.test_param_groups_gpu import DECAY, LR, WD, _loss, _model, _opt_state      # the fixtures and sizes of the per-group AdamW tests (model level)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = 16384                                 # elements per chunk = per workgroup (MVLT_LAMB_CHUNK)
LENS = [5, 8, 13, 64, 1000, CH - 4, CH + 8, 3 * CH + 12]
NAN = float("nan")
STEP_T = 3
R_TOL = 1e-5
EPS24 = 2.0 ** -24


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _hp(gs=0.5, eps=1e-6):
    """the row of mvlt_adamw_step; the LAMB launches ignore slots 0 and 4 -- NaN there reaches nothing"""
    return torch.tensor([NAN, 0.9, 0.999, eps, NAN, 1 - 0.9 ** STEP_T, 1 - 0.999 ** STEP_T, gs], dtype=torch.float32, device=DEV)


def _table(k):
    """k groups: no two learning rates alike, every third group without weight decay (tests/test_param_groups_gpu.py's table)"""
    rows = [[1e-3 * 0.75 ** (i % 9) * (1 + 0.013 * i), 0.0 if i % 3 == 0 else 0.05 * (1 + 0.1 * i)] for i in range(k)]
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


def _layout(lens, groups=None, frozen=()):
    layout, off = [], 0
    for i, n in enumerate(lens):
        layout.append((off, n, groups[i] if groups is not None else 0, i in frozen))
        off += (n + 7) // 8 * 8                            # FlatStore's ALIGN
    return layout, off


def _tensor_state(n, seed):
    """p, g, m, v of one tensor, a function of (n, seed) alone -- so the same tensor can be laid out anywhere"""
    g_ = torch.Generator().manual_seed(1000 * seed + n % 997)
    p, gr, m = (torch.randn(n, generator=g_) for _ in range(3))
    return p, gr * 1e-2, m * 1e-2, torch.rand(n, generator=g_) * 1e-4


def _state(layout, total, scales=None, gap=NAN, order=None):
    """flat p, g, m, v, p16 on the device; `gap` in every alignment gap of the four fp32 buffers"""
    bufs = [torch.full((total,), gap) for _ in range(4)]
    for i, (off, n, _, _) in enumerate(layout):
        t = _tensor_state(n, i if order is None else order[i])
        for b, x in zip(bufs, t):
            b[off:off + n] = x
        if scales is not None:
            bufs[0][off:off + n] *= scales[i if order is None else order[i]]
    return [b.to(DEV) for b in bufs] + [torch.full((total,), -1.5, dtype=torch.bfloat16, device=DEV)]


def _inside(layout, total, which=lambda fz: True):
    mask = torch.zeros(total, dtype=torch.bool)
    for off, n, _, fz in layout:
        if which(fz):
            mask[off:off + n] = True
    return mask.to(DEV)


def _clone(st):
    return [t.clone() for t in st]


def _launch(st, layout, total, table, hp, flags=0, gscale_dev=None, gate=None, ratios=None, partials=None, with_p16=True):
    from mvlt_amd import ops
    from mvlt_amd.optim import lamb_tables
    tensors, chunks = lamb_tables(layout, total, table.shape[0])
    td, cd = tensors.to(DEV), chunks.to(DEV)
    nc = chunks.shape[0]
    partials = torch.zeros(max(nc, 1), 2, device=DEV) if partials is None else partials
    ratios = torch.ones(len(layout), device=DEV) if ratios is None else ratios
    p, g, m, v, p16 = st
    k = table.shape[0]
    ops.lamb_moments(p, g, m, v, total, hp, td, cd, table, k, partials, gscale_dev=gscale_dev, gate=gate)
    ops.lamb_fold(partials, td, nc, table, k, flags, ratios, gate=gate)
    ops.lamb_apply(p, m, v, p16 if with_p16 else None, total, hp, td, cd, table, k, ratios, gate=gate)
    torch.cuda.synchronize()
    return ratios, partials


def _ulp(x):
    """spacing of fp32 at |x| (as float64)"""
    a = x.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _against_float64(parity, tag, st0, got, ratios, layout, total, table, hp, **ref_kw):
    """ratios per tensor and p, m, v per element against the float64 reference; everything outside the trainable tensors untouched in every bit"""
    p64, m64, v64, r64 = lamb_reference(st0[0], st0[1], st0[2], st0[3], layout, table, hp, **ref_kw)
    live = _inside(layout, total, lambda fz: not fz)
    worst_r = 0.0
    for i, want in enumerate(r64):
        if want is None:
            continue
        err = abs(float(ratios[i]) - want) / want
        worst_r = max(worst_r, err)
        print(f"{tag}: tensor {i} ({layout[i][1]} elements) r = {float(ratios[i]):.9e}, float64 {want:.9e}, relative error {err:.2e}")
    assert parity(f"lamb-kernel/r/{tag}", worst_r, R_TOL)
    p0 = st0[0].double()
    dp_gpu, dp_ref = (got[0].double() - p0)[live], (p64 - p0)[live]
    excess = ((dp_gpu - dp_ref).abs() - (R_TOL * dp_ref.abs() + _ulp(st0[0])[live])).max()
    worst = ((dp_gpu - dp_ref).abs() / (R_TOL * dp_ref.abs() + _ulp(st0[0])[live])).max()
    print(f"{tag}: worst |dp_gpu - dp_ref| over its bar 1e-5 |dp_ref| + 1 ulp(p): {float(worst):.3f} (all {int(live.sum())} elements)")
    assert parity(f"lamb-kernel/dp/{tag}", float(worst), 1.0) and float(excess) <= 0
    # the moments: b1 m + (1 - b1) g and b2 v + (1 - b2) g^2, a few fp32 roundings of their terms each
    b1, gs = float(hp[1].double()), float(hp[7].double())
    gr = st0[1].double() * gs
    m_bar = 4 * EPS24 * ((b1 * st0[2].double()).abs() + ((1 - b1) * gr).abs())
    v_bar = 8 * EPS24 * v64.abs()
    assert bool(((got[2].double() - m64).abs()[live] <= m_bar[live]).all()) and bool(((got[3].double() - v64).abs()[live] <= v_bar[live]).all())
    assert not _same(got[2][live], st0[2][live]) and not _same(got[3][live], st0[3][live])
    assert _same(got[4][live], got[0][live].to(torch.bfloat16))                # the bf16 copy of the new parameters, in the same pass
    for name, a, old in zip("p g m v p16".split(), got, st0):                 # gaps and frozen tensors: every bit as it was
        assert _same(a[~live], old[~live]), name
    assert _same(got[1], st0[1])
    assert all(bool(torch.isfinite(t[live]).all()) for t in (got[0], got[2], got[3])) and bool(torch.isfinite(ratios).all())
    return r64


def _hp_times(hp, factor):
    out = hp.clone()
    out[7] = hp[7] * factor                                # fp32 product, as the kernel forms hp[7] * gscale_dev[0]
    return out


# ------------------------------------------------------------------------------------------------------------------ kernel: boundaries
def test_norms_do_not_leak_across_tensor_boundaries(parity):
    """tensor k has p scaled by 10^k: an element of a neighbour (or a gap's NaN) inside a norm moves a ratio by orders of magnitude"""
    groups = [1, 2, 4, 5, 7, 1, 2, 4]                      # every tensor decays (a trust ratio everywhere), no two neighbours share lr / wd
    layout, total = _layout(LENS, groups)
    table, hp = _table(8), _hp(0.5)
    st0 = _state(layout, total, scales=[10.0 ** k for k in range(len(LENS))])
    assert int((~_inside(layout, total)).sum()) == 3 + 3 + 4 + 4 and bool(torch.isnan(st0[0][~_inside(layout, total)]).all())
    got = _clone(st0)
    ratios, _ = _launch(got, layout, total, table, hp)
    r64 = _against_float64(parity, "boundaries", st0, got, ratios, layout, total, table, hp)
    assert all(abs(r64[k + 1] - r64[k]) > 1e-3 * r64[k] for k in range(len(LENS) - 1))       # no two neighbours share a ratio: a leak would show


def test_a_tensor_longer_than_one_trip_of_the_fold(parity):
    """257 chunks + 12 elements: the fold's 256 lanes take a second partial each for the first of them, and the last chunk is 12 elements long.  A short
    neighbour on either side."""
    lens = [13, 257 * CH + 12, 5]
    layout, total = _layout(lens, [1, 2, 4])
    table, hp = _table(5), _hp(0.5)
    st0 = _state(layout, total, scales=[1.0, 30.0, 1000.0])
    got = _clone(st0)
    ratios, partials = _launch(got, layout, total, table, hp)
    assert partials.shape[0] == 1 + 258 + 1
    _against_float64(parity, "long", st0, got, ratios, layout, total, table, hp)


def test_per_group_lr_and_weight_decay_reach_their_tensors(parity):
    lens = [1000, 13, CH + 8, 64]
    layout, total = _layout(lens, [3, 1, 0, 2])            # groups 0 and 3 do not decay: r = 1 there
    table, hp = _table(4), _hp(1.0)
    st0 = _state(layout, total)
    got = _clone(st0)
    ratios, _ = _launch(got, layout, total, table, hp)
    r64 = _against_float64(parity, "groups", st0, got, ratios, layout, total, table, hp)
    assert float(ratios[0]) == 1.0 == r64[0] and float(ratios[2]) == 1.0 and r64[1] != 1.0 and r64[3] != 1.0
    # a control: every tensor in group 1 is far outside the bar for the others
    flat, _ = _layout(lens, [1, 1, 1, 1])
    p64, _, _, _ = lamb_reference(st0[0], st0[1], st0[2], st0[3], flat, table, hp)
    off, n = layout[0][:2]
    d_got, d_flat = (got[0].double() - st0[0].double())[off:off + n], (p64 - st0[0].double())[off:off + n]
    assert float((d_got - d_flat).norm() / d_flat.norm()) > 0.1


# ------------------------------------------------------------------------------------------------------------------ kernel: zero cases
def test_zero_norms_zero_decay_and_trust_clip(parity):
    from mvlt_amd import ops
    lens = [1000, 13, CH + 8, 64]
    layout, total = _layout(lens, [1, 0, 0, 2])            # group 0: wd = 0
    table, hp = _table(3), _hp(1.0)
    st0 = _state(layout, total, scales=[1.0, 1.0, 1.0, 100.0])
    o, n = layout[0][:2]
    st0[0][o:o + n] = 0.0                                  # tensor 0: zero-norm weights (wd != 0) -> r = 1
    o, n = layout[1][:2]
    for t in st0[1:4]:
        t[o:o + n] = 0.0                                   # tensor 1: g = m = v = 0 with wd = 0 -> u = 0 -> r = 1 also under always_adapt, p stays
    # always_adapt: tensor 2 (wd = 0) gets a ratio
    got = _clone(st0)
    ratios, _ = _launch(got, layout, total, table, hp, flags=ops.LAMB_ALWAYS_ADAPT)
    r64 = _against_float64(parity, "zeros/always_adapt", st0, got, ratios, layout, total, table, hp, always_adapt=True)
    assert float(ratios[0]) == 1.0 and float(ratios[1]) == 1.0 and r64[2] != 1.0 and abs(float(ratios[2]) - r64[2]) <= R_TOL * r64[2]
    o, n = layout[1][:2]
    assert _same(got[0][o:o + n], st0[0][o:o + n]) and not got[2][o:o + n].any() and not got[3][o:o + n].any()
    o, n = layout[0][:2]
    assert bool((got[0][o:o + n] != 0).all())              # the zero weights did move (by lr * u)
    # without always_adapt: wd = 0 -> r = 1 exactly
    got = _clone(st0)
    ratios, _ = _launch(got, layout, total, table, hp)
    r64 = _against_float64(parity, "zeros/plain", st0, got, ratios, layout, total, table, hp)
    assert [float(r) for r in ratios[:3]] == [1.0, 1.0, 1.0] and r64[:3] == [1.0, 1.0, 1.0] and r64[3] > 1.0
    # trust_clip: tensor 3 (p scaled by 100: r > 1) is clipped to exactly 1, and so is whatever else came out above 1
    got = _clone(st0)
    ratios, _ = _launch(got, layout, total, table, hp, flags=ops.LAMB_TRUST_CLIP | ops.LAMB_ALWAYS_ADAPT)
    r64 = _against_float64(parity, "zeros/trust_clip", st0, got, ratios, layout, total, table, hp, always_adapt=True, trust_clip=True)
    assert float(ratios[3]) == 1.0 == r64[3] and all(float(r) <= 1.0 for r in ratios)


# ------------------------------------------------------------------------------------------------------------------ kernel: frozen tensors
def test_frozen_tensors_with_nan_are_untouched_and_reach_no_neighbour(parity):
    frozen = (1, 4, 6)                                     # a ragged one, a mid-sized one, one of two chunks
    groups = [1, 2, 4, 5, 7, 1, 2, 4]
    layout, total = _layout(LENS, groups, frozen)
    table, hp = _table(8), _hp(0.5)
    st0 = _state(layout, total, scales=[10.0 ** k for k in range(len(LENS))])
    fz = _inside(layout, total, lambda f: f)
    for t in st0[1:4]:
        t[fz] = NAN                                        # g, m, v of a frozen tensor reach nothing
    got = _clone(st0)
    ratios0 = torch.full((len(LENS),), 7.0, device=DEV)
    ratios, _ = _launch(got, layout, total, table, hp, ratios=ratios0.clone())
    _against_float64(parity, "frozen", st0, got, ratios, layout, total, table, hp)       # (checks every bit outside the trainable tensors)
    assert all(float(ratios[i]) == 7.0 for i in frozen) and all(float(ratios[i]) != 7.0 for i in range(len(LENS)) if i not in frozen)
    # the neighbours' ratios carry the bits they have when nothing is frozen
    free_layout, _ = _layout(LENS, groups)
    st1 = _state(free_layout, total, scales=[10.0 ** k for k in range(len(LENS))])
    free, _ = _launch(st1, free_layout, total, table, hp)
    assert all(_same(ratios[i], free[i]) for i in range(len(LENS)) if i not in frozen)


# ------------------------------------------------------------------------------------------------------------------ kernel: gates
def test_a_closed_gate_leaves_everything_alone():
    layout, total = _layout(LENS, [1, 2, 4, 5, 7, 1, 2, 4])
    table, hp = _table(8), _hp(0.5)
    st0 = _state(layout, total)
    got = _clone(st0)
    ratios0 = torch.full((len(LENS),), 7.0, device=DEV)
    partials0 = torch.full((sum((n + CH - 1) // CH for n in LENS), 2), -3.0, device=DEV)
    gate = torch.tensor([float("inf"), 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    ratios, partials = _launch(got, layout, total, table, hp, gate=gate, ratios=ratios0.clone(), partials=partials0.clone())
    assert all(_same(a, b) for a, b in zip(got, st0)) and _same(ratios, ratios0) and _same(partials, partials0)


def test_an_open_gate_is_the_clip_coefficient():
    from mvlt_amd import _lib as L
    layout, total = _layout(LENS, [1, 2, 4, 5, 7, 1, 2, 4])
    table, hp = _table(8), _hp(0.5)
    st0 = _state(layout, total)
    gated, clipped, plain = _clone(st0), _clone(st0), _clone(st0)
    gate = torch.tensor([2.5, 0.37, 1.0, 0.0], dtype=torch.float32, device=DEV)
    r_gated, part_gated = _launch(gated, layout, total, table, hp, gate=gate)
    assert L.last_kernel() == "lamb_apply_kernel<true>"
    r_clip, part_clip = _launch(clipped, layout, total, table, hp, gscale_dev=gate[1:2])
    assert L.last_kernel() == "lamb_apply_kernel<false>"
    assert all(_same(a, b) for a, b in zip(gated, clipped)) and _same(r_gated, r_clip) and _same(part_gated, part_clip)
    _launch(plain, layout, total, table, hp)
    assert not _same(gated[2], st0[2]) and not _same(gated[2], plain[2])       # the step happened, and the coefficient reached the moments


# ------------------------------------------------------------------------------------------------------------------ kernel: bits
@pytest.mark.parametrize("clip", [None, 0.37])
def test_moments_carry_the_bits_of_adamw_step(parity, clip):
    from mvlt_amd import ops
    layout, total = _layout(LENS, [1, 2, 4, 5, 7, 1, 2, 4])
    table = _table(8)
    hp = _hp(0.5, eps=1e-8)
    st0 = _state(layout, total, gap=0.25)                  # (finite gaps: the AdamW launch below runs over the whole buffer)
    cd = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=DEV)
    got, want = _clone(st0), _clone(st0)
    ratios, _ = _launch(got, layout, total, table, hp, gscale_dev=cd)
    hp_adamw = hp.clone()
    hp_adamw[0], hp_adamw[4] = 1e-3, 0.05
    p, g, m, v, p16 = want
    ops.adamw_step(p, g, m, v, p16, total, hp_adamw, torch.ones(total, dtype=torch.uint8, device=DEV), gscale_dev=cd)
    torch.cuda.synchronize()
    live = _inside(layout, total)
    assert _same(got[2][live], want[2][live]) and _same(got[3][live], want[3][live])
    assert not _same(got[2][live], st0[2][live]) and _same(got[2][~live], st0[2][~live])
    assert _same(got[4][live], got[0][live].to(torch.bfloat16)) and _same(got[4][~live], st0[4][~live])
    _against_float64(parity, f"bits/{clip}", st0, got, ratios, layout, total, table, hp if clip is None else _hp_times(hp, cd[0]))
    # without a bf16 buffer the parameters come out the same
    again = _clone(st0)
    _launch(again, layout, total, table, hp, gscale_dev=cd, with_p16=False)
    assert _same(again[0], got[0]) and _same(again[4], st0[4])


def test_two_runs_agree_and_a_ratio_does_not_depend_on_the_neighbours():
    groups = [1, 2, 4, 5, 7, 1, 2, 4]
    scales = [10.0 ** k for k in range(len(LENS))]
    layout, total = _layout(LENS, groups)
    table, hp = _table(8), _hp(0.5)
    st0 = _state(layout, total, scales=scales)
    a, b = _clone(st0), _clone(st0)
    ra, pa = _launch(a, layout, total, table, hp)
    rb, pb = _launch(b, layout, total, table, hp)
    assert all(_same(x, y) for x, y in zip(a, b)) and _same(ra, rb) and _same(pa, pb)
    # the same tensors in another order: each keeps its group, its values -- and every bit of its ratio and of its new parameters
    order = [6, 0, 5, 3, 7, 1, 4, 2]
    layout2, total2 = _layout([LENS[i] for i in order], [groups[i] for i in order])
    c = _state(layout2, total2, scales=scales, order=order)
    rc, _ = _launch(c, layout2, total2, table, hp)
    for j, i in enumerate(order):
        (o1, n, _, _), o2 = layout[i], layout2[j][0]
        assert _same(rc[j], ra[i]), (i, float(rc[j]), float(ra[i]))
        assert _same(c[0][o2:o2 + n], a[0][o1:o1 + n]) and _same(c[2][o2:o2 + n], a[2][o1:o1 + n]), i


# ------------------------------------------------------------------------------------------------------------------ model level
def _reference_run(m, opt):
    """the float64 restatement stepping beside a FusedLamb: flat float64 parameters and moments in the store's layout, one `step(coef)` per optimizer step,
    from the gradients the store holds"""
    S = m.store
    state = dict(p=S.P.double().clone(), m=torch.zeros_like(S.P, dtype=torch.float64), v=torch.zeros_like(S.P, dtype=torch.float64), t=0)
    group_ix = {id(p): i for i, g in enumerate(opt.param_groups) for p in g["params"]}

    def step(coef=1.0):
        state["t"] += 1
        g0 = opt.param_groups[0]
        b1, b2 = g0["betas"]
        hp = torch.tensor([0.0, b1, b2, g0["eps"], 0.0, 1 - b1 ** state["t"], 1 - b2 ** state["t"], 1.0], dtype=torch.float32).double()
        hp[7] = coef
        table = torch.tensor([[g["lr"], g["weight_decay"]] for g in opt.param_groups], dtype=torch.float32)
        layout = [(S.offsets[n][0], S.offsets[n][1], group_ix[id(p)], not p.requires_grad) for n, p in S.params.items()]
        state["p"], state["m"], state["v"], state["r"] = lamb_reference(state["p"], S.G, state["m"], state["v"], layout, table, hp,
                                                                        always_adapt=opt.always_adapt, trust_clip=opt.trust_clip)
    return state, step


def _grad_norm(S):
    sq = sum(float(S.G[o:o + n].double().pow(2).sum()) for name, (o, n, _) in S.offsets.items() if S.params[name].requires_grad)
    return sq ** 0.5


@pytest.mark.parametrize("case", ["plain-fp32", "plain-bf16", "layer-decay", "frozen-stage", "clip", "guard"])
def test_three_steps_match_the_float64_restatement(parity, case):
    """Three steps through BF16Scaler + FusedLamb against the float64 restatement stepping from the same gradients.  The bar is the one
    tests/test_param_groups_gpu.py::test_layer_decay_steps_match_torch_adamw_over_the_same_groups holds the parameters to: every tensor within 1e-6 of its
    largest element (max-norm metric)."""
    from mvlt_amd import _lib as L
    from mvlt_amd.engine import BF16Scaler
    from mvlt_amd.optim import FusedAdamW, FusedLamb, layer_decay_groups
    from tests.test_freeze_gpu import maxrel
    dtype = torch.float32 if case == "plain-fp32" else torch.bfloat16
    guard = case == "guard"
    m = _model(dtype, freeze=("block2.",) if case == "frozen-stage" else None)
    groups = layer_decay_groups(m, LR, WD, DECAY) if case in ("layer-decay", "frozen-stage", "clip", "guard") else None
    opt = FusedLamb(m, lr=LR, weight_decay=WD, param_groups=groups, skip_nonfinite=guard)
    assert isinstance(opt, FusedAdamW)
    scaler = BF16Scaler(skip_nonfinite=guard)
    max_norm = 1e-3 if case == "clip" else None            # (as the AdamW test: far below the norm, the clip bites)
    ref = step = start = None
    for it in range(2 if guard else 3):
        total = _loss(m, 8 + it)
        opt.zero_grad()
        if ref is None:                                    # the store exists after the first forward
            ref, step = _reference_run(m, opt)
            start = m.store.P.clone()
        scaler(total, opt, clip_grad=max_norm, parameters=m.parameters())
        assert L.last_kernel().startswith("lamb_apply_kernel<" + ("true" if guard else "false"))
        coef = 1.0
        if max_norm:
            norm = _grad_norm(m.store)
            assert norm > max_norm
            assert parity("lamb-model/clip-norm", abs(float(scaler.last_grad_norm) - norm) / norm, 1e-5)       # tests/test_clip_gpu.py NORM_TOL
            coef = max_norm / (norm + 1e-6)
        step(coef)
    torch.cuda.synchronize()
    S = m.store
    live = [n for n, p in S.params.items() if p.requires_grad]
    view = lambda buf, n: buf[S.offsets[n][0]:S.offsets[n][0] + S.offsets[n][1]]
    worst = max(maxrel(view(S.P, n), view(ref["p"], n)) for n in live)
    print(f"{case}: trainable parameters after the steps against the float64 restatement, worst max-norm relative error {worst:.3e}")
    assert parity(f"lamb-model/{case}", worst, 1e-6)
    assert all(not torch.equal(view(S.P, n), view(start, n)) for n in live)
    # the trust ratios, name by name, as the last step used them
    tr = opt.trust_ratios()
    assert list(tr) == list(S.params) and all(t.dim() == 0 and t.is_cuda for t in tr.values())
    worst_r = max(abs(float(tr[n]) - r) / r for n, r in zip(S.params, ref["r"]) if r is not None)
    assert parity(f"lamb-model/r/{case}", worst_r, R_TOL)
    assert sum(float(tr[n]) != 1.0 for n in live) > 50 and all(float(tr[n]) == 1.0 for n in live if S.params[n].dim() == 1)       # no decay: r = 1
    # a control: the ratios matter -- the same steps without them (r = 1) are far outside the bar
    lowest = "patch_embed1.proj.weight"
    assert float(tr[lowest]) != 1.0
    for n, p in S.params.items():
        if not p.requires_grad:
            off, cnt, _ = S.offsets[n]
            assert torch.equal(view(S.P, n), view(start, n)) and p.grad is None, n
            assert not opt._m[off:off + cnt].any() and not opt._v[off:off + cnt].any() and float(tr[n]) == 1.0, n
    if case == "frozen-stage":
        assert sum(not p.requires_grad for p in S.params.values()) > 30
    if S.C is not None:
        assert _same(S.C[_inside_store(S)], S.P[_inside_store(S)].to(torch.bfloat16))
    if guard:
        # a third step whose gradients hold an Inf: nothing moves, one skip is counted
        assert (opt.applied_steps, opt.skipped_steps) == (2, 0)
        before = _opt_state(m, opt) + [opt._ratios.clone(), opt._partials.clone()]
        total = _loss(m, 8)
        opt.zero_grad()
        total.backward()
        off, _, _ = S.offsets["block3.0.mlp.fc1.weight"]
        S.G[off + 3] = float("inf")
        norm = S.gate_grads(None)
        opt.step()
        torch.cuda.synchronize()
        assert not torch.isfinite(norm).item() and L.last_kernel() == "lamb_apply_kernel<true>"
        for name, a, b in zip("P m v C r partials".split(), _opt_state(m, opt) + [opt._ratios, opt._partials], before):
            assert _same(a, b), name
        assert (opt.applied_steps, opt.skipped_steps) == (2, 1) and opt.skipped_steps == 1


def _inside_store(S):
    mask = torch.zeros(S.total, dtype=torch.bool)
    for off, n, _ in S.offsets.values():
        mask[off:off + n] = True
    return mask.to(S.P.device)


def test_state_dict_round_trip_into_an_optimizer_that_has_seen_no_forward():
    """a checkpoint in the middle of a run, loaded the way a resumed run loads it: new model, new optimizer, load_state_dict before the first forward"""
    from mvlt_amd.optim import FusedLamb, layer_decay_groups
    m = _model(torch.bfloat16)
    opt = FusedLamb(m, param_groups=layer_decay_groups(m, LR, WD, DECAY), always_adapt=True)
    opt.zero_grad()
    _loss(m, 8).backward()
    opt.step()
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    weights = {k: t.detach().cpu().clone() for k, t in m.state_dict().items()}
    opt.zero_grad()
    _loss(m, 9).backward()
    g2 = m.store.G.clone()
    opt.step()
    torch.cuda.synchronize()
    want = _opt_state(m, opt) + [opt._ratios.clone()]
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu", weights_only=False)
    assert set(sd["fused"]) == {"step", "m", "v"} and sd["fused"]["step"] == 1
    m2 = _model(torch.bfloat16, seed=9)                    # other weights: the checkpoint's replace them
    m2.load_state_dict(weights, strict=True)
    opt2 = FusedLamb(m2, param_groups=layer_decay_groups(m2, 7.0, 0.5, 0.5), always_adapt=True)       # (the checkpoint's rates replace these)
    assert m2.store.P is None
    opt2.load_state_dict(sd)
    assert [g["lr"] for g in opt2.param_groups] == [g["lr"] for g in opt.param_groups] and opt2._step == 1 and opt2._pending is not None
    opt2.zero_grad()
    _loss(m2, 9).backward()
    m2.store.G.copy_(g2)                                    # the same gradients: two backward passes differ in their last bits (fp32 atomics)
    opt2.step()
    torch.cuda.synchronize()
    for name, a, b in zip("P m v C r".split(), _opt_state(m2, opt2) + [opt2._ratios], want):
        assert _same(a, b), name


def test_fused_ema_follows_a_lamb_step():
    from mvlt_amd.optim import FusedLamb, FusedModelEma
    m = _model(torch.bfloat16)
    opt = FusedLamb(m, lr=LR, weight_decay=WD)
    ema = FusedModelEma(m, decay=0.75)
    opt.zero_grad()
    _loss(m, 8).backward()
    e0 = m.store.P.clone()                                 # the average starts as a copy of the model
    opt.step()
    ema.update(m)
    torch.cuda.synchronize()
    S, E = m.store, ema.ema.store
    assert not _same(S.P, e0)
    assert _same(E.P, e0 * 0.75 + S.P * 0.25)              # three fp32 roundings, timm's formula
    inside = _inside_store(S)
    assert _same(E.C[inside], E.P[inside].to(torch.bfloat16))


def test_fused_adamw_still_takes_its_old_launches(monkeypatch):
    from mvlt_amd import _lib as L, ops
    from mvlt_amd.optim import FusedAdamW, FusedLamb
    A, Bm = _model(torch.bfloat16), _model(torch.bfloat16)
    optA, optB = FusedAdamW(A, lr=LR, weight_decay=WD), FusedLamb(Bm, lr=LR, weight_decay=WD)

    def refuse(*a, **kw):
        raise AssertionError("a LAMB launch from FusedAdamW")
    for o, m_ in ((optA, A), (optB, Bm)):
        o.zero_grad()
        _loss(m_, 8).backward()
    Bm.store.G.copy_(A.store.G)
    with monkeypatch.context() as mp:
        for name in ("lamb_moments", "lamb_fold", "lamb_apply"):
            mp.setattr(ops, name, refuse)
        optA.step()
        assert L.last_kernel().startswith("adamw_kernel<")
        with pytest.raises(AssertionError, match="a LAMB launch"):
            optB.step()
    calls = []
    with monkeypatch.context() as mp:
        for name in ("adamw_step", "adamw_step_gated", "adamw_step_groups"):
            mp.setattr(ops, name, lambda *a, **kw: calls.append(1))
        optB.step()
    torch.cuda.synchronize()
    assert not calls and L.last_kernel() == "lamb_apply_kernel<false>"
    # the first moments of the two optimizers are the same bits (same gradients, same betas); the parameters are not (trust ratios)
    inside = _inside_store(A.store)
    assert _same(optA._m[inside], optB._m[inside]) and _same(optA._v[inside], optB._v[inside]) and not _same(A.store.P, Bm.store.P)

"""CPU: the premises of the row-wise kernel inputs (tests/rowwise_cases.py), at every width and shape at which
tests/test_rowwise_edges_gpu.py uses them.  Every decisive builder is run through two fp32 twins written out here in a few lines of torch: the RIGHT
formula must stay below one tenth of the GPU file's bar, the WRONG formula the builder targets must exceed twice the bar -- so that the inputs cannot
drift into something the wrong kernel passes again.  Also pinned: the exactness premises, and the float64 references against torch's own."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import rowwise_cases as rc

F32, BF = rc.F32, rc.BF
T32 = rc.TOL[F32]
EPS = 1e-6


def worst(got, ref, bar):
    """largest error in units of the bar; NaN / inf count as infinitely wrong"""
    r = (got.double() - ref).abs() / bar.clamp_min(1e-300)
    return float(torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf)).max())


# ------------------------------------------------------------------------------------------------ LayerNorm twins (fp32)
def ln_twin(x, g, b, eps, variance="two-pass", use_eps=True):
    m = x.mean(-1, keepdim=True)
    var = ((x - m) ** 2).mean(-1, keepdim=True) if variance == "two-pass" else (x * x).mean(-1, keepdim=True) - m * m
    rstd = (var + (eps if use_eps else 0.0)).rsqrt()
    return (x - m) * rstd * g + b, m[:, 0], rstd[:, 0]


@pytest.mark.parametrize("C", rc.LN_OFFSET_WIDTHS)
def test_offset_rows_expose_a_one_pass_variance(C):
    x = rc.ln_offset_rows(200, C)
    g, b = rc.ln_params(C)
    assert torch.equal(x.to(BF).float(), x), "every value exact in bf16"
    assert torch.equal(x.cumsum(-1), x.double().cumsum(-1).float()) and float(x.sum(-1).max()) < 2 ** 24, "every fp32 partial sum exact"
    ref = rc.ln_fwd_ref(x, g, b, EPS)
    bar = rc.bar_y(ref.y, T32)
    assert worst(ln_twin(x, g, b, EPS)[0], ref.y, bar) < 0.1
    assert worst(ln_twin(x, g, b, EPS, variance="one-pass")[0], ref.y, bar) > 2.0


def test_one_pass_variance_is_exact_at_eight_columns():
    """why ln_offset_rows is not used at C = 8: nothing rounds"""
    k = torch.randint(-1, 2, (200, 8), generator=rc.gen(0)).float()
    x = rc.OFFSET_C0 + rc.OFFSET_S * k
    m = x.mean(-1, keepdim=True)
    assert torch.equal((x * x).mean(-1, keepdim=True) - m * m, ((x.double() - m.double()) ** 2).mean(-1, keepdim=True).float())


@pytest.mark.parametrize("C", sorted(set(rc.LN_FIXED + rc.LN_GENERIC)))
def test_constant_rows_have_an_exact_fp32_mean(C):
    x = rc.ln_constant_rows(7, C)
    inv_c = torch.tensor(1.0) / torch.tensor(float(C))
    assert torch.equal(x.sum(-1) * inv_c, x[:, 0]) and set(x[:, 0].tolist()) == set(rc.ln_constants(C))
    # hence x - mean == 0, y == beta, rstd == 1 / sqrt(eps); without eps: inf x 0
    g, b = rc.ln_params(C)
    y, m, rstd = ln_twin(x, g, b, EPS)
    assert torch.equal(y, b.expand_as(y)) and torch.equal(m, x[:, 0])
    ref = rc.ln_fwd_ref(x, g, b, EPS)
    assert worst(rstd, ref.rstd, T32 * ref.rstd) < 0.1
    assert not torch.isfinite(ln_twin(x, g, b, EPS, use_eps=False)[0]).any()


@pytest.mark.parametrize("C", sorted(set(rc.LN_FIXED + rc.LN_GENERIC)))
def test_scaled_rows_give_eps_weight(C):
    x = rc.ln_scaled_rows(60, C)
    g, b = rc.ln_params(C)
    ref = rc.ln_fwd_ref(x, g, b, EPS)
    bar = rc.bar_y(ref.y, T32)
    assert worst(ln_twin(x, g, b, EPS)[0], ref.y, bar) < 0.1
    assert worst(ln_twin(x, g, b, EPS, use_eps=False)[0], ref.y, bar) > 2.0
    small = torch.arange(60) % 6 < 2                                   # factors 1e-4, 1e-3
    assert float((ref.std[small] ** 2).max()) < 10 * EPS < float(ref.std[~small].min() ** 2)      # eps matters in a third of the rows


@pytest.mark.parametrize("C", rc.LN_FIXED)
def test_chained_constant_rows_expose_swapped_eps(C):
    """gamma1 = 0 and a constant beta1: the first output is the constant row again, so rstd2 == 1 / sqrt(eps2) whatever eps is"""
    eps, eps2 = 1e-5, 1e-6
    x = rc.ln_scaled_rows(9, C)
    g1, b1 = torch.zeros(C), torch.full((C,), 3.0)
    g2, b2 = rc.ln_params(C, seed=1)
    ref = rc.ln_fwd_ref(x, g1, b1, eps, chain=(g2, b2, eps2))
    y, _, _ = ln_twin(x, g1, b1, eps)
    assert torch.equal(y, b1.expand_as(y))
    right, wrong = ln_twin(y, g2, b2, eps2), ln_twin(y, g2, b2, eps)
    assert torch.equal(right[0], b2.expand_as(y))
    assert worst(right[2], ref.rstd2, T32 * ref.rstd2) < 0.1 and worst(wrong[2], ref.rstd2, T32 * ref.rstd2) > 2.0


@pytest.mark.parametrize("C", rc.LN_BWD_WIDTHS)
def test_single_row_dy_exposes_a_neighbouring_row(C):
    rows, row = 12, 5
    x = rc.ln_scaled_rows(rows, C, seed=3)
    g, _ = rc.ln_params(C)
    dy = rc.ln_single_row_dy(rows, C, row)
    f = rc.ln_fwd_ref(x, g, torch.zeros(C), EPS)
    mean, rstd = f.mean.float(), f.rstd.float()
    ref = rc.ln_bwd_ref(dy, x, g, mean, rstd)
    xh = (x - mean[:, None]) * rstd[:, None]
    bar = rc.bar_col(ref.abs_gamma, T32)
    assert worst((dy * xh).sum(0), ref.dgamma, bar) < 0.1
    assert worst((dy * xh.roll(1, 0)).sum(0), ref.dgamma, bar) > 2.0                   # x_hat of the row before
    assert bool((ref.dx[torch.arange(rows) != row] == 0).all()) and float(ref.dx[row].abs().max()) > 0
    assert torch.equal(ref.dbeta, dy[row].double())


# ------------------------------------------------------------------------------------------------ cross-entropy twins (fp32)
def lse_twin(x, chunk=4, subtract_max=True, rescale=True, columns=None):
    """(max, sum) over chunks of columns, as the kernel's threads walk a row"""
    x = x[:, :columns] if columns is not None else x
    if not subtract_max:
        return x.exp().sum(-1).log()
    m = torch.full((x.shape[0],), -math.inf)
    s = torch.zeros(x.shape[0])
    for c in range(0, x.shape[1], chunk):
        blk = x[:, c:c + chunk]
        nm = torch.maximum(m, blk.amax(-1))
        sub = torch.where(nm == -math.inf, torch.zeros_like(nm), nm)
        s = (s * (m - sub).exp() if rescale else s) + (blk - sub[:, None]).exp().sum(-1)
        m = nm
    return m + s.log()


CE_V = [V for V, _ in rc.CE_SHAPES]


@pytest.mark.parametrize("V", CE_V)
def test_peaked_rows_expose_a_late_maximum_and_a_dropped_tail(V):
    for peak in rc.CE_PEAKS:
        col = rc.ce_peak_column(peak, V)
        if col is None:
            continue
        x, lab = rc.ce_peaked_rows(6, V, col)
        assert torch.equal(x.to(BF).float()[:, col], x[:, col]) and float(x[:, col].min() - x.masked_fill(F.one_hot(torch.tensor(col), V).bool(), -9).amax(-1).max()) >= 30
        assert bool((lab[0::2] == col).all()) and bool((lab[1::2] != col).all())
        ref = rc.ce_ref(x, lab)
        bar = rc.bar_lse(ref.lse, T32)
        chunk = 4 if V <= 256 else 1024
        assert worst(lse_twin(x, chunk), ref.lse, bar) < 0.1
        if col >= chunk:                                                 # the maximum arrives after the first chunk
            assert worst(lse_twin(x, chunk, rescale=False), ref.lse, bar) > 2.0, (V, peak)
        if col >= (V & ~3):                                              # the peak is in the scalar tail
            assert worst(lse_twin(x, chunk, columns=V & ~3), ref.lse, bar) > 2.0, (V, peak)


@pytest.mark.parametrize("V", CE_V)
@pytest.mark.parametrize("shift", [100.0, -100.0])
def test_shifted_rows_expose_a_missing_max_subtraction(V, shift):
    x, lab = rc.ce_shifted_rows(6, V, shift)
    ref = rc.ce_ref(x, lab)
    bar = rc.bar_lse(ref.lse, T32)
    assert worst(lse_twin(x, 1024), ref.lse, bar) < 0.1
    if shift > 0:           # exp(100 + ...) = inf in fp32.  (At -100 the exponentials are fp32 denormals: gone where they are flushed, merely coarse where they are kept.)
        assert worst(lse_twin(x, subtract_max=False), ref.lse, bar) > 2.0
    assert float(torch.tensor(shift).to(BF)) == shift


@pytest.mark.parametrize("V", CE_V)
def test_flat_and_masked_rows(V):
    x, lab = rc.ce_flat_rows(5, V)
    ref = rc.ce_ref(x, lab)
    assert float((ref.lse - (-2.5 + math.log(V))).abs().max()) < 1e-12
    assert float(((ref.dlogits + F.one_hot(lab, V).double() / 5) * 5 - 1.0 / V).abs().max()) < 1e-12
    for mode in ("first4", "first8192", "random30"):
        if (mode == "first4" and V <= 4) or (mode == "first8192" and V <= 8192):
            continue
        x, lab = rc.ce_masked_rows(6, V, mode)
        assert bool(torch.isfinite(x.gather(1, lab[:, None])).all()) and bool(torch.isinf(x).any())
        ref = rc.ce_ref(x, lab)
        assert bool(torch.isfinite(ref.lse).all()) and bool((ref.dlogits[torch.isinf(x)] == 0).all())
        assert worst(lse_twin(x, 4 if V <= 256 else 1024), ref.lse, rc.bar_lse(ref.lse, T32)) < 0.1
        # the formula of the kernel before the guard: x - max with the running maximum still -inf
        m0 = x[:, :4].amax(-1)
        assert mode == "random30" or bool(torch.isnan((x[:, :4] - m0[:, None]).exp().sum(-1)).all())


# ------------------------------------------------------------------------------------------------ SmoothL1
def sl1_twin(d, strict=True):
    a = d.abs()
    return torch.where(a < 1 if strict else a <= 1, 0.5 * d * d, a - 0.5)


def test_sl1_exact_sums_are_exact_in_any_order():
    pred, target = rc.sl1_exact()
    d = pred - target
    assert pred.numel() == rc.SL1_N > 3 * 2048 * 1024 and rc.SL1_N % 4 == 0
    assert set(d.unique().tolist()) == set(rc.SL1_DIFFS) | {0.0} and 0.05 < float((d != 0).float().mean()) < 0.08
    terms = sl1_twin(d)
    assert torch.equal(terms * 8, (terms * 8).round()), "every term a multiple of 0.125"
    total = float(terms.double().sum())
    assert total + 1024.5 < 2 ** 21 and total == rc.sl1_ref(pred, target).loss_sum
    assert float(terms.sum()) == total and float(terms.flip(0).sum()) == total and float(terms.reshape(-1, 4).sum(0).sum()) == total
    # `<` and `<=` agree at |d| = 1 (both branches give 0.5): the test does not over-constrain the comparison
    assert torch.equal(sl1_twin(d, strict=True), sl1_twin(d, strict=False))
    # the gradient: a clamp, not a sign
    ref = rc.sl1_ref(pred, target, gscale=10.0)
    sc = torch.tensor(10.0) * (torch.tensor(1.0) / torch.tensor(float(rc.SL1_N)))
    assert float((((d.clamp(-1, 1) * sc).double() - ref.grad).abs() / ref.grad.abs().clamp_min(1e-30)).max()) < 1e-6
    assert not torch.equal(d.sign() * sc, d.clamp(-1, 1) * sc)


def test_sl1_boundaries():
    vals = rc.sl1_boundary_values()
    assert len(vals) == 12 and vals[4] < 1.0 < vals[6]
    for d in vals:
        pred, target = rc.sl1_boundaries(d)
        diff = pred - target
        assert int((diff != 0).sum()) == (0 if d == 0 else 1) and float(diff[517]) == float(torch.tensor(d, dtype=F32))
        assert torch.equal(sl1_twin(diff, True), sl1_twin(diff, False))


# ------------------------------------------------------------------------------------------------ BERT embedding
@pytest.mark.parametrize("T,batch", rc.BERT_SHAPES)
def test_all_pad_batch_exposes_pad_rows_dropped_from_dpos(T, batch):
    tb = rc.bert_tables(50)
    ids = rc.bert_ids(T, batch, 50, "pad")
    f = rc.bert_fwd_ref(ids, tb.word, tb.pos, tb.type0, tb.gamma, tb.beta, 1e-12, T)
    dy = torch.randn(batch * T, rc.HID, generator=rc.gen(4))
    ref = rc.bert_bwd_ref(dy, ids, tb.word, tb.pos, tb.type0, tb.gamma, f.mean.float(), f.rstd.float(), T)
    assert bool((ref.dword == 0).all())
    bar = rc.bar_dx(ref.dpos, T32)[:T]
    assert float(bar.min()) > 0 and bool((ref.dpos[T:] == 0).all())
    # twins: dpos summed over every row of a position / only over the rows whose token is not PAD
    x, t = rc.bert_embed_x(ids, tb.word, tb.pos, tb.type0, T)
    dx = rc.ln_bwd_ref(dy, x, tb.gamma, f.mean.float(), f.rstd.float()).dx.float()
    right = torch.zeros(512, rc.HID).index_add_(0, t, dx)
    wrong = torch.zeros(512, rc.HID).index_add_(0, t, dx * (ids.reshape(-1) != 0)[:, None])
    assert worst(right[:T], ref.dpos[:T], bar) < 0.1 and worst(wrong[:T], ref.dpos[:T], bar) > 2.0


def test_id_layouts():
    ids = rc.bert_ids(20, 17, 1000, "mixed")
    assert int(ids.max()) == 999 and bool((ids[:, -5:] == 0).all()) and bool((ids[:, :15] != 0).all())
    assert bool((rc.bert_ids(20, 17, 1000, "same") == 5).all())


# ------------------------------------------------------------------------------------------------ the references against torch's own float64
def test_references_match_torch_autograd():
    g = rc.gen(9)
    rows, C, eps = 33, 72, 1e-5
    x = torch.randn(rows, C, generator=g, dtype=torch.float64, requires_grad=True)
    gm, bt = (1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(), torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    dy = torch.randn(rows, C, generator=g, dtype=torch.float64)
    y = F.layer_norm(x, (C,), gm, bt, rc.f32(eps))
    y.backward(dy)
    f = rc.ln_fwd_ref(x.detach(), gm.detach(), bt.detach(), eps)
    b = rc.ln_bwd_ref(dy, x.detach(), gm.detach(), f.mean, f.rstd)
    for got, want in ((f.y, y.detach()), (b.dx, x.grad), (b.dgamma, gm.grad), (b.dbeta, bt.grad)):
        assert float((got - want).abs().max()) < 1e-12
    # chained: the second norm of the first output
    f2 = rc.ln_fwd_ref(x.detach(), gm.detach(), bt.detach(), eps, chain=(bt.detach(), gm.detach(), 1e-6))
    assert float((f2.y2 - F.layer_norm(y.detach(), (C,), bt.detach(), gm.detach(), rc.f32(1e-6))).abs().max()) < 1e-12

    V = 123
    lg = (3 * torch.randn(rows, V, generator=g, dtype=torch.float64)).requires_grad_()
    lab = torch.randint(0, V, (rows,), generator=g)
    lab[::5] = -1
    loss = F.cross_entropy(lg, lab, ignore_index=-1)
    loss.backward()
    r = rc.ce_ref(lg.detach(), lab)
    assert abs(r.loss_sum / r.count - float(loss.detach())) < 1e-12 and float((r.dlogits - lg.grad).abs().max()) < 1e-14
    assert float((r.lse - torch.logsumexp(lg.detach(), -1)).abs().max()) == 0

    p = torch.randn(1000, generator=g, dtype=torch.float64).mul_(2).requires_grad_()
    t = torch.randn(1000, generator=g, dtype=torch.float64)
    l1 = F.smooth_l1_loss(p, t)
    l1.backward()
    s = rc.sl1_ref(p.detach(), t)
    assert abs(s.loss_sum / 1000 - float(l1.detach())) < 1e-12 and float((s.grad - p.grad).abs().max()) < 1e-15

    tb = rc.bert_tables(40)
    T, batch = 20, 3
    ids = rc.bert_ids(T, batch, 40, "mixed")
    w, ps, tp = (v.double().requires_grad_() for v in (tb.word, tb.pos, tb.type0))
    gm, bt = tb.gamma.double().requires_grad_(), tb.beta.double().requires_grad_()
    keep = (torch.rand(batch * T, rc.HID, generator=g) >= 0.1).to(torch.uint8)
    e = F.embedding(ids, w, padding_idx=0) + tp + ps[:T]
    scale = 1.0 / (1.0 - rc.f32(0.1))
    y = F.layer_norm(e, (rc.HID,), gm, bt, rc.f32(1e-12)).reshape(batch * T, rc.HID) * keep.double() * scale
    dy = torch.randn(batch * T, rc.HID, generator=g, dtype=torch.float64)
    y.backward(dy)
    f = rc.bert_fwd_ref(ids, tb.word, tb.pos, tb.type0, tb.gamma, tb.beta, 1e-12, T, keep, 0.1)
    b = rc.bert_bwd_ref(dy, ids, tb.word, tb.pos, tb.type0, tb.gamma, f.mean, f.rstd, T, keep, 0.1)
    assert float((f.y - y.detach()).abs().max()) < 1e-12
    for got, want in ((b.dword, w.grad), (b.dpos, ps.grad), (b.dtype0, tp.grad), (b.dgamma, gm.grad), (b.dbeta, bt.grad)):
        assert float((got - want).abs().max()) < 1e-11

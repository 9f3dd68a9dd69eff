"""CPU: the premises of tests/loss_cases.py (docs/loss_options.md).  The float64 reference the GPU file measures the kernels of csrc/loss.hip against IS
torch's F.cross_entropy(weight=, ignore_index=, label_smoothing=) -- value and gradient, on every case --, and every wrong formula a kernel could compute
instead moves that reference past a bar on at least one case, so the cases can tell them apart."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import loss_cases as lc
from tests import rowwise_cases as rc


@pytest.fixture(scope="module")
def built():
    return {c.name: lc.build(c) for c in lc.CASES}


def test_the_case_list_covers_what_the_kernels_branch_on():
    shapes = {(c.V, c.ld) for c in lc.CASES}
    assert {(2, 2), (48, 48), (122, 122), (122, 128), (30522, 30522), (30522, 30528)} <= shapes
    assert any(c.rows > 1024 for c in lc.CASES)                                   # the finish kernel's stride loop
    assert any(c.ld % 4 == 0 and c.V % 4 == 0 for c in lc.CASES)                   # vector path, no tail
    assert any(c.ld % 4 == 0 and c.V % 4 != 0 for c in lc.CASES)                   # vector path + scalar tail
    assert any(c.ld % 4 != 0 for c in lc.CASES)                                    # scalar path
    opts = {(c.e, c.weights) for c in lc.CASES}
    assert {(0.1, None), (0.3, None), (0.0, "rand"), (0.1, "rand"), (0.1, "tiny")} <= opts
    assert any(c.ignored == "all" for c in lc.CASES) and len(lc.SHIFTED) == 12 and all(c.data == "shifted" and c.e == 0.1 for c in lc.SHIFTED)
    assert all(0.0 <= c.e < 1.0 and (c.e > 0 or c.weights) for c in lc.CASES)       # no case is the plain loss


def test_inputs_are_what_they_claim(built):
    for c in lc.CASES:
        i = built[c.name]
        assert tuple(i.x.shape) == (c.rows, c.ld) and i.x.dtype == torch.float32 and i.labels.dtype == torch.int64
        assert bool((i.x[:, c.V:] == lc.PAD_FILL).all()) and bool(torch.isfinite(i.x[:, :c.V]).all())
        ign = i.labels == lc.IGNORE
        assert bool(((i.labels >= 0) & (i.labels < c.V))[~ign].all())
        if c.ignored == "all":
            assert bool(ign.all())
        else:
            assert 0.15 <= float(ign.float().mean()) <= 0.25 and not bool(ign[0])
        if c.weights:
            assert tuple(i.weight.shape) == (c.V,) and bool((i.weight > 0).all())
            den = float(i.weight.double()[i.labels[~ign]].sum())
            assert (den < 1.0) == (c.weights == "tiny") or c.ignored == "all"         # "tiny": den < 1 although every weight is positive
        if c.data == "shifted":
            assert float(i.x[:, :c.V].min()) > lc.SHIFT - 30


def test_the_reference_is_torch(built):
    """loss to 1e-13 relative, gradient to 1e-11 of the largest entry, in float64; the all-ignored cases are NaN / zero in both"""
    for c in lc.CASES:
        i = built[c.name]
        x = i.x[:, :c.V].double().requires_grad_(True)
        w = None if i.weight is None else i.weight.double()
        loss = F.cross_entropy(x, i.labels, weight=w, ignore_index=lc.IGNORE, label_smoothing=c.e)
        ref = lc.case_ref(c, i, gscale=1.0)
        if c.ignored == "all":
            assert math.isnan(float(loss.detach())) and math.isnan(float(ref.loss)) and float(ref.den) == 0 and not bool(ref.dlogits.any())
            continue
        (g,) = torch.autograd.grad(loss, x)
        loss = loss.detach()
        assert abs(float(loss) - float(ref.loss)) <= 1e-13 * abs(float(loss)), c.name
        assert float((g - ref.dlogits).abs().max()) <= 1e-11 * float(g.abs().max()), c.name
        # gscale multiplies the gradient as the C ABI passes it (a float)
        ref3 = lc.case_ref(c, i, gscale=3.7)
        assert float((rc.f32(3.7) * g - ref3.dlogits).abs().max()) <= 1e-11 * 3.7 * float(g.abs().max()), c.name
        # the pieces the kernels hand over: loss = num / den, num = sum of the kept rows' two terms
        keep = i.labels != lc.IGNORE
        y = i.labels.clamp_min(0)
        wv = torch.ones(c.V, dtype=torch.float64) if w is None else w
        num = ((1 - c.e) * wv[y] * (ref.lse - x.detach().gather(1, y[:, None])[:, 0]) + c.e / c.V * ref.smooth)[keep].sum()
        assert abs(float(num) - float(ref.num)) <= 1e-12 * abs(float(num)) and float(ref.W) == pytest.approx(float(wv.sum()), rel=1e-15), c.name


@pytest.mark.parametrize("wrong", lc.WRONG)
def test_every_wrong_formula_is_exposed(built, wrong):
    """in float64 on the CPU, against the fp32 bar: at least one case (with a backward) moves past it; and where the formula names a premise -- padding, weights,
    ignored rows, den < 1 -- the cases WITHOUT that premise do not move at all"""
    hits = [c.name for c in lc.CASES if c.backward and c.ignored != "all" and lc.exposed(c, built[c.name], wrong)]
    assert hits, wrong
    needs = {"e_over_ld": lambda c: c.ld != c.V and c.e > 0, "sum_over_ld": lambda c: c.ld != c.V and c.e > 0, "smooth_ignored": lambda c: c.e > 0,
             "den_rows": lambda c: c.weights is not None, "label_no_1me": lambda c: c.e > 0, "W_is_V": lambda c: c.weights is not None and c.e > 0,
             "den_clamped": lambda c: c.weights == "tiny"}[wrong]
    assert all(needs(lc.BY_NAME[n]) for n in hits), (wrong, [n for n in hits if not needs(lc.BY_NAME[n])])
    # (not every case with the premise moves: 30522 -> 30528 changes e / V by 2e-4 of itself, below the bar; 122 -> 128 is what exposes e / ld)
    assert any(lc.BY_NAME[n].V <= 122 for n in hits), wrong                    # ... and a narrow case, cheap to look at, is among them


def test_the_naive_smoothing_sum_fails_on_the_shifted_rows(built):
    """W lse - sum_c w_c x_c formed in fp32 from an fp32 lse and a plain fp32 sum loses the row's smoothing term on logits near 3e4 at the narrow widths (half an
    ulp of 3e4 is 1e-3, the term is a few units); against the pivot x[r, 0] the same fp32 arithmetic keeps it.  This is what the GPU file's shifted-rows test
    decides about the kernel."""
    worst_naive, worst_pivot = 0.0, 0.0
    for c in lc.SHIFTED:
        if c.V > 200:
            continue
        i = built[c.name]
        ref = lc.case_ref(c, i)
        x = i.x[:, :c.V]
        w = torch.ones(c.V) if i.weight is None else i.weight
        lse32 = torch.logsumexp(x.double(), -1).float()
        naive = w.sum() * lse32 - (w * x).sum(-1)
        piv = x[:, :1]
        m = x.amax(-1)
        pivot = w.sum() * ((m - piv[:, 0]) + (x - m[:, None]).exp().sum(-1).log()) - (w * (x - piv)).sum(-1)
        bar = lc.bar_row(ref.smooth, rc.TOL[lc.F32])
        worst_naive = max(worst_naive, float(((naive.double() - ref.smooth).abs() / bar).max()))
        worst_pivot = max(worst_pivot, float(((pivot.double() - ref.smooth).abs() / bar).max()))
    assert worst_naive > 1.0 and worst_pivot < 0.05, (worst_naive, worst_pivot)

"""GPU, kernel level: the label-smoothed / class-weighted cross entropy of csrc/loss.hip (include/mvlt_hip_loss.h, docs/loss_options.md) against the float64
reference of tests/loss_cases.py, which tests/test_loss_cases_cpu.py shows to be F.cross_entropy and to tell every wrong formula apart.

Every case runs the forward (row kernel + finish kernel) and, from what the forward left, the backward into fp32 and into bf16 dlogits.  Judged: lse and the
row's smoothing term per row, den, W, the mean loss, every element of dlogits, the zeroed padding columns, and that nothing outside the outputs was written.
Tolerances: rowwise_cases.TOL through the bars of loss_cases; every figure is printed before it is asserted."""
import math

import pytest
import torch

from tests import loss_cases as lc
from tests import rowwise_cases as rc

pytestmark = pytest.mark.gpu

BF, F32 = rc.BF, rc.F32
SENTINEL, GUARD = 12345.0, 16
TAG = {BF: "bf16", F32: "fp32"}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as _ops
    return _ops


class Out:
    """an output buffer of n elements followed by GUARD sentinel elements that must survive"""

    def __init__(self, n, dtype=F32):
        self.n = n
        self.buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=dev())
        self.t = self.buf[:n]

    def intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())


def place(x, offset):
    """the fp32 matrix as a flat device tensor `offset` elements into its allocation (offset 1: off the 16-byte grid, the scalar path of both kernels)"""
    flat = torch.full((x.numel() + offset + GUARD,), SENTINEL, dtype=F32, device=dev())
    flat[offset:offset + x.numel()] = x.reshape(-1).to(dev())
    t = flat[offset:offset + x.numel()]
    assert t.data_ptr() % 16 == (4 * offset) % 16
    return t


def judge(parity, quantity, what, got, ref, bar):
    err = (got.double() - ref.double()).abs()
    bar = bar if torch.is_tensor(bar) else torch.full_like(err, float(bar))
    ratio = float((err / bar).max()) if err.numel() else 0.0
    print(f"{what}: {quantity}: worst error / bar = {ratio:.3e} (max abs error {float(err.max()) if err.numel() else 0.0:.3e})")
    ok = parity(f"{quantity}/{what}", ratio, 1.0) and bool(torch.isfinite(got).all())
    assert ok, f"{what}: {quantity} misses its bar: error / bar = {ratio:.3e}"


def run_case(ops, parity, case, *, offset=0, gscale=1.0, extra_ldd=0):
    from mvlt_amd._lib import last_kernel
    inp = lc.build(case)
    V, ld, rows, e = case.V, case.ld, case.rows, case.e
    what = case.name + (f"+{offset}el" if offset else "") + (f"+ldd{extra_ldd}" if extra_ldd else "")
    x = place(inp.x, offset)
    labels = inp.labels.to(dev())
    w = None if inp.weight is None else inp.weight.to(dev())
    ref = lc.smooth_ref(inp.x.to(dev()), labels, V, weight=w, e=e, gscale=gscale)
    lse, smooth, acc = Out(rows), Out(rows), Out(3)
    ops.ce_smooth_fwd(x, labels, lse.t, smooth.t, acc.t, rows, V, ld, label_smoothing=e, weight=w)
    torch.cuda.synchronize()
    assert "ce_smooth_finish_kernel" in last_kernel(), last_kernel()
    assert lse.intact() and smooth.intact() and acc.intact(), f"{what}: the forward wrote past an output"
    t = rc.TOL[F32]
    judge(parity, "lse", what, lse.t, ref.lse, lc.bar_row(ref.lse, t))
    if e > 0:
        judge(parity, "row smoothing term", what, smooth.t, ref.smooth, lc.bar_row(ref.smooth, t))
    else:
        assert bool((smooth.t == SENTINEL).all()), f"{what}: e == 0 must not write the smoothing terms"
    num, den, W = (float(v) for v in acc.t)
    print(f"{what}: num {num!r} den {den!r} W {W!r}; reference {float(ref.num)!r} {float(ref.den)!r} {float(ref.W)!r}")
    assert abs(W - float(ref.W)) <= t * float(ref.W), (what, W, float(ref.W))
    assert abs(den - float(ref.den)) <= t * float(ref.den), (what, den, float(ref.den))
    if case.ignored == "all":
        assert den == 0.0 and num == 0.0 and math.isnan(float(acc.t[0] / acc.t[1])), (what, num, den)
    else:
        judge(parity, "loss", what, acc.t[0:1] / acc.t[1:2], ref.loss.reshape(1), lc.bar_loss(ref.loss, t))
    if not case.backward:
        return
    gs = torch.tensor([gscale], dtype=F32, device=dev())
    for odt in (F32, BF):
        ldd = ld + extra_ldd
        dl = Out(rows * ldd, odt)
        ops.ce_smooth_bwd(x, labels, lse.t, gs, acc.t, dl.t, rows, V, ld, ldd, label_smoothing=e, weight=w)
        torch.cuda.synchronize()
        assert "ce_smooth_bwd_kernel" in last_kernel(), last_kernel()       # (the bf16 instantiation's name comes back mangled)
        assert dl.intact(), f"{what}: the backward wrote past dlogits"
        got = dl.t.view(rows, ldd)
        assert bool((got[:, V:] == 0).all()), f"{what}: padding columns [V, ldd) of {TAG[odt]} dlogits are not zero"
        if case.ignored == "all":
            assert bool((got == 0).all()), f"{what}: every row is ignored, the gradient must be zero"
            continue
        ign = labels == lc.IGNORE
        assert bool((got[ign] == 0).all()), f"{what}: an ignored row's gradient must be zero"
        judge(parity, f"dlogits {TAG[odt]}", what, got[:, :V], ref.dlogits, lc.bar_dlogits(ref, rc.tol(F32, odt), gscale, odt))
    assert bool((x == place(inp.x, offset)).all())                                 # the logits are read, never written


PLAIN = [c for c in lc.CASES if c.data != "shifted"]


@pytest.mark.parametrize("name", [c.name for c in PLAIN])
def test_ce_smooth_cases(ops, parity, name):
    """every shape x option combination, the all-ignored, den < 1, peaked and flat cases; vector path where ld is a multiple of 4, scalar path elsewhere"""
    run_case(ops, parity, lc.BY_NAME[name])


@pytest.mark.parametrize("name", [c.name for c in lc.SHIFTED])
def test_ce_smooth_shifted_rows(ops, parity, name):
    """cancellation: logits near 3e4, e = 0.1.  The row's smoothing term must meet its per-row bar -- a sum formed as W lse - sum_c w_c x_c in fp32 does not
    (tests/test_loss_cases_cpu.py)"""
    run_case(ops, parity, lc.BY_NAME[name])


@pytest.mark.parametrize("name", ["V48-ld48-r37-normal-e0.1+w", "V122-ld128-r37-normal-e0.1+w", "V122-ld128-r37-normal-e0.3", "V30522-ld30528-r5-normal-e0.1",
                                  "V30522-ld30528-r5-normal-e0.1+w", "V122-ld128-r37-shifted-e0.1"])
def test_ce_smooth_off_the_16_byte_grid(ops, parity, name):
    """the same matrices one element into their allocation: ld is a multiple of 4, the base pointer is not 16-byte aligned -- the scalar path of both kernels"""
    run_case(ops, parity, lc.BY_NAME[name], offset=1)


@pytest.mark.parametrize("name", ["V122-ld122-r37-normal-e0.1+w", "V122-ld128-r37-normal-e0.1", "V48-ld48-r1030-normal-e0.1+w", "V30522-ld30528-r5-normal-e0.3"])
def test_ce_smooth_gscale_and_wider_dlogits(ops, parity, name):
    """gscale = 3.7 from the device scalar; dlogits 8 columns wider than the logits (ldd != ld), all of them zeroed"""
    run_case(ops, parity, lc.BY_NAME[name], gscale=3.7, extra_ldd=8)


def test_two_runs_give_the_same_bits(ops):
    for name in ("V30522-ld30528-r5-normal-e0.1+w", "V48-ld48-r1030-normal-e0.1+w", "V122-ld122-r37-normal-e0.3"):
        c = lc.BY_NAME[name]
        inp = lc.build(c)
        x, labels = inp.x.to(dev()).reshape(-1), inp.labels.to(dev())
        w = None if inp.weight is None else inp.weight.to(dev())
        gs = torch.ones(1, device=dev())
        runs = []
        for _ in range(2):
            lse, smooth, acc = (torch.empty(n, device=dev()) for n in (c.rows, c.rows, 3))
            dl = torch.empty(c.rows * c.ld, device=dev(), dtype=BF)
            ops.ce_smooth_fwd(x, labels, lse, smooth, acc, c.rows, c.V, c.ld, label_smoothing=c.e, weight=w)
            ops.ce_smooth_bwd(x, labels, lse, gs, acc, dl, c.rows, c.V, c.ld, c.ld, label_smoothing=c.e, weight=w)
            runs.append((lse, smooth, acc, dl))
        torch.cuda.synchronize()
        for a, b in zip(*runs):
            assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------------------------ engine.cross_entropy
def test_options_off_is_the_plain_function_bit_for_bit():
    from mvlt_amd import engine
    for V, rows in ((2, 37), (122, 37), (48, 1030)):
        x0, lab = rc.ce_shifted_rows(rows, V, 0.0, seed=3)
        lab[::5] = -100
        x0, lab = x0.to(dev()), lab.to(dev())
        a = x0.clone().requires_grad_(True)
        b = x0.clone().requires_grad_(True)
        la = engine.cross_entropy(a, lab, label_smoothing=0.0, weight=None)
        lb = engine._CrossEntropyFn.apply(b, lab, -100)
        assert type(la.grad_fn).__name__ == type(lb.grad_fn).__name__
        (2.5 * la).backward()
        (2.5 * lb).backward()
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.grad, b.grad), V


@pytest.mark.parametrize("e,weighted", [(0.1, False), (0.3, True), (0.0, True)])
def test_engine_cross_entropy_is_torchs(parity, e, weighted):
    """the autograd function: loss and gradient against F.cross_entropy in float64 on the same device tensors, ignore_index at its default of -100"""
    import torch.nn.functional as F
    from mvlt_amd import engine
    for V, rows in ((48, 37), (122, 64)):
        x0, lab = rc.ce_shifted_rows(rows, V, 0.0, seed=5)
        lab[1::5] = -100
        x0, lab = x0.to(dev()), lab.to(dev())
        w = (0.5 + 1.5 * torch.rand(V, generator=rc.gen(1))).to(dev()) if weighted else None
        x = x0.clone().requires_grad_(True)
        loss = engine.cross_entropy(x, lab, label_smoothing=e, weight=w)
        assert type(loss.grad_fn).__name__.startswith("_SmoothCrossEntropyFn")
        (1.5 * loss).backward()
        xd = x0.double().requires_grad_(True)
        want = F.cross_entropy(xd, lab, weight=None if w is None else w.double(), label_smoothing=e)
        (1.5 * want).backward()
        den = float(w[lab[lab != -100]].sum()) if weighted else float((lab != -100).sum())
        what = f"V{V} e{e} {'w' if weighted else '-'}"
        judge(parity, "engine loss", what, loss.detach().reshape(1), want.detach().reshape(1), lc.bar_loss(want.detach(), rc.TOL[F32]))
        judge(parity, "engine dlogits", what, x.grad, xd.grad, rc.bar_dlogits(xd.grad, rc.TOL[F32], 1.5, den, F32))


def test_engine_cross_entropy_refuses_bad_options():
    from mvlt_amd import engine
    from mvlt_amd._lib import MVLTError
    x, lab = torch.randn(8, 48, device=dev()), torch.zeros(8, dtype=torch.int64, device=dev())
    for e in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(MVLTError, match="label_smoothing"):
            engine.cross_entropy(x, lab, label_smoothing=e)
    for w in (torch.ones(48), torch.ones(47, device=dev()), torch.ones(48, device=dev(), dtype=torch.float64), torch.ones(1, 48, device=dev()), [1.0] * 48):
        with pytest.raises(MVLTError, match="weight must be"):
            engine.cross_entropy(x, lab, weight=w)
    assert math.isfinite(float(engine.cross_entropy(x, lab, label_smoothing=0.1, weight=torch.ones(48, device=dev()))))


# ------------------------------------------------------------------------------------------------------------------ guards
def test_bad_arguments_are_refused_before_any_launch(ops):
    """argument checks of the two entry points: an error code and a message, nothing launched; the device works afterwards"""
    import mvlt_amd._lib as L
    rows, V, ld = 4, 8, 8
    x, lab = torch.randn(rows * ld, device=dev()), torch.zeros(rows, dtype=torch.int64, device=dev())
    lse, smooth, acc, gs = (torch.zeros(n, device=dev()) for n in (rows, rows, 3, 1))
    dl = torch.zeros(rows * ld, device=dev())
    w = torch.ones(V, device=dev())
    p = lambda t: None if t is None else t.data_ptr()
    err = lambda: L.lib.mvlt_last_error().decode()
    bad = lambda good, i, v: good[:i] + [v] + good[i + 1:]
    # logits, labels, ignore, e, weight, lse, smooth, acc, rows, V, ld, dtype, stream
    fwd = [p(x), p(lab), -1, 0.1, p(w), p(lse), p(smooth), p(acc), rows, V, ld, 1, None]
    # logits, labels, ignore, e, weight, lse, gscale, acc, dlogits, rows, V, ld, ldd, dtype, out_dtype, stream
    bwd = [p(x), p(lab), -1, 0.1, p(w), p(lse), p(gs), p(acc), p(dl), rows, V, ld, ld, 1, 1, None]
    f, b = L.lib.mvlt_ce_smooth_fwd, L.lib.mvlt_ce_smooth_bwd
    torch.cuda.synchronize()
    for fn, good, name, nulls in ((f, fwd, "mvlt_ce_smooth_fwd", (0, 1, 5, 6, 7)), (b, bwd, "mvlt_ce_smooth_bwd", (0, 1, 5, 6, 7, 8))):
        iV, ild, idt = (9, 10, 11) if fn is f else (10, 11, 13)
        for i in nulls:
            assert fn(*bad(good, i, None)) < 0 and f"{name}: null pointer" in err(), (name, i)
        for v in (0, -3):
            assert fn(*bad(good, iV, v)) < 0 and "V must be positive" in err(), (name, v)
        assert fn(*bad(good, ild, V - 1)) < 0 and "smaller than V" in err(), name
        for e in (-0.01, 1.0, 2.0, float("nan")):
            assert fn(*bad(good, 3, e)) < 0 and "label_smoothing must be in [0, 1)" in err(), (name, e)
        for d in (0, 2):
            assert fn(*bad(good, idt, d)) < 0 and "must be fp32" in err(), (name, d)
        assert fn(*bad(good, iV - 1, -1)) < 0 and "rows must not be negative" in err(), name
    assert b(*bad(bwd, 12, V - 1)) < 0 and "ldd = 7 is smaller" in err()
    assert b(*bad(bwd, 14, 2)) < 0 and "out_dtype" in err()
    # the same refusals through the op layer raise MVLTError; bf16 logits are refused by the entry point, not cast
    with pytest.raises(L.MVLTError, match="label_smoothing"):
        ops.ce_smooth_fwd(x, lab, lse, smooth, acc, rows, V, ld, label_smoothing=1.0)
    with pytest.raises(L.MVLTError, match="must be fp32"):
        ops.ce_smooth_fwd(x.bfloat16(), lab, lse, smooth, acc, rows, V, ld, label_smoothing=0.1)
    with pytest.raises(L.MVLTError, match="smaller than V"):
        ops.ce_smooth_bwd(x, lab, lse, gs, acc, dl, rows, V, ld - 1, ld, label_smoothing=0.1)
    torch.cuda.synchronize()
    assert not lse.any() and not acc.any() and not dl.any()                      # nothing ran
    # rows == 0: the finish launch alone -- acc = {0, 0, W}; the backward launches nothing
    acc.fill_(7.0)
    ops.ce_smooth_fwd(x, lab, lse, smooth, acc, 0, V, ld, label_smoothing=0.1, weight=w)
    ops.ce_smooth_bwd(x, lab, lse, gs, acc, dl, 0, V, ld, ld, label_smoothing=0.1, weight=w)
    torch.cuda.synchronize()
    assert acc.tolist() == [0.0, 0.0, float(V)] and not dl.any()
    # and the device is as usable as before
    ops.ce_smooth_fwd(x, lab, lse, smooth, acc, rows, V, ld, label_smoothing=0.1, weight=w)
    ref = lc.smooth_ref(x.view(rows, ld), lab, V, weight=w, e=0.1)
    torch.cuda.synchronize()
    assert abs(float(acc[0] / acc[1]) - float(ref.loss)) <= 1e-3 * float(ref.loss)

"""CPU: the premises of tests/test_gelu_range_gpu.py (tests/gelu_cases.py; docs/gelu_range.md).  The sweep is complete and bf16-exact, every one-hot construction
isolates exactly one activation per observed element, the restated forms meet their design bounds, and the comparison notices what a subtly wrong kernel does."""
import math

import pytest
import torch

from tests import gelu_cases as gc

BF, F64 = torch.bfloat16, torch.float64


def bits(t):
    return t.float().to(BF).view(torch.int16).to(torch.int32) & 0xffff


# ================================================================== the sweep
def test_sweep_is_bf16_exact_and_complete():
    """64 rows x 128 columns: every bf16 value of the 32 binades 2^-28 .. 2^3 (up to just under 16), both signs, each exactly once; a_m, w_j and the products are
    bf16-exact; the table's clamp at 2^-9, the polynomial clamps at 3.985 / 4, the sigmoid clamp at 7 and |h| = 8 have values on both sides"""
    a, w, h = gc.row_values(), gc.col_values(256), gc.sweep(256)
    assert gc.bf16_exact(a[:gc.NMAIN + 2]) and gc.bf16_exact(w) and gc.bf16_exact(h[:gc.NMAIN + 2])
    assert gc.bf16_exact(a) and not gc.bf16_exact(h[list(gc.DENORMAL_ROWS)])          # (the denormal row: the operand is exact, its products are not)
    assert torch.equal(h[:, :128], h[:, 128:])
    main = bits(h[:gc.NMAIN, :128]).flatten()
    want = [(s << 15) | (e << 7) | m for s in (0, 1) for e in range(127 - 28, 127 + 4) for m in range(128)]
    assert sorted(main.tolist()) == sorted(want) and len(set(want)) == 8192
    mag = h[:gc.NMAIN].abs()
    for edge in (2.0 ** -9, gc.PHI_CLAMP, gc.DG_CLAMP, gc.SIG_CLAMP, 8.0):
        assert bool((mag < edge).any()) and bool((mag > edge).any())
    for edge in (2.0 ** -9, 4.0, 8.0):                                                # (3.985 and 7 are not bf16 values)
        assert bool((mag == edge).any())
    assert float(mag.max()) == 15.9375
    extra = h[gc.NMAIN:]
    assert bool((extra[0] == 0).all()) and bool(torch.signbit(extra[0]).all())
    assert float(extra[1, 0]) == 2.0 ** -126 and 0 < float(extra[2].abs().max()) < 2.0 ** -126


# ================================================================== isolation
def one_hot_columns(m, cols):
    """every column of `cols` has exactly one nonzero entry, a 1; returns the row of each"""
    sub = m[:, cols]
    assert bool(((sub != 0).sum(0) == 1).all()) and bool(((sub == 1).sum(0) == 1).all())
    return sub.argmax(0).tolist()


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("hid", [64, 128, 192, 256])
def test_forward_and_dx_operands_isolate_one_activation(C, hid):
    seen = []
    for s in range(gc.fwd_slices(C, hid)):
        c = gc.mlp_fwd_case(C, hid, s)
        assert torch.equal(gc.h_of(c), c.h) and gc.bf16_exact(c.x) and gc.bf16_exact(c.w1)
        assert one_hot_columns(c.w2.t(), c.cols) == c.units                            # out[:, c] = G[:, unit]: one term
        rest = [k for k in range(C) if k not in c.cols]
        assert not bool(c.w2[rest].any())
        seen += c.units
    assert sorted(seen) == list(range(hid))                                            # every hidden-unit position observed once
    seen = []
    for g in range(gc.dx_groups(C, hid)):
        c = gc.mlp_dx_case(C, hid, g)
        assert torch.equal(gc.h_of(c), c.h)                                            # the selector columns of W1 meet zeros in x
        assert bool((c.dy @ c.w2 == 1).all())                                          # dG = 1 at every unit
        k = len(c.units)
        assert one_hot_columns(c.w1, list(range(1, 1 + k))) == c.units and not bool(c.w1[:, 1 + k:].any())
        assert torch.equal(c.w1[:, 0], gc.col_values(hid))
        seen += c.units
    assert sorted(seen) == list(range(hid))


@pytest.mark.parametrize("C", [64, 128])
def test_weight_gradient_operands_isolate_one_activation(C):
    hid = 256
    for M in ((64,) if C == 64 else (64, 128)):
        c = gc.mlp_dw2_case(C, hid, M)
        assert torch.equal(gc.h_of(c), c.h) and c.rows[:64] == list(range(64))
        assert one_hot_columns(c.dy, list(range(M))) == list(range(M)) and not bool(c.dy[:, M:].any())      # dW2[c] = G[c]: one term
        assert not bool((c.dy @ c.w2).any())                                           # dG = 0: dW1 = db1 = 0
    seen = []
    for part in range(gc.dw1_parts(C)):
        c = gc.mlp_dw1_case(C, hid, part)
        M = len(c.rows)
        assert M <= C - 1 and torch.equal(gc.h_of(c), c.h)
        assert bool((c.dy @ c.w2 == 1).all())
        assert one_hot_columns(c.x, list(range(1, 1 + M))) == list(range(M)) and not bool(c.x[:, 1 + M:].any())      # dW1[:, 1 + m] = dH[m]: one term
        seen += c.rows
    assert seen == list(range(gc.NROWS)) and gc.dw1_parts(64) == 2 and gc.dw1_parts(128) == 1


@pytest.mark.parametrize("N", [128, 131, 136])
def test_gemm_operands(N):
    c = gc.gemm_case(N)
    assert torch.equal(c.A @ c.B.t(), c.h) and bool((c.A2 @ c.B2.t() == 1).all())
    assert gc.bf16_exact(c.A) and gc.bf16_exact(c.B) and c.A.shape == (67, 8)


# ================================================================== the forms meet their design bounds
def worst(form):
    h = gc.sweep(128)
    g, dg = gc.emulate(form, h)
    r, dr = gc.exact(h)
    nz = h != 0
    phi = torch.where(nz, (g - r) / torch.where(nz, h, torch.ones_like(h)), torch.zeros_like(h)).abs()
    return h, (g - r).abs(), (dg - dr).abs(), phi


def test_design_bounds():
    """the bounds the comments of csrc/common.h, csrc/mlp_wgrad.hip and DESIGN state, at every bf16 input of the sweep (float32 arithmetic as the source writes it)"""
    h, eg, ed, ephi = worst("sigmoid")
    assert float(eg.max()) <= 3.0e-5 and float(ed.max()) <= 9.5e-5
    h, eg, ed, ephi = worst("poly")
    inside = h.abs() <= 4
    assert float(ed[inside].max()) <= 2.8e-4 and float(ed.max()) <= 2.8e-4 + 5.0e-4
    assert 1.0e-4 < float(ephi.max()) <= 1.05e-4                       # (just over the 1.0e-4 the comment used to state)
    assert abs(float(h.flatten()[ephi.argmax()])) == 2.59375 and abs(float(ephi.max()) - 1.040e-4) < 5e-8      # the figure and the place common.h and DESIGN cite
    assert float(eg.max()) <= 4.1e-4                                    # = 3.9 x 1.05e-4
    # the tail past the clamp: Phi~ is constant there, within 4e-7 of 0 / 1.  (In exact arithmetic the polynomial is 6e-7 inside [0, 1] at 3.985; the fp32 Horner
    # -- terms of magnitude 3.5 cancel -- lands at -3.6e-7 / 1 + 3.6e-7: |gelu~(h)| <= 4e-7 |h| with EITHER sign, against 7.2e-5 |h| clamped at 4.)
    tail = gc.poly_phi(torch.tensor([-16.0, -gc.PHI_CLAMP, gc.PHI_CLAMP, 16.0])).double()
    assert tail[0] == tail[1] and tail[2] == tail[3] and float(tail[:2].abs().max()) <= 4e-7 and float((tail[2:] - 1).abs().max()) <= 4e-7
    h, eg, ed, ephi = worst("pair")
    inside = h.abs() <= gc.PHI_CLAMP
    assert float(ed[inside].max()) <= 1.1e-4 and float(ed.max()) <= 5.7e-4 and float(ephi.max()) <= 1.05e-4
    for form in ("erf", "erf2"):                                        # A&S 7.1.26: 1.5e-7 in erf = 0.75e-7 in Phi, plus float32 rounding of a value near 1 (6e-8 a step)
        h, eg, ed, ephi = worst(form)
        assert float(ephi.max()) <= 3e-7 and float(ed.max()) <= 3e-7
    h, eg, ed, ephi = worst("lut")
    table = (h.abs() >= 2.0 ** -9)
    assert float(ephi[table].max()) <= 1.5e-7 and float(ed[table].max()) <= 1.5e-7       # the table is exact to 1e-7; above 8 Phi and GELU' are 0 / 1 to 1e-14
    # below 2^-9 the lookup returns the entry of 2^-9: Phi'(0) 2^-9 = 7.8e-4 in Phi (times |h| < 2^-9 in GELU), GELU''(0) 2^-9 = 1.56e-3 in GELU'
    ephi[gc.NMAIN:] = 0                                                 # (the extra rows: a denormal product has no relative precision; their GELU error is in eg)
    assert float(ephi[~table].max()) <= 7.8e-4 and float(ed[~table].max()) <= 1.56e-3 and float(eg[~table].max()) <= 7.8e-4 * 2.0 ** -9


def test_bars_are_small_against_the_function():
    """a bar never reaches a quarter of the distance to the neighbouring activation's value where that matters (|h| >= 1/4): a misplaced element cannot hide"""
    h = gc.sweep(128)[:gc.NMAIN]
    r, dr = gc.exact(h)
    rows = list(range(gc.NMAIN))
    for form in gc.FORMS:
        for what, ref in (("g", r), ("dg", dr)):
            b = gc.bar(form, what, h, ref, rows, rounded=True)
            assert bool((b <= 2.0 ** -8 * ref.abs() + 2.5e-3).all()), (form, what)


# ================================================================== the comparison notices a wrong kernel
def kernel_like(form, what, h, *, rounded, v=None, lanes=False):
    g, dg = gc.emulate(form, h, v, lanes)
    got = g if what == "g" else dg
    return got.float().to(BF).double() if rounded else got


PERTURBED = [
    ("poly", "g", "coef_sign", False), ("poly", "dg", "coef_sign", False), ("poly", "g", "clamp4", False), ("poly", "g", None, True), ("poly", "dg", None, True),
    ("sigmoid", "dg", "coef_sign", False), ("sigmoid", "g", None, True), ("sigmoid", "dg", None, True),
    ("lut", "g", "index", False), ("lut", "dg", "index", False), ("lut", "g", "sign", False), ("lut", "dg", "sign", False), ("lut", "g", None, True),
    ("erf", "g", None, True), ("erf2", "dg", None, True),
]


@pytest.mark.parametrize("form", list(gc.FORMS))
@pytest.mark.parametrize("rounded", [False, True])
def test_the_forms_as_they_stand_pass(form, rounded):
    h = gc.sweep(128)
    rows = list(range(gc.NROWS))
    for what, ref in zip(("g", "dg"), gc.exact(h)):
        ratio = gc.compare(kernel_like(form, what, h, rounded=rounded), ref, gc.bar(form, what, h, ref, rows, rounded=rounded), h, f"{form} {what}")
        assert ratio <= 1.0


@pytest.mark.parametrize("form,what,v,lanes", PERTURBED)
@pytest.mark.parametrize("rounded", [False, True])
def test_perturbed_forms_fail(form, what, v, lanes, rounded):
    """one coefficient's sign, the Phi clamp at 4 instead of 3.985 (the overshoot common.h describes), the two packed lanes exchanged, the table index off by one, the
    sign FMA dropped: each is over its bar somewhere, and the failure names (row, col, h, got, want)"""
    h = gc.sweep(128)
    rows = list(range(gc.NROWS))
    ref = gc.exact(h)[0 if what == "g" else 1]
    with pytest.raises(AssertionError, match=r"\(row, col, h, got, want\): \[\(\d+, \d+, ") as e:
        gc.compare(kernel_like(form, what, h, rounded=rounded, v=v, lanes=lanes), ref, gc.bar(form, what, h, ref, rows, rounded=rounded), h, f"{form} {what} {v}")
    if v == "clamp4":                                                  # the overshoot shows where common.h says: from |h| = 4 on
        row, col, hh, got, want = e.value.first[0]
        assert math.isfinite(got) and abs(hh) >= 4

"""CPU: the premises of tests/test_gelu_range_gpu.py (tests/gelu_cases.py; docs/gelu_range.md).  The sweep is complete and bf16-exact, every one-hot construction
isolates exactly one activation per observed element, the restated forms meet their design bounds, and the comparison notices what a subtly wrong kernel does."""
import math
import os
import re

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


# ================================================================== the 8-phase NT GEMM epilogues (tests/test_gelu_p8_gpu.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = sorted(gc.P8_M)


def source(name):
    return open(os.path.join(ROOT, "mvlt_amd", name)).read()


def test_p8_epilogues_compile_the_polynomials():
    """EPI 3 / 4 of nt_epilogue_lean call gelu_fast2 / gelu_fast_grad2, which are gelu_poly1 / gelu_poly_grad1 under MVLT_GELU_POLY bits 1 / 0; the default is 3 and
    neither the build nor the 8-phase translation unit sets another: the bars of the 8-phase cases are the `poly` ones"""
    common, epi, p8 = source("csrc/common.h"), source("csrc/gemm_common.h"), source("csrc/gemm_nt_p8.hip")
    assert re.search(r"#ifndef MVLT_GELU_POLY\n#define MVLT_GELU_POLY 3\n#endif", common)
    assert re.search(r"f32x2 gelu_fast2\(f32x2 x\) \{\n#if MVLT_GELU_POLY & 2\n  return f32x2\{gelu_poly1\(x\[0\]\), gelu_poly1\(x\[1\]\)\};\n#endif", common)
    assert re.search(r"f32x2 gelu_fast_grad2\(f32x2 x\) \{\n#if MVLT_GELU_POLY & 1\n  return f32x2\{gelu_poly_grad1\(x\[0\]\), gelu_poly_grad1\(x\[1\]\)\};\n#endif", common)
    lean = epi[epi.index("void nt_epilogue_lean("):epi.index("void nt_epilogue_192(")]
    assert re.search(r"if \(EPI == 3\) \{\n\s+if \(p\.H\) store8\(p\.H, v\);[^}]*gelu_fast2\(", lean) and re.search(r"if \(EPI == 4\) \{[^}]*gelu_fast_grad2\(f32x2\{o8\[e\]", lean)
    assert "gelu_erf" not in lean and "MVLT_GELU_POLY" not in p8 and "MVLT_GELU_POLY" not in source("build.py")
    assert "nt_epilogue_lean<128, EPI, WMT, 4, EPI != 2 && !RAG>" in p8                  # NWN = 4, FULL = true for EPI 3 / 4 of the whole-tile instantiations


@pytest.mark.parametrize("BM", TILES)
def test_p8_sweep_operands_and_tile_coverage(BM):
    """cases 1 and 2: one product per element, equal to the tiled sweep; the act 2 accumulator is 2^(m mod 3 - n mod 5) and stays a non-zero fp32 value with the bias.
    Every 32-row half of a wave row x 128-column half of a tile (the unit the epilogue stages and the period of the mantissas) sees every value of the sweep -- all
    8192 bf16 values of the 32 binades and the three extra rows -- and every row position of a tile sees as many different sweep rows as there are row tiles"""
    c = gc.p8_sweep_case(BM)
    M, N = c.M, c.N
    assert (M, N) == (gc.P8_M[BM], 2048) and M % BM == 0 and N % 256 == 0 and (M // BM) * (N // 256) >= 192
    assert gc.bf16_exact(c.A) and gc.bf16_exact(c.B) and gc.bf16_exact(c.A2) and gc.bf16_exact(c.B2)
    assert not bool(c.A[:, 1:].any()) and not bool(c.B[:, 1:].any()) and not bool(c.A2[:, 0].any()) and not bool(c.A2[:, 2:].any()) and not bool(c.B2[:, 2:].any())
    u = c.u1()
    assert u.shape == (M, N) and torch.equal(c.A @ c.B.t(), c.t1.h[u]) and torch.equal(u, c.u2())
    m, n = gc.grid(M, N)
    acc = c.A2 @ c.B2.t()
    assert torch.equal(acc, 2.0 ** ((m % 3) - (n % 5)).double())
    assert len({(a, b) for a in range(3) for b in range(5)}) == 15 and math.gcd(3, 32) == math.gcd(5, 8) == 1       # the row AND the column name the accumulator
    withb = acc + c.bias2
    assert int((c.bias2 != 0).sum()) == len(gc.BIAS2) and bool((withb != 0).all()) and torch.equal(withb.float().double(), withb)
    assert {k % 256 // 64 for k in gc.BIAS2} == {0, 1, 2, 3} and {k % 64 // 8 for k in gc.BIAS2} >= {0, 7}
    full = set(range(gc.NFLAT))
    for rc in range(BM // 32):
        rows = ((m[:, 0] % BM) // 32 == rc).nonzero()[:, 0]
        for cc in range(2):
            cols = ((n[0] % 256) // 128 == cc).nonzero()[:, 0]
            assert set(u[rows][:, cols].unique().tolist()) == full, (rc, cc)
    want = bits(gc.sweep(128)[:gc.NMAIN]).flatten().tolist()
    assert sorted(bits(c.t1.h[:gc.NMAIN * 128]).tolist()) == sorted(want) and len(set(want)) == 8192
    for r in range(BM):
        assert len(set((u[r::BM, 0] // 128).tolist())) == M // BM


@pytest.mark.parametrize("BM", TILES)
def test_p8_bias_operands(BM):
    """case 3: the four launches carry every one of the 8192 main values exactly once, each an fp32 value; a column's value has no period of 64 or 128 columns"""
    seen = []
    for rep in range(4):
        c = gc.p8_bias_case(BM, rep)
        assert not bool(c.A.any()) and gc.bf16_exact(c.bias) and c.bias.shape == (c.N,)
        u = c.u1()
        assert u.shape == (c.M, c.N) and bool((u == u[0]).all()) and torch.equal(c.t1.h[u[0]], c.bias)
        for period in (64, 128):
            assert not bool((c.bias[period:] == c.bias[:-period]).any())
        seen += u[0].tolist()
    assert sorted(seen) == list(range(gc.NMAIN * 128))


@pytest.mark.parametrize("BM", TILES)
def test_p8_position_operands(BM):
    """case 4, the two conditions of the fixed seed: |h| <= 256 everywhere (h indexes the integer table) and at least half of the elements in 1 <= |h| <= 4, where
    GELU separates neighbouring integers by far more than a bar; the hash of act 2 reaches every sweep value and repeats with no row or column period"""
    c = gc.p8_position_case(BM)
    assert set(c.A.unique().tolist()) == set(c.B.unique().tolist()) == {-1.0, 0.0, 1.0} and c.K == 192 and c.A.shape == (gc.P8_M[BM], 192)
    h = c.A @ c.B.t()
    mag = h.abs()
    assert float(mag.max()) <= gc.INT_LIM and torch.equal(h, h.round()) and gc.bf16_exact(h)
    assert float(((mag >= 1) & (mag <= 4)).double().mean()) >= 0.5
    assert torch.equal(c.t1.h[c.u1()], h)
    t = gc.int_table()
    near = (t.h >= -3) & (t.h <= 5)                                                     # (GELU(-4) and GELU(-5) are both 1e-4 from 0: no more than a bar apart)
    assert bool(((t.g[1:] - t.g[:-1]).abs()[near[1:] & near[:-1]] > 8 * t.bar_g[1:][near[1:] & near[:-1]]).all())
    u = c.u2()
    assert set(u.unique().tolist()) == set(range(gc.NFLAT))
    for p in (1, 16, 32, 64, 67, 128, 256):
        assert float((u[p:] == u[:-p]).double().mean()) < 0.01 and float((u[:, p:] == u[:, :-p]).double().mean()) < 0.01, p


def p8_cases(BM):
    """(name, case, act, bias) of cases 1-4 on ONE row of tiles: the rows 0 .. BM - 1 of the launched case, which hold every position of a tile"""
    sw, pos = gc.p8_sweep_case(BM, BM), gc.p8_position_case(BM, BM)
    out = [("1 sweep act 1", sw, 1, None), ("2 sweep act 2", sw, 2, None), ("2 sweep act 2 + bias", sw, 2, sw.bias2)]
    out += [(f"3 bias only {rep}", c, 1, c.bias) for rep in (0, 3) for c in (gc.p8_bias_case(BM, rep, BM),)]
    return out + [("4 position act 1", pos, 1, None), ("4 position act 2", pos, 2, None)]


def p8_run(c, act, bias, move, name):
    C, H = gc.p8_model(c, act, move, bias)
    if act == 1:
        return gc.p8_check_act1(c, C, name)
    return gc.p8_check_act2(c, C, name, bias)


@pytest.mark.parametrize("BM", TILES)
def test_p8_models_as_they_stand_pass(BM):
    for name, c, act, bias in p8_cases(BM):
        assert p8_run(c, act, bias, None, name) <= 1.0
        if act == 1:
            gc.p8_check_h(c, gc.p8_model(c, act, None, bias)[1], name)


# the cases that must notice each move (asserted exactly: a case that is blind to a move is named by its absence)
ALL_ACT2 = ("2 sweep act 2", "2 sweep act 2 + bias", "4 position act 2")
CAUGHT_BY = {
    "slot1": ALL_ACT2, "slot2": ALL_ACT2,                                                # (act 1 prefetches nothing)
    "chunk64": ("1 sweep act 1",) + ALL_ACT2 + ("3 bias only 0", "3 bias only 3", "4 position act 1"),
    "chunk128": ALL_ACT2 + ("3 bias only 0", "3 bias only 3", "4 position act 1"),       # (the rank-one sweep of act 1 repeats every 128 columns)
    "bias_wave": ("2 sweep act 2 + bias", "3 bias only 0", "3 bias only 3"),
    "rows16": ("1 sweep act 1",) + ALL_ACT2 + ("4 position act 1",),                     # (the bias-only rows are all alike)
    "bias_order": ("2 sweep act 2 + bias", "3 bias only 0", "3 bias only 3"),
}


@pytest.mark.parametrize("move", gc.P8_MOVES)
@pytest.mark.parametrize("BM", TILES)
def test_p8_moves_are_caught(BM, move):
    """the moves a wrong epilogue would make -- the two prefetch slots exchanged, a lane chunk addressed 64 / 128 columns on, the bias chunk of the neighbouring wave
    column, rows r and r + 16 of a staged half exchanged, GELU on the wrong side of the bias -- applied to the restated form: each is over its bar in the named cases"""
    caught = []
    for name, c, act, bias in p8_cases(BM):
        try:
            p8_run(c, act, bias, move, name)
        except gc.OverBar as e:
            assert len(e.first[0]) == 5
            caught.append(name)
    assert caught and sorted(caught) == sorted(CAUGHT_BY[move]), (move, caught)

"""GPU: every bf16 input between saturation and zero through every kernel copy of GELU / GELU' (tests/gelu_cases.py, whose premises tests/test_gelu_cases_cpu.py
pins; the argument, the kernel each case asserts and the measured margins are in docs/gelu_range.md).  Every pre-activation is a_m w_j -- a power of two times
1 + k / 128 -- and the second matrix of each launch is one-hot, so one observed output element is ONE activation: it is compared with the float64 exact-erf GELU
(or its autograd derivative) under a bar derived on the CPU from the form the kernel compiles, per sign and binade.  Outputs sit between sentinel rows that must come
back unchanged; every case asserts the kernel it meant to reach and that the plan names it."""
import pytest
import torch

from tests import gelu_cases as gc
from tests.test_exact_gpu import dev, last_kernel, ops, ran          # noqa: F401  (ops is the module-scoped fixture)

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PAD, SENTINEL = 3, 7.0
ALL_ROWS = list(range(gc.NROWS))


def guarded(shape, dtype, fill=0.0):
    """(buffer, view): an output of `shape` holding `fill` as rows (elements, for a vector) PAD .. PAD + n of a sentinel-filled buffer"""
    shape = tuple(shape)
    buf = torch.full((shape[0] + 2 * PAD,) + shape[1:], SENTINEL, device=dev(), dtype=dtype)
    view = buf[PAD: PAD + shape[0]]
    view.fill_(fill)
    return buf, view


def untouched(buf, what):
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), f"{what}: the guard around the output was written"


def put(t, dtype=BF):
    return t.to(dtype).to(dev()).contiguous()


def check(parity, form, what, got, h, rows, *, rounded, name):
    """one activation per element of `got` against the float64 reference of h under the form's bar; records the worst error / bar"""
    ref = gc.exact(h)[0 if what == "g" else 1]
    ratio = gc.compare(got, ref, gc.bar(form, what, h, ref, rows, rounded=rounded), h, name)
    parity(f"{form} {what}/{name}", ratio, 1.0)


def check_sum(parity, form, what, got, h, rows, weights, *, rounded_terms, rounded_sum, name):
    """got[j] = sum_m weights[m] act(h[m][j]) against the float64 sum: the terms' bars summed, the fp32 accumulation, half a bf16 ulp where the sum is rounded"""
    ref = gc.exact(h)[0 if what == "g" else 1]
    w = weights.abs()[:, None]
    total = (ref * weights[:, None]).sum(0)
    b = (gc.bar(form, what, h, ref, rows, rounded=rounded_terms) * w).sum(0) + h.shape[0] * 2.0 ** -23 * (ref.abs() * w).sum(0)
    if rounded_sum:
        b = b + gc.half_ulp_bf16(total.abs() + b)
    hrow = h.abs().max(0).values[None, :]
    ratio = gc.compare(got.reshape(1, -1), total[None, :], b[None, :], hrow, name)
    parity(f"{form} {what} sum/{name}", ratio, 1.0)


def zero(t, what):
    assert not bool(t.any()), f"{what}: must be exactly 0"


def check_h(hst, h, name):
    """the stored pre-activation equals h bit for bit (the denormal row, whose products are no bf16 values and which the hardware may flush: below ABS)"""
    keep = [m for m in range(h.shape[0]) if m not in gc.DENORMAL_ROWS]
    assert torch.equal(hst[keep].double().cpu(), h[keep]), f"{name}: the stored pre-activation is not h"
    assert float(hst[list(gc.DENORMAL_ROWS)].double().abs().max()) <= gc.ABS


# ================================================================== fused MLP: forward and input gradient
FWD = [(C, hid, h_out) for C in (64, 128) for hid in (64, 128, 192, 256) for h_out in (False, True)]


@pytest.mark.parametrize("C,hid,h_out", FWD)
def test_mlp_forward_gelu(ops, parity, C, hid, h_out):
    """mlp_fused_kernel<C, 0> (hid 64, or with h_out) / mlp_pipe_kernel<C, 0>: gelu_poly1.  out[m][c] = bf16(gelu~(h[m][c + C s])) for every slice s"""
    fam = f"{'mlp_fused_kernel' if h_out or hid < 128 else 'mlp_pipe_kernel'}<{C}, 0>"
    M = gc.NROWS
    b1, b2, res = torch.zeros(hid, device=dev()), torch.zeros(C, device=dev()), torch.zeros(M, C, device=dev())
    for s in range(gc.fwd_slices(C, hid)):
        c = gc.mlp_fwd_case(C, hid, s)
        x, w1, w2 = put(c.x), put(c.w1), put(c.w2)
        obuf, out = guarded((M, C), F32, SENTINEL)
        hbuf, hst = guarded((M, hid), BF, SENTINEL) if h_out else (None, None)
        ops.mlp_fwd(x, w1, b1, w2, b2, res, out, M, C, hid, h_out=hst)
        ran(fam)
        assert ops.mlp_plan("fwd", x, w1, b1, w2, b2, res, out, M, C, hid, h_out=hst).name == last_kernel()
        check(parity, "poly", "g", out[:, c.cols], c.h[:, c.units], ALL_ROWS, rounded=True, name=f"fwd C {C} hid {hid} slice {s}")
        zero(out[:, [k for k in range(C) if k not in c.cols]], "unobserved output columns")
        untouched(obuf, "out")
        if h_out:
            check_h(hst, c.h, "h_out")
            untouched(hbuf, "h_out")


@pytest.mark.parametrize("C,hid", [(C, hid) for C in (64, 128) for hid in (64, 128, 192, 256)])
def test_mlp_input_gradient_gelu_grad(ops, parity, C, hid):
    """mlp_fused_kernel<C, 1> (hid 64) / mlp_pipe_kernel<C, 1>: gelu_poly_grad1.  dx[m][1 + k] = bf16(gelu'~(h[m][j_k])) for every group of C - 1 units;
    dx[m][0] = sum_j bf16(gelu'~(h[m][j])) w_j"""
    fam = f"{'mlp_fused_kernel' if hid < 128 else 'mlp_pipe_kernel'}<{C}, 1>"
    M = gc.NROWS
    b1 = torch.zeros(hid, device=dev())
    for g in range(gc.dx_groups(C, hid)):
        c = gc.mlp_dx_case(C, hid, g)
        x, dy, w1, w2 = put(c.x), put(c.dy), put(c.w1), put(c.w2)
        xbuf, dx = guarded((M, C), BF, SENTINEL)
        ops.mlp_bwd_dx(x, dy, w1, w1.t().contiguous(), w2.t().contiguous(), b1, dx, M, C, hid)
        ran(fam)
        assert ops.mlp_plan("bwd_dx", x, dy, w1, w1.t().contiguous(), w2.t().contiguous(), b1, dx, M, C, hid).name == last_kernel()
        k = len(c.units)
        name = f"dx C {C} hid {hid} group {g}"
        check(parity, "poly", "dg", dx[:, 1: 1 + k], c.h[:, c.units], ALL_ROWS, rounded=True, name=name)
        zero(dx[:, 1 + k:], "unobserved dx columns")
        check_col0(parity, dx[:, 0], c.h, hid, name)
        untouched(xbuf, "dx")


def check_col0(parity, got, h, hid, name):
    """dx[m][0] = sum_j bf16(gelu'~(h[m][j])) w_j, rounded to bf16: the float64 sum with the summed bar"""
    ref = gc.exact(h)[1]
    w = gc.col_values(hid)[None, :]
    total = (ref * w).sum(1)
    b = (gc.bar("poly", "dg", h, ref, ALL_ROWS, rounded=True) * w).sum(1) + hid * 2.0 ** -23 * (ref.abs() * w).sum(1)
    b = b + gc.half_ulp_bf16(total.abs() + b)
    ratio = gc.compare(got.reshape(-1, 1), total[:, None], b[:, None], h.abs().max(1).values[:, None], name + " col 0")
    parity(f"poly dg sum/{name}", ratio, 1.0)


# ================================================================== fused MLP: weight gradients
# routing: no row_scale -> mlp_wgrad2_kernel (the table); rows_per_scale 50 / 20 with factors of exactly 1 -> mlp_wgrad_kernel (gelu_fast_both2: the sigmoid form at
# MVLT_GELU_POLY = 3); partials: the bf16 partial tiles of mlp_wgrad2_kernel, folded by tn_fold_flush behind it
ROUTES = [("table", 0, False), ("table-partials", 0, True), ("rows-50", 50, False), ("rows-20", 20, False)]
HID_DW = 256


def run_dw(ops, c, C, hid, rps, partials):
    M = c.x.shape[0]
    x, dy, w1, w2t = put(c.x), put(c.dy), put(c.w1), put(c.w2.t())
    b1 = torch.zeros(hid, device=dev())
    g = gc.NS()
    g.bufs = {}
    for k, shape in (("dw1", (hid, C)), ("db1", (hid,)), ("dw2", (C, hid)), ("db2", (C,))):
        g.bufs[k], t = guarded(shape, F32, 0.0)                # the kernels accumulate: into zeros, so that a small value is not rounded away
        setattr(g, k, t)
    kw = {}
    if rps:
        kw.update(row_scale=torch.ones((M + rps - 1) // rps, device=dev()), rows_per_scale=rps)
    if partials:                                               # deferred fold: the weight-gradient kernel itself is the last launch and can be asserted
        kw.update(partials=torch.full((1 << 20,), SENTINEL, device=dev(), dtype=BF), defer_fold=True)
    ops.mlp_bwd_dw(x, dy, w1, w2t, b1, g.dw1, g.db1, g.dw2, g.db2, M, C, hid, **kw)
    launched = last_kernel()
    plan = ops.mlp_plan("bwd_dw", x, dy, w1, w2t, b1, g.dw1, g.db1, g.dw2, g.db2, M, C, hid, **kw)
    if rps:
        assert launched == plan.name == f"mlp_wgrad_kernel<{C}>", launched
        g.form = "sigmoid"
    else:
        assert launched == plan.name == f"mlp_wgrad2_kernel<{C}, {4 if C == 64 else 8}>" and plan.fold == int(partials), (launched, plan.name, plan.fold)
        if partials:
            zero(g.dw1, "dW1 before the flush"), zero(g.dw2, "dW2 before the flush")
            ops.tn_fold_flush(kw["partials"])
            ran("tn_fold_multi_kernel")
        g.form = "lut"
    return g


def dw_untouched(g):
    for k, b in g.bufs.items():
        untouched(b, k)


@pytest.mark.parametrize("route,rps,partials", ROUTES)
@pytest.mark.parametrize("C,M", [(64, 64), (128, 64), (128, 128)])
def test_mlp_weight_gradient_gelu_through_dw2(ops, parity, C, M, route, rps, partials):
    """dy one-hot: dW2[c][j] = bf16(gelu~(h[c][j])), one term per element; db2 = 1; dG = 0, so dW1 = db1 = 0"""
    c = gc.mlp_dw2_case(C, HID_DW, M)
    g = run_dw(ops, c, C, HID_DW, rps, partials)
    check(parity, g.form, "g", g.dw2[:M], c.h, c.rows, rounded=True, name=f"dW2 C {C} M {M} {route}")
    zero(g.dw2[M:], "dW2 rows without a token"), zero(g.dw1, "dW1"), zero(g.db1, "db1")
    assert torch.equal(g.db2.cpu(), (torch.arange(C) < M).float()), "db2"
    dw_untouched(g)


@pytest.mark.parametrize("route,rps,partials", ROUTES)
@pytest.mark.parametrize("C", [64, 128])
def test_mlp_weight_gradient_gelu_grad_through_dw1(ops, parity, C, route, rps, partials):
    """x one-hot beside column 0, dG = 1: dW1[j][1 + m] = bf16(gelu'~(h[m][j])); dW1[j][0], db1[j] and dW2[0][j] are sums over the rows (float64, summed bars; the
    partial-tile path rounds the sums of dW1 / dW2 to bf16 once more)"""
    for part in range(gc.dw1_parts(C)):
        c = gc.mlp_dw1_case(C, HID_DW, part)
        M = len(c.rows)
        g = run_dw(ops, c, C, HID_DW, rps, partials)
        name = f"dW1 C {C} rows {c.rows[0]}..{c.rows[-1]} {route}"
        check(parity, g.form, "dg", g.dw1[:, 1: 1 + M].t(), c.h, c.rows, rounded=True, name=name)
        zero(g.dw1[:, 1 + M:], "dW1 columns without a token")
        a = gc.row_values()[c.rows]
        check_sum(parity, g.form, "dg", g.dw1[:, 0], c.h, c.rows, a, rounded_terms=True, rounded_sum=partials, name=name + " col 0")
        check_sum(parity, g.form, "dg", g.db1, c.h, c.rows, torch.ones(M, dtype=F64), rounded_terms=True, rounded_sum=False, name=name + " db1")
        check_sum(parity, g.form, "g", g.dw2[0], c.h, c.rows, torch.ones(M, dtype=F64), rounded_terms=True, rounded_sum=partials, name=name + " dW2 row 0")
        zero(g.dw2[1:], "dW2 rows without dy")
        assert torch.equal(g.db2.cpu(), (torch.arange(C) < 1).float() * M), "db2"
        dw_untouched(g)


# ================================================================== GEMM epilogues act 1 / act 2
# operand type, output type, N, first column, ldc, family of act 1, family of act 2, forms of the epilogue
GEMM = [
    (BF, BF, 128, 0, 128, "gemm_nt_dma_kernel<128, 0, 3, 32", "gemm_nt_dma_kernel<128, 0, 4, 32", ("poly",)),
    (BF, BF, 136, 0, 136, "gemm_nt_dma_kernel<128, 0, 3, 32", "gemm_nt_dma_kernel<128, 0, 4, 32", ("poly",)),          # a second column tile of 8 columns
    (BF, BF, 64, 0, 64, "gemm_nt_dma_kernel<64, 0, 3, 64", "gemm_nt_dma_kernel<64, 0, 4, 64", ("poly",)),
    (BF, BF, 64, 64, 64, "gemm_nt_dma_kernel<64, 0, 3, 64", "gemm_nt_dma_kernel<64, 0, 4, 64", ("poly",)),             # the other 64 mantissas
    (BF, F32, 128, 0, 128, "gemm_nt_dma_kernel<128, 0, 0, 64", "gemm_nt_dma_kernel<128, 0, 0, 64", ("erf2",)),         # fp32 output: the generic epilogue, no rounding
    (BF, F32, 136, 0, 136, "gemm_nt_dma_kernel<128, 0, 0, 64", "gemm_nt_dma_kernel<128, 0, 0, 64", ("erf2",)),
    (BF, F32, 131, 0, 136, "gemm_nt_dma_kernel<128, 0, 0, 64", "gemm_nt_dma_kernel<128, 0, 0, 64", ("erf2", "erf")),   # ragged last chunk: the scalar erf forms
    (BF, BF, 131, 0, 136, "gemm_nt_dma_kernel<128, 0, 0, 64", "gemm_nt_dma_kernel<128, 0, 0, 64", ("erf2", "erf")),    # ... rounded once
    (F32, F32, 128, 0, 128, "gemm_nt_kernel<float, 128>", "gemm_nt_kernel<float, 128>", ("erf2",)),
    (F32, F32, 136, 0, 136, "gemm_nt_kernel<float, 128>", "gemm_nt_kernel<float, 128>", ("erf2",)),
    (F32, F32, 131, 0, 131, "gemm_nt_kernel<float, 128>", "gemm_nt_kernel<float, 128>", ("erf",)),                     # unaligned rows: every column scalar
    (F32, F32, 64, 64, 64, "gemm_nt_kernel<float, 64>", "gemm_nt_kernel<float, 64>", ("erf2",)),
]


def check_any(parity, forms, what, got, h, rows, *, rounded, name):
    """the bar of an epilogue that applies one of `forms` per column chunk: the larger of their bars"""
    ref = gc.exact(h)[0 if what == "g" else 1]
    b = torch.stack([gc.bar(f, what, h, ref, rows, rounded=rounded) for f in forms]).max(0).values
    parity(f"{'|'.join(forms)} {what}/{name}", gc.compare(got, ref, b, h, name), 1.0)


@pytest.mark.parametrize("dtype,odtype,N,j0,ldc,fam1,fam2,forms", GEMM)
def test_gemm_nt_gelu_epilogues(ops, parity, dtype, odtype, N, j0, ldc, fam1, fam2, forms):
    """act 1: C = gelu~(a_m w_n), H = h.  act 2: the product is exactly 1 and H = h comes from the host: C = gelu'~(h)"""
    c = gc.gemm_case(N, 8, j0)
    M, K = gc.NROWS, 8
    rounded = odtype == BF
    name = f"{'bf16' if dtype == BF else 'fp32'}->{'bf16' if rounded else 'fp32'} N {N}+{j0}"
    A, B = put(c.A, dtype), put(c.B, dtype)
    obuf, out = guarded((M, ldc), odtype, SENTINEL)
    hbuf, H = guarded((M, ldc), odtype, SENTINEL)
    ops.gemm_nt(A, B, out, M, N, K, K, K, ldc, act=1, H=H)
    ran(fam1)
    assert ops.gemm_nt_plan(A, B, out, M, N, K, K, K, ldc, act=1, H=H).name == last_kernel()
    check_any(parity, forms, "g", out[:, :N], c.h, ALL_ROWS, rounded=rounded, name=name + " act 1")
    check_h(H[:, :N], c.h, "H")
    for buf, t, what in ((obuf, out, "C"), (hbuf, H, "H")):
        untouched(buf, what)
        assert bool((t[:, N:] == SENTINEL).all()), f"{what}: columns past N were written"
    A2, B2 = put(c.A2, dtype), put(c.B2, dtype)
    Hin = torch.full((M, ldc), SENTINEL, device=dev(), dtype=odtype)
    Hin[:, :N] = c.h.to(odtype).to(dev())
    o2buf, out2 = guarded((M, ldc), odtype, SENTINEL)
    ops.gemm_nt(A2, B2, out2, M, N, K, K, K, ldc, act=2, H=Hin)
    ran(fam2)
    assert ops.gemm_nt_plan(A2, B2, out2, M, N, K, K, K, ldc, act=2, H=Hin).name == last_kernel()
    check_any(parity, forms, "dg", out2[:, :N], c.h, ALL_ROWS, rounded=rounded, name=name + " act 2")
    untouched(o2buf, "C")
    assert bool((out2[:, N:] == SENTINEL).all()), "C: columns past N were written"


# ================================================================== gelu_bwd
@pytest.mark.parametrize("dtype", [BF, F32])
def test_gelu_bwd_range(ops, parity, dtype):
    """gelu_bwd_kernel: gelu_erf_grad at dy = 1 over the full set and a ragged tail (n = 67 x 128 + 5: no multiple of 8).  The tail's last element is +0 (the set has
    -0 only): GELU'(+0) = 1/2 through the other side of copysign"""
    h = gc.sweep(128)
    tail = torch.cat([h[30, :4], torch.zeros(1, dtype=F64)])
    assert not bool(torch.signbit(tail[-1]))
    flat = torch.cat([h.flatten(), tail])
    n = flat.numel()
    assert n % 8 == 5
    hd = put(flat, dtype)
    buf, out = guarded((n,), dtype, SENTINEL)
    ops.gelu_bwd(torch.ones(n, device=dev(), dtype=dtype), hd, out)
    ran("gelu_bwd_kernel")
    rounded = dtype == BF
    check(parity, "erf", "dg", out[:h.numel()].reshape(h.shape), h, ALL_ROWS, rounded=rounded, name=f"gelu_bwd {dtype}")
    check(parity, "erf", "dg", out[h.numel():].reshape(1, 5), tail[None, :], [30], rounded=rounded, name=f"gelu_bwd {dtype} tail")
    untouched(buf, "out")

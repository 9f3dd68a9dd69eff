"""GPU: the fused-MLP kernels of csrc/mlp_fused.hip, mlp_pipe.hip and mlp_wgrad.hip, the GELU epilogues of the GEMMs and gelu_bwd on SATURATED integer data (tests/mlp_cases.py, whose premises
tests/test_mlp_cases_cpu.py pins; the argument is in docs/mlp_exact.md).  Every pre-activation is an integer with |h| >= 16: a unit that is on passes h and
dG through its bf16 tile unchanged, a unit that is off contributes at most a derived, per-element bound, and the MLP becomes two integer GEMMs whose float64
reference must be met bit for bit -- one dropped row, one misplaced hidden unit or one row under another sample's DropPath factor is a hard mismatch with a
row and a column to print.  Every case asserts the kernel family it meant to reach, and that the launch ran what ops.mlp_plan names
for the same arguments.  Operands are row slices of buffers whose other rows hold a finite poison
(7.0: a wrong read shows as an integer error; NaN would not pass the zero page the kernels substitute past the last row), outputs are slices of
sentinel-filled buffers whose surroundings must come back unchanged."""
import pytest
import torch

from tests import mlp_cases as mc
from tests.test_exact_gpu import dev, last_kernel, ops, ran          # noqa: F401  (ops is the module-scoped fixture)

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
PAD, POISON = 3, 7.0


def guarded(t=None, shape=None, dtype=None, fill=POISON):
    """(buffer, view): `t` -- or an output of `shape` -- as rows PAD .. PAD + rows of a buffer filled with `fill`"""
    shape = tuple(t.shape) if t is not None else tuple(shape)
    buf = torch.full((shape[0] + 2 * PAD,) + shape[1:], fill, device=dev(), dtype=t.dtype if t is not None else dtype)
    view = buf[PAD: PAD + shape[0]]
    if t is not None:
        view.copy_(t)
    return buf, view


def untouched(buf, what, fill=POISON):
    assert bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all()), f"{what}: rows outside the output were written"


def on_device(c):
    """the operands of a case on the device: x and dy between poisoned rows"""
    d = mc.NS(x=guarded(c.x.to(dev()))[1], dy=guarded(c.dy.to(dev()))[1], w1=c.w1.to(dev()), w2=c.w2.to(dev()), b1=c.b1.to(dev()), b2=c.b2.to(dev()),
              res=c.res.to(dev()), scale=None if c.scale is None else c.scale.to(dev()))
    d.w1t, d.w2t = d.w1.t().contiguous(), d.w2.t().contiguous()
    d.kw = dict(row_scale=d.scale, rows_per_scale=c.rps)
    d.ref = mc.NS(**{k: v.to(dev()) for k, v in vars(c.ref).items()})
    d.bound = mc.NS(**{k: (None if v is None or not c.off else v.to(dev())) for k, v in vars(c.bound).items()})
    return d


# ================================================================== forward and input gradient
@pytest.mark.parametrize("C,hid,h_out,fam,M,rps,factors,off", mc.FWD_CASES)
def test_mlp_forward_and_dx(ops, C, hid, h_out, fam, M, rps, factors, off):
    c = mc.fwd_case(C, hid, M, rps, factors, off)
    d = on_device(c)
    what = f"C {C} hid {hid} M {M}"
    obuf, out = guarded(shape=(M, C), dtype=F32)
    hbuf, hst = guarded(shape=(M, hid), dtype=BF) if h_out else (None, None)
    ops.mlp_fwd(d.x, d.w1, d.b1, d.w2, d.b2, d.res, out, M, C, hid, h_out=hst, **d.kw)
    ran(f"{fam}<{C}, 0>")
    assert ops.mlp_plan("fwd", d.x, d.w1, d.b1, d.w2, d.b2, d.res, out, M, C, hid, h_out=hst, **d.kw).name == last_kernel()
    mc.compare(out, d.ref.out, d.bound.out, what + " out")
    untouched(obuf, "out")
    if h_out:
        mc.compare(hst, d.ref.h, None, what + " h_out")
        untouched(hbuf, "h_out")
    # out_op: the bf16 copy is `out` rounded once, next to out and alone
    for with_out in (True, False):
        o2buf, o2 = guarded(shape=(M, C), dtype=F32)
        pbuf, op = guarded(shape=(M, C), dtype=BF)
        ops.mlp_fwd(d.x, d.w1, d.b1, d.w2, d.b2, d.res, o2 if with_out else None, M, C, hid, out_op=op, h_out=hst, **d.kw)
        ran(f"{fam}<{C}, 0>")
        assert ops.mlp_plan("fwd", d.x, d.w1, d.b1, d.w2, d.b2, d.res, o2 if with_out else None, M, C, hid, out_op=op, h_out=hst, **d.kw).name == last_kernel()
        assert torch.equal(op, out.to(BF)), "out_op is not out rounded once"
        mc.compare(op, d.ref.out, d.bound.out, what + " out_op")
        assert torch.equal(o2, out) if with_out else bool((o2buf == POISON).all())
        untouched(pbuf, "out_op"), untouched(o2buf, "out")
    xbuf, dx = guarded(shape=(M, C), dtype=BF)
    ops.mlp_bwd_dx(d.x, d.dy, d.w1, d.w1t, d.w2t, d.b1, dx, M, C, hid, **d.kw)
    ran(f"{'mlp_fused_kernel' if hid < 128 else 'mlp_pipe_kernel'}<{C}, 1>")        # no pre-activation output on this side: the pipelined kernel from 128 units on
    assert ops.mlp_plan("bwd_dx", d.x, d.dy, d.w1, d.w1t, d.w2t, d.b1, dx, M, C, hid, **d.kw).name == last_kernel()
    mc.compare(dx, d.ref.dx, d.bound.dx, what + " dx")
    untouched(xbuf, "dx")


# ================================================================== weight gradients
def run_dw(ops, c, d, **kw):
    """one launch into sentinel-surrounded gradients that hold 3.0 (the kernels accumulate)"""
    g = mc.NS()
    g.b1buf, g.dw1 = guarded(shape=(c.hid, c.C), dtype=F32)
    g.b2buf, g.dw2 = guarded(shape=(c.C, c.hid), dtype=F32)
    g.b3buf, g.db1 = guarded(shape=(c.hid,), dtype=F32)
    g.b4buf, g.db2 = guarded(shape=(c.C,), dtype=F32)
    for t in (g.dw1, g.dw2, g.db1, g.db2):
        t.fill_(3.0)
    ops.mlp_bwd_dw(d.x, d.dy, d.w1, d.w2t, d.b1, g.dw1, g.db1, g.dw2, g.db2, c.M, c.C, c.hid, **d.kw, **kw)
    g.launched = last_kernel()
    g.plan = ops.mlp_plan("bwd_dw", d.x, d.dy, d.w1, d.w2t, d.b1, g.dw1, g.db1, g.dw2, g.db2, c.M, c.C, c.hid, **d.kw, **kw)
    return g


def check_dw(g, d, what):
    for k in ("dw1", "db1", "dw2", "db2"):
        mc.compare(getattr(g, k), getattr(d.ref, k) + 3.0, getattr(d.bound, k), f"{what} {k}")
    for b, k in ((g.b1buf, "dw1"), (g.b2buf, "dw2"), (g.b3buf, "db1"), (g.b4buf, "db2")):
        untouched(b, k)


@pytest.mark.parametrize("name,C,hid,M,scaled", mc.WG_CASES)
def test_mlp_weight_gradients_tile_uniform(ops, name, C, hid, M, scaled):
    """mlp_wgrad2_kernel: one tile per split (M = 1, 63, 65) and two / three tiles per split (the LDS-DMA ring, the prefetch under the barrier, slot reuse, a
    ragged last tile, idle workgroups behind the last split); scaled: factors 1, 2, 0, 0.5 cycling over 64-row samples -- the accumulator-rescale branch, a dropped
    tile between two live ones, a split whose every tile is dropped (its partial tiles must still be written, as zeros).  The atomic path, the bf16 partial
    tiles with the immediate fold and the deferred fold behind tn_fold_flush all equal the reference; the two folds equal each other bit for bit."""
    c = mc.wg_case(C, hid, M, scaled)
    d = on_device(c)
    fam = f"mlp_wgrad2_kernel<{C}, {4 if C == 64 else 8}>"
    g = run_dw(ops, c, d)
    ran(fam)
    assert g.plan.name == g.launched and g.plan.fold == 0
    check_dw(g, d, name + " atomic")
    scratch = torch.full((16 * 1024 * 1024,), POISON, device=dev(), dtype=BF)
    now = run_dw(ops, c, d, partials=scratch)
    ran("tn_fold_kernel")
    assert now.plan.name == fam and now.plan.fold == 1 and now.plan.partials_need <= scratch.numel() * 2       # (the launch ran the two folds behind the planned kernel)
    check_dw(now, d, name + " immediate fold")
    scratch.fill_(POISON)
    later = run_dw(ops, c, d, partials=scratch, defer_fold=True)
    ran(fam)
    assert later.plan.name == later.launched and later.plan.fold == 1
    assert bool((later.dw1 == 3.0).all()) and bool((later.dw2 == 3.0).all()), "a deferring launch touched dW before the flush"
    ops.tn_fold_flush(scratch)
    ran("tn_fold_multi_kernel")
    check_dw(later, d, name + " deferred fold")
    for k in ("dw1", "dw2"):                                  # (the bias gradients stay fp32 atomics: equal where exact, which check_dw has asserted)
        assert torch.equal(getattr(later, k), getattr(now, k)), f"{k}: the deferred fold differs from the immediate one"


@pytest.mark.parametrize("C,hid,rps,factors", mc.R2_CASES)
def test_mlp_weight_gradients_factor_per_row(ops, C, hid, rps, factors):
    """mlp_wgrad_kernel (rows_per_scale % 64 != 0): two samples per tile (100 rows per sample), three with pairwise different factors (52: stage 2 of a
    64 x 32 px input with T = 20) and four (20)"""
    c = mc.r2_case(C, hid, rps, factors)
    d = on_device(c)
    g = run_dw(ops, c, d)
    ran(f"mlp_wgrad_kernel<{C}>")
    assert g.plan.name == g.launched and g.plan.fold == 0
    check_dw(g, d, f"rows_per_scale {rps}")


# ================================================================== GEMM GELU epilogues, gelu_bwd
GEMM_GELU = [  # dtype, M, N, K, family of act 1 (H stored), family of act 2: two small shapes of NT_PLAIN (tests/test_exact_gpu.py) per operand type
    (BF, 257, 200, 200, "gemm_nt_dma_kernel<128, 0, 3, 32", "gemm_nt_dma_kernel<128, 0, 4, 32"),
    (BF, 257, 40, 72, "gemm_nt_dma_kernel<64, 0, 3, 64", "gemm_nt_dma_kernel<64, 0, 4, 64"),
    (F32, 257, 200, 100, "gemm_nt_kernel<float, 128>", "gemm_nt_kernel<float, 128>"),
    (F32, 257, 40, 36, "gemm_nt_kernel<float, 64>", "gemm_nt_kernel<float, 64>"),
]


@pytest.mark.parametrize("dtype,M,N,K,fam1,fam2", GEMM_GELU)
def test_gemm_nt_gelu_epilogues_saturated(ops, dtype, M, N, K, fam1, fam2):
    """act 1 (GELU, pre-activation stored to H) and act 2 (v * GELU'(H)).  The erf forms of the fp32 kernel are exact on both sides; the fast forms of the bf16
    LDS-DMA kernel are exact on the on side (after the bf16 store) and within the derived bound on the off side."""
    c = mc.gemm_case(M, N, K, 400 + N + K)
    A, W, bias = c.A.to(dtype).to(dev()), c.W.to(dtype).to(dev()), c.bias.to(dev())
    fast = dtype == BF
    obuf, out = guarded(shape=(M, N), dtype=dtype)
    hbuf, H = guarded(shape=(M, N), dtype=dtype)
    ops.gemm_nt(A, W, out, M, N, K, K, K, N, bias=bias, act=1, H=H)
    ran(fam1)
    mc.compare(H, c.h.to(dev()), None, "H")
    mc.compare(out, c.G.to(dev()), c.bound_G.to(dev()) if fast else None, "gelu")
    untouched(obuf, "C"), untouched(hbuf, "H")
    Hin = c.h.to(dtype).to(dev())
    o2buf, out2 = guarded(shape=(M, N), dtype=dtype)
    ops.gemm_nt(A, W, out2, M, N, K, K, K, N, act=2, H=Hin)
    ran(fam2)
    mc.compare(out2, c.dH.to(dev()), c.bound_dH.to(dev()) if fast else None, "v * gelu'(H)")
    untouched(o2buf, "C")


@pytest.mark.parametrize("dtype", [BF, F32])
def test_gelu_bwd_saturated(ops, dtype):
    c = mc.gemm_case(257, 200, 100, 500)
    dy, h = c.v.to(dtype).to(dev()), c.h.to(dtype).to(dev())
    buf, out = guarded(shape=tuple(dy.shape), dtype=dtype)
    ops.gelu_bwd(dy, h, out)
    mc.compare(out, c.dH.to(dev()), None, "gelu_bwd")
    untouched(buf, "out")

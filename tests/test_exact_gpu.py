"""GPU: bit-exact checks of the GEMM, conv and reduction kernels on small-integer data.

With operands of magnitude <= 3 every product and every partial sum is an integer below 2^24, so fp32 accumulation is exact in ANY order: atomics,
split-K, m-splits and ordered folds must reproduce the float64 reference bit for bit, a bf16 / fp16 output is the exact result rounded once to
nearest-even, and one dropped, doubled or misaddressed element is a hard mismatch with a row and a column to print.  Every GEMM case asserts the kernel
family it meant to reach through mvlt_amd._lib.last_kernel(): a case that silently falls to another kernel fails instead of testing nothing.
(The GELU epilogues, act 1 / 2, are not exact on N(0,1) data and stay with the tolerance tests of test_kernels_gpu.py; on saturated data they and the fused MLP
are: test_mlp_exact_gpu.py.)"""
import ctypes as C_

import pytest
import torch

from tests.gemm_inst_cases import (BF, F16, F32, LIM, dev, exact, gather_3x3, gather_patch, integral, ints, last_kernel, pad_cols, phys_rows, picks,     # noqa: F401
                                    ran, sparse_pm1)          # (the helpers live beside the instantiation cases, tests/gemm_inst_cases.py; other test files import them from here)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as _ops
    return _ops


# ================================================================== gemm_nt
NT_PLAIN = [  # dtype, M, N, K, family: the smallest shapes with a ragged last row tile, a ragged last column tile and a K that is no whole number of k-steps
    (BF, 257, 200, 200, "gemm_nt_dma_kernel<128, 0, 1, 64"),
    (BF, 257, 40, 72, "gemm_nt_dma_kernel<64, 0, 1, 64"),
    (BF, 257, 576, 136, "gemm_nt_dma_kernel<192, 0, 1, 64"),        # N % 192 == 0 is what selects the tile: whole column tiles by construction
    (BF, 130, 203, 72, "gemm_nt_dma_kernel<128, 0, 1, 64"),         # N % 8 != 0: the last chunk of a row is stored column by column
    (BF, 257, 200, 1288, "gemm_nt_dma_kernel<128, 0, 1, 64"),       # long K: the ring of LDS stages wraps many times (21 k-steps, the last one ragged)
    (BF, 257, 40, 776, "gemm_nt_dma_kernel<64, 0, 1, 64"),
    (BF, 257, 576, 648, "gemm_nt_dma_kernel<192, 0, 1, 64"),
    (F32, 257, 200, 644, "gemm_nt_kernel<float, 128>"),
    (F32, 257, 200, 100, "gemm_nt_kernel<float, 128>"),
    (F32, 257, 40, 36, "gemm_nt_kernel<float, 64>"),
    (F32, 130, 203, 20, "gemm_nt_kernel<float, 128>"),
    # the 8-phase tiles are chosen by whole rounds of the chip: the shapes of test_kernels_gpu.py, an odd number of k-tiles
    (BF, 6400, 2048, 192, "gemm_nt_p8_kernel<1, 4, 2, 2, false>"),
    (BF, 6144, 2048, 192, "gemm_nt_p8_kernel<1, 3, 2, 2, false>"),
    (BF, 7680, 1600, 192, "gemm_nt_p8_kernel<1, 3, 3, 2, false>"),
    (BF, 1490, 30522, 192, "gemm_nt_p8_kernel<1, 4, 2, 2, true>"),  # ragged M and N on the 256 x 256 tile
    (BF, 9000, 1600, 192, "gemm_nt_p8_kernel<1, 3, 3, 2, true>"),   # ragged M on the 192 x 320 tile
]


@pytest.mark.parametrize("dtype,M,N,K,family", NT_PLAIN)
def test_gemm_nt_plain_with_bias(ops, dtype, M, N, K, family):
    A, W, bias = ints((M, K), -3, 3, dtype, 1), ints((N, K), -3, 3, dtype, 2), ints(N, -9, 9, F32, 3)
    ref = integral(A.double() @ W.double().t() + bias.double())
    ldc = (N + 7) // 8 * 8
    for odt in (F32, BF):
        buf = torch.full((M + 1, ldc), 7.0, device=dev(), dtype=odt)          # one guard row, guard columns behind N
        ops.gemm_nt(A, W, buf, M, N, K, K, K, ldc, bias=bias)
        ran(family)
        exact(buf[:M, :N], ref, f"plain {odt}")
        assert (buf[M] == 7.0).all() and (buf[:M, N:] == 7.0).all(), "wrote outside the M x N block"


NT_EPI = [  # dtype, M, N, K, family of the residual epilogue, family of the generic one
    (BF, 257, 200, 200, "gemm_nt_dma_kernel<128, 0, 2, 64", "gemm_nt_dma_kernel<128, 0, 0, 64"),
    (BF, 257, 40, 72, "gemm_nt_dma_kernel<64, 0, 2, 64", "gemm_nt_dma_kernel<64, 0, 0, 64"),
    (F32, 257, 200, 100, "gemm_nt_kernel<float, 128>", "gemm_nt_kernel<float, 128>"),
    (F32, 257, 40, 36, "gemm_nt_kernel<float, 64>", "gemm_nt_kernel<float, 64>"),
    (BF, 6400, 2048, 192, "gemm_nt_p8_kernel<2, 4, 2, 2, false>", None),
    (BF, 6144, 2048, 192, "gemm_nt_p8_kernel<2, 3, 2, 2, false>", None),
    (BF, 7680, 1600, 640, "gemm_nt_p8_kernel<2, 3, 3, 2, false>", None),      # (the 192 x 320 tile carries the residual epilogue from K = 640 on)
    (BF, 9000, 1600, 640, "gemm_nt_p8_kernel<2, 3, 3, 2, true>", None),
]


@pytest.mark.parametrize("dtype,M,N,K,fam_res,fam_gen", NT_EPI)
def test_gemm_nt_epilogue_terms(ops, dtype, M, N, K, fam_res, fam_gen):
    """epi(v) = (v + bias) * row_scale[m / rows_per_scale] + R with rows_per_scale not dividing M, R aliasing C, R in fp32 beside a bf16 C (r_fp32), and H handed
    over with act = 0 (the pre-activation is stored by act 1 only: H must come back untouched).  Factors in {0, 0.5, 1, 2}: every term a multiple of 0.5."""
    A, W, bias = ints((M, K), -3, 3, dtype, 4), ints((N, K), -3, 3, dtype, 5), ints(N, -9, 9, F32, 6)
    rps = M // 3 - 5                                                        # 4 factors, the last group short
    scale = picks((M + rps - 1) // rps, [0.0, 0.5, 1.0, 2.0], 7)
    srow = scale.double().repeat_interleave(rps)[:M, None]
    pre = integral(A.double() @ W.double().t() + bias.double())
    for odt in (F32, dtype):
        R = ints((M, N), -5, 5, odt, 8)
        ref = integral(pre * srow + R.double(), 0.5)
        out = R.clone()
        ops.gemm_nt(A, W, out, M, N, K, K, K, N, bias=bias, row_scale=scale, rows_per_scale=rps, R=out)
        ran(fam_res)
        exact(out, ref, f"row_scale + R aliasing C, {odt}")
        out2 = torch.full((M, N), 7.0, device=dev(), dtype=odt)              # R in a buffer of its own, no factor
        ops.gemm_nt(A, W, out2, M, N, K, K, K, N, bias=bias, R=R)
        ran(fam_res)
        exact(out2, integral(pre + R.double()), f"R beside C, {odt}")
    if dtype == BF:
        R32 = ints((M, N), -5, 5, F32, 9)
        o16 = torch.full((M, N), 7.0, device=dev(), dtype=BF)
        ops.gemm_nt(A, W, o16, M, N, K, K, K, N, bias=bias, row_scale=scale, rows_per_scale=rps, R=R32)
        ran(fam_res)
        exact(o16, integral(pre * srow + R32.double(), 0.5), "r_fp32")
    if fam_gen is not None:
        # a factor without a residual has no lean variant: the generic epilogue
        out = torch.full((M, N), 7.0, device=dev(), dtype=F32)
        ops.gemm_nt(A, W, out, M, N, K, K, K, N, bias=bias, row_scale=scale, rows_per_scale=rps)
        ran(fam_gen)
        exact(out, integral(pre * srow, 0.5), "row_scale alone")
    H = torch.full((M, N), 7.0, device=dev(), dtype=dtype)
    out = torch.empty(M, N, device=dev(), dtype=dtype)
    ops.gemm_nt(A, W, out, M, N, K, K, K, N, bias=bias, act=0, H=H)
    exact(out, pre, "act 0 with H")
    assert (H == 7.0).all(), "act 0 wrote H"


NT_STATS = [  # dtype, M, N, K, nonzero K columns of A, family
    (BF, 1000, 200, 200, 64, "gemm_nt_dma_kernel<128, 0, 5, 64"),
    (BF, 1000, 40, 72, 64, "gemm_nt_dma_kernel<64, 0, 5, 64"),
    (BF, 1000, 192, 136, 64, "gemm_nt_dma_kernel<192, 0, 5, 64"),
    (F32, 1000, 200, 100, 64, "gemm_nt_kernel<float, 128>"),
    (F32, 1000, 24, 36, 36, "gemm_nt_kernel<float, 64>"),
    (BF, 6400, 2048, 192, 48, "gemm_nt_p8_kernel<5, 4, 2, 2, false>"),
    (BF, 6144, 2048, 192, 48, "gemm_nt_p8_kernel<5, 3, 2, 2, false>"),
]


@pytest.mark.parametrize("dtype,M,N,K,nz,family", NT_STATS)
def test_gemm_nt_column_statistics(ops, dtype, M, N, K, nz, family):
    """col_sum / col_sumsq of the stored values, with one accumulator and with four interleaved ones, fp32 and fp16 C.  Operands in {-1, 0, 1} and A nonzero in
    its first `nz` columns only: |C| <= nz <= 64, so the squares summed over M stay below 2^24 (asserted on the reference)."""
    A = ints((M, K), -1, 1, dtype, 10)
    A[:, nz:] = 0
    W = ints((N, K), -1, 1, dtype, 11)
    ref = integral(A.double() @ W.double().t())
    assert float(ref.abs().max()) <= 64
    s1, s2 = integral(ref.sum(0)), integral((ref * ref).sum(0))
    for odt in ((F32, F16) if dtype == BF and N % 8 == 0 else (F32,)):
        for copies in (1, 4):
            out = torch.full((M, N), 7.0, device=dev(), dtype=odt)
            st = torch.zeros(2, copies, N, device=dev())
            ops.gemm_nt(A, W, out, M, N, K, K, K, N, col_sum=st[0], col_sumsq=st[1], col_copies=copies)
            ran(family)
            exact(out, ref, f"C {odt} copies {copies}")
            exact(st[0].sum(0), s1, f"col_sum {odt} copies {copies}")
            exact(st[1].sum(0), s2, f"col_sumsq {odt} copies {copies}")


@pytest.mark.parametrize("M,N,K,S,family", [(130, 100, 1000, 4, "gemm_nt_dma_kernel<128, 0, 0, 64"), (130, 40, 1000, 16, "gemm_nt_dma_kernel<64, 0, 0, 64"),
                                            (257, 200, 2120, 16, "gemm_nt_dma_kernel<128, 0, 0, 64"), (257, 200, 456, 4, "gemm_nt_dma_kernel<128, 0, 0, 64")])
def test_gemm_nt_split_k(ops, M, N, K, S, family):
    """K cut over S workgroups per tile (K no multiple of S x 64), fp32 atomics into a zeroed C: exact whatever order the atomics land in; the bias is added once"""
    A, W, bias = ints((M, K), -3, 3, BF, 12), ints((N, K), -3, 3, BF, 13), ints(N, -9, 9, F32, 14)
    assert K % (S * 64) != 0
    ref = integral(A.double() @ W.double().t() + bias.double())
    out = torch.zeros(M + 1, N, device=dev())
    ops.gemm_nt(A, W, out, M, N, K, K, K, N, bias=bias, split_k=S)
    ran(family)
    exact(out[:M], ref, "split_k")
    assert (out[M] == 0).all()


FLAKY_STAGES = [(4096, 320, 64), (1024, 320, 128), (256, 320, 320), (64, 320, 512)]        # image tokens, text tokens, width of the 256 px / T = 320 step (B = 2)


def _nt_token_subrange(ops, dtype, Bsz, rows, stride, off, Cin, Cout, family):
    from mvlt_amd._lib import rowmap
    X = ints((Bsz * stride, Cin), -3, 3, dtype, 15)
    W, bias = ints((Cout, Cin), -3, 3, dtype, 16), ints(Cout, -9, 9, F32, 17)
    ostride, ooff = stride + 5, off + 3
    sel, osel = phys_rows(Bsz, rows, stride, off), phys_rows(Bsz, rows, ostride, ooff)
    ref = integral(X[sel].double() @ W.double().t() + bias.double())
    Y = torch.full((Bsz * ostride, Cout), 7.0, device=dev(), dtype=dtype)
    ops.gemm_nt(X, W, Y, Bsz * rows, Cout, Cin, Cin, Cin, Cout, a_map=rowmap(rows, stride, off), c_map=rowmap(rows, ostride, ooff), bias=bias)
    ran(family)
    exact(Y[osel], ref, "token sub-range")
    keep = torch.ones(Bsz * ostride, dtype=torch.bool, device=dev())
    keep[osel] = False
    assert (Y[keep] == 7.0).all(), "rows outside the map were written"
    return Y


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("rows,off", [(100, 0), (23, 100)])
def test_gemm_nt_token_subrange(ops, dtype, rows, off):
    """mode 0: A = a token sub-range of a (B, N, C) buffer, C written into the same range of another buffer; the other rows keep their sentinel"""
    fam = "gemm_nt_dma_kernel<128, 0, 1, 64" if dtype == BF else "gemm_nt_kernel<float, 128>"
    _nt_token_subrange(ops, dtype, 3, rows, 123, off, 72, 200, fam)


@pytest.mark.parametrize("hw,T,Cw", FLAKY_STAGES)
def test_gemm_nt_token_subrange_step_geometry(ops, hw, T, Cw):
    """the row geometry of the 256 px / T = 320 train step, fp32 operands, three times in-process: identical bits (integer sums do not depend on the order of anything, so a
    difference between runs is a race or an uninitialised read)"""
    fam = "gemm_nt_kernel<float, 64>" if Cw <= 64 else "gemm_nt_kernel<float, 128>"
    for rows, off in ((hw, 0), (T, hw)):
        runs = [_nt_token_subrange(ops, F32, 2, rows, hw + T, off, Cw, Cw, fam) for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("r,h_out,w_out,Cin,Cout", [(2, 3, 5, 16, 72), (4, 2, 3, 16, 40), (8, 3, 2, 16, 200)])
def test_gemm_nt_patch_gather_and_scatter(ops, dtype, r, h_out, w_out, Cin, Cout):
    """mode 1 on a non-square grid with text tokens behind the image tokens: the gather on A, and the scatter on C (its input gradient) with every row the map does not
    reach -- the text rows -- keeping its sentinel"""
    from mvlt_amd._lib import patchmap
    Bsz, T = 3, 7
    w_in, hw_in = r * w_out, r * h_out * r * w_out
    tokens = hw_in + T
    K, M = r * r * Cin, Bsz * h_out * w_out
    X = ints((Bsz * tokens, Cin), -3, 3, dtype, 18)
    W, bias = ints((Cout, K), -3, 3, dtype, 19), ints(Cout, -9, 9, F32, 20)
    pm = patchmap(r, w_in, tokens, h_out * w_out, w_out, Cin)
    narrow = "64" if Cout <= 64 else "128"
    ref = integral(gather_patch(X, Bsz, r, h_out, w_out, tokens).double() @ W.double().t() + bias.double())
    out = torch.full((M + 1, Cout), 7.0, device=dev(), dtype=dtype)
    ops.gemm_nt(X, W, out, M, Cout, K, Cin, K, Cout, a_map=pm, bias=bias)
    ran(f"gemm_nt_dma_kernel<{narrow}, 1, 1, 64" if dtype == BF else f"gemm_nt_kernel<float, {narrow}>")
    exact(out[:M], ref, "patch gather")
    assert (out[M] == 7.0).all()
    # scatter: dX[tokens] = dY @ Wk through the map, alone and added to what the buffer held (R aliasing C)
    dY, WkT = ints((M, Cout), -3, 3, dtype, 21), W.t().contiguous()
    prod = integral(dY.double() @ W.double())                                 # [M, K], K = (di, dj, c)
    want = torch.full((Bsz, tokens, Cin), 7.0, device=dev(), dtype=torch.float64)
    want[:, :hw_in] = prod.reshape(Bsz, h_out, w_out, r, r, Cin).permute(0, 1, 3, 2, 4, 5).reshape(Bsz, hw_in, Cin)
    dX = torch.full((Bsz * tokens, Cin), 7.0, device=dev(), dtype=dtype)
    ops.gemm_nt(dY, WkT, dX, M, K, Cout, Cout, Cout, Cin, c_map=pm)
    knar = "64" if K <= 64 else "128"
    ran(f"gemm_nt_dma_kernel<{knar}, 0, 6, 64" if dtype == BF else f"gemm_nt_kernel<float, {knar}>")
    exact(dX, want.reshape(Bsz * tokens, Cin), "patch scatter")
    base = ints((Bsz * tokens, Cin), -5, 5, dtype, 22)
    acc = base.clone()
    ops.gemm_nt(dY, WkT, acc, M, K, Cout, Cout, Cout, Cin, c_map=pm, R=acc)
    ran(f"gemm_nt_dma_kernel<{knar}, 0, 7, 64" if dtype == BF else f"gemm_nt_kernel<float, {knar}>")
    want2 = base.double().reshape(Bsz, tokens, Cin).clone()
    want2[:, :hw_in] += want[:, :hw_in]
    exact(acc, want2.reshape(Bsz * tokens, Cin), "patch scatter + R")


CONV3_NT = [  # h, w, Cin, Cout, variant, family (bf16), family (fp32)
    (8, 16, 64, 64, "plain", "conv3_nt_kernel<16, 64, 1>", "gemm_nt_kernel<float, 64>"),
    (8, 16, 64, 128, "acc", "conv3_nt_kernel<16, 128, 2>", "gemm_nt_kernel<float, 128>"),
    (4, 32, 64, 192, "stats", "conv3_nt_kernel<32, 192, 5>", "gemm_nt_kernel<float, 128>"),
    (2, 64, 128, 64, "strided", "conv3_nt_kernel<64, 64, 1>", "gemm_nt_kernel<float, 64>"),
    (5, 12, 16, 72, "plain", "gemm_nt_dma_kernel<128, 2, 1, 64", "gemm_nt_kernel<float, 128>"),       # not a halo shape: the generic gathered GEMM
    (5, 12, 16, 40, "acc", "gemm_nt_dma_kernel<64, 2, 2, 64", "gemm_nt_kernel<float, 64>"),
    (5, 12, 16, 192, "stats", "gemm_nt_dma_kernel<192, 2, 5, 64", "gemm_nt_kernel<float, 128>"),
    # three 128-pixel tiles per image: the interior tile's halo rows are a neighbouring tile's real pixels (above: one tile per image, every halo row zero padding
    # or inside the tile).  Two channel slices; two column tiles on BN 128 and on BN 192; the plain, statistics and residual epilogues
    (24, 16, 128, 256, "plain", "conv3_nt_kernel<16, 128, 1>", "gemm_nt_kernel<float, 128>"),
    (12, 32, 64, 384, "stats", "conv3_nt_kernel<32, 128, 5>", "gemm_nt_kernel<float, 128>"),       # (384 = 3 x 128: the 192-wide tile is for N % 128 != 0 only)
    (12, 32, 64, 576, "stats", "conv3_nt_kernel<32, 192, 5>", "gemm_nt_kernel<float, 128>"),       # three column tiles on BN 192
    (6, 64, 64, 128, "acc", "conv3_nt_kernel<64, 128, 2>", "gemm_nt_kernel<float, 128>"),
]
CONV3_DGRAD = [(24, 16, 64, 128, "conv3_nt_kernel<16, 64, 1>"), (12, 32, 192, 64, "conv3_nt_kernel<32, 192, 1>"), (6, 64, 128, 64, "conv3_nt_kernel<64, 128, 1>")]      # h, w, Cin, Cout, family


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("h,w,Cin,Cout,variant,fam_bf,fam_f32", CONV3_NT)
def test_gemm_nt_conv3x3_gather(ops, dtype, h, w, Cin, Cout, variant, fam_bf, fam_f32):
    """mode 2 on a rectangular h x w grid with text tokens behind the pixels of every image (never read: they hold 99): all four zero-padded borders, the LDS-halo kernel
    and the generic gather, with the epilogues the MIM decoder uses"""
    from mvlt_amd._lib import conv3map, rowmap
    Bsz, T = 3, 5
    tokens, M, K = h * w + T, Bsz * h * w, 9 * Cin
    lim = 1 if variant == "stats" else 3
    X = ints((Bsz, tokens, Cin), -lim, lim, dtype, 23)
    X[:, h * w:] = 99
    if variant == "stats":
        X[:, :, 7:] = 0                                                     # |C| <= 9 taps x 7 channels = 63
    W = ints((Cout, K), -lim, lim, dtype, 24)
    ref = integral(gather_3x3(X, Bsz, h, w, tokens).double() @ W.double().t())
    amap, fam = conv3map(h, w, tokens, Cin), (fam_bf if dtype == BF else fam_f32)
    if variant == "plain":
        for odt in (F32, dtype):
            out = torch.full((M + 1, Cout), 7.0, device=dev(), dtype=odt)
            ops.gemm_nt(X, W, out, M, Cout, K, Cin, K, Cout, a_map=amap)
            ran(fam)
            exact(out[:M], ref, f"conv3x3 {odt}")
            assert (out[M] == 7.0).all()
    elif variant == "acc":
        base = ints((M, Cout), -5, 5, F32, 25)
        out = base.clone()
        ops.gemm_nt(X, W, out, M, Cout, K, Cin, K, Cout, a_map=amap, R=out)
        ran(fam)
        exact(out, integral(ref + base.double()), "conv3x3 + R")
    elif variant == "stats":
        assert float(ref.abs().max()) <= 64
        for odt in ((F32, F16) if dtype == BF else (F32,)):
            out = torch.full((M, Cout), 7.0, device=dev(), dtype=odt)
            st = torch.zeros(2, 4, Cout, device=dev())
            ops.gemm_nt(X, W, out, M, Cout, K, Cin, K, Cout, a_map=amap, col_sum=st[0], col_sumsq=st[1], col_copies=4)
            ran(fam)
            exact(out, ref, f"conv3x3 {odt}")
            exact(st[0].sum(0), integral(ref.sum(0)), "col_sum")
            exact(st[1].sum(0), integral((ref * ref).sum(0)), "col_sumsq")
    else:
        stride, off = h * w + 7, 3
        buf = torch.full((Bsz * stride, Cout), 7.0, device=dev(), dtype=dtype)
        ops.gemm_nt(X, W, buf, M, Cout, K, Cin, K, Cout, a_map=amap, c_map=rowmap(h * w, stride, off))
        ran(fam)
        sel = phys_rows(Bsz, h * w, stride, off)
        exact(buf[sel], ref, "conv3x3, batch-strided rows")
        keep = torch.ones(Bsz * stride, dtype=torch.bool, device=dev())
        keep[sel] = False
        assert (buf[keep] == 7.0).all()


@pytest.mark.parametrize("h,w,Cin,Cout,family", CONV3_DGRAD)
def test_gemm_nt_conv3x3_input_gradient(ops, h, w, Cin, Cout, family):
    """the input gradient as the MIM decoder takes it: the same 3x3 gather over dz with flipped, transposed taps, three tiles per image.  The reference does not
    flip: dx[b, y, x, ci] = sum over (dy, dx, co) of dz[b, y - dy + 1, x - dx + 1, co] W[co, dy, dx, ci], tap by tap in float64"""
    from mvlt_amd._lib import conv3map
    Bsz, T = 3, 5
    tokens, M = h * w + T, Bsz * h * w
    dz = ints((Bsz, tokens, Cout), -3, 3, BF, 52)
    dz[:, h * w:] = 99
    Wk = ints((Cout, 3, 3, Cin), -3, 3, BF, 53)                                # [out][kh][kw][cin], the forward layout
    Wf = Wk.flip(1, 2).permute(3, 1, 2, 0).reshape(Cin, 9 * Cout).contiguous()      # [cin][flipped tap][out]
    pad = torch.zeros(Bsz, h + 2, w + 2, Cout, device=dev(), dtype=torch.float64)
    pad[:, 1:-1, 1:-1] = dz[:, : h * w].double().reshape(Bsz, h, w, Cout)
    ref = torch.zeros(Bsz, h, w, Cin, device=dev(), dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            ref += pad[:, 2 - dy: 2 - dy + h, 2 - dx: 2 - dx + w] @ Wk[:, dy, dx].double()
    ref = integral(ref.reshape(M, Cin))
    for odt in (F32, BF):
        out = torch.full((M + 1, Cin), 7.0, device=dev(), dtype=odt)
        ops.gemm_nt(dz, Wf, out, M, Cin, 9 * Cout, Cout, 9 * Cout, Cin, a_map=conv3map(h, w, tokens, Cout))
        ran(family)
        exact(out[:M], ref, f"conv3x3 input gradient {odt}")
        assert (out[M] == 7.0).all()


@pytest.mark.parametrize("N,K,M,odt", [(64, 72, 257, F32), (128, 200, 257, F32), (64, 72, 130, BF)])
def test_gemm_nt_layernorm_epilogue_c_part(ops, N, K, M, odt):
    """post_y: the C / R part of the LayerNorm epilogue is the residual epilogue and exact; the normalised rows and their statistics are checked against a
    float64 reference on exactly known rows, with per-row bars and guards, by tests/test_fusedln_edges_gpu.py (test_gemm_layernorm_epilogue)"""
    A, W, bias = ints((M, K), -3, 3, BF, 26), ints((N, K), -3, 3, BF, 27), ints(N, -9, 9, F32, 28)
    rps = M // 2 - 3
    scale = picks((M + rps - 1) // rps, [0.0, 0.5, 1.0, 2.0], 29)
    R = ints((M, N), -5, 5, odt, 30)
    ref = integral((A.double() @ W.double().t() + bias.double()) * scale.double().repeat_interleave(rps)[:M, None] + R.double(), 0.5)
    g, b = torch.ones(N, device=dev()), torch.zeros(N, device=dev())
    y = torch.zeros(M, N, device=dev(), dtype=BF)
    mean, rstd = torch.empty(M, device=dev()), torch.empty(M, device=dev())
    out = torch.full((M + 1, N), 7.0, device=dev(), dtype=odt)
    ops.gemm_nt(A, W, out, M, N, K, K, K, N, bias=bias, row_scale=scale, rows_per_scale=rps, R=R, post_ln=(g, b, 1e-6, y, mean, rstd))
    ran(f"gemm_nt_dma_kernel<{N}, 0, 8, 64")
    exact(out[:M], ref, "C beside post_y")
    assert (out[M] == 7.0).all() and torch.isfinite(y.float()).all()


# ================================================================== gemm_tn
def tn(A, B, Cw, M, N1, N2, *, lda=None, ldb=None, ldc=None, a_map=None, b_map=None, colsum_a=None, colsum_b=None, splits=0, trans_c=0, taps=0, seg=0, dgrad=None,
       partials=None, defer=False, overwrite=False):
    """mvlt_gemm_tn with every argument in the caller's hands (ops.gemm_tn swaps narrow operands by itself)"""
    from mvlt_amd import _lib as L
    a = L.GemmTNArgs(L.ptr(A), L.ptr(B), L.ptr(Cw), M, N1, N2, lda or A.shape[-1], ldb or B.shape[-1], ldc or Cw.shape[-1], L.DT[A.dtype],
                     a_map or L.rowmap(), b_map or L.rowmap(), L.ptr(colsum_a), splits, L.ptr(colsum_b), trans_c, taps, seg)
    if dgrad is not None:
        a.dgrad_wt, a.dgrad_out, a.dgrad_ld = L.ptr(dgrad[0]), L.ptr(dgrad[1]), dgrad[1].stride(0)
    if partials is not None:
        a.partials, a.partials_bytes, a.defer_fold = L.ptr(partials), partials.numel() * partials.element_size(), 1 if defer else 0
    a.c_overwrite = 1 if overwrite else 0
    L.check(L.lib.mvlt_gemm_tn(C_.byref(a), L.stream_ptr()), "mvlt_gemm_tn")


def tn_dma(N1, N2, bmode):
    """the instantiation mvlt_gemm_tn picks for a bf16 N1 x N2 output (its tile rule, restated): 64-wide tile sides for sides <= 64 and for outputs of at most 128 x 128"""
    small = N1 <= 128 and N2 <= 128
    bmt, bn = (64 if N1 <= 64 or small else 128), (64 if N2 <= 64 or small else 128)
    ns = {256: 2, 192: 3, 128: 4}[bmt + bn]
    return f"gemm_tn_dma_kernel<{bmt}, {bn}, {bmode}, {ns}, false>"


TN_ATOMIC = [  # dtype, M, N1, N2, splits, family: ragged tiles on both sides, M no multiple of the 64-row k-tile (nor of the split count)
    (BF, 200, 72, 100, 0, "gemm_tn_dma_kernel<64, 64, 3, 4, false>"),
    (BF, 200, 72, 100, 3, "gemm_tn_dma_kernel<64, 64, 3, 4, false>"),
    (BF, 1000, 136, 200, 5, "gemm_tn_dma_kernel<128, 128, 3, 2, false>"),
    (BF, 1000, 136, 40, 5, "gemm_tn_dma_kernel<128, 64, 3, 3, false>"),
    (BF, 1000, 40, 136, 5, "gemm_tn_dma_kernel<64, 128, 3, 3, false>"),
    (BF, 129, 30522, 72, 0, "gemm_tn_dma_kernel<128, 128, 3, 2, false>"),      # N1 = the vocabulary: not a multiple of 8 (lda padded to one)
    (BF, 129, 30522, 40, 0, "gemm_tn_dma_kernel<128, 64, 3, 3, false>"),
    (F32, 200, 136, 200, 0, "gemm_tn_kernel<float, 128>"),
    (F32, 200, 136, 200, 3, "gemm_tn_kernel<float, 128>"),
    (F32, 1000, 72, 40, 7, "gemm_tn_kernel<float, 64>"),
    (F32, 129, 30522, 36, 0, "gemm_tn_kernel<float, 64>"),
]


@pytest.mark.parametrize("dtype,M,N1,N2,splits,family", TN_ATOMIC)
def test_gemm_tn_atomic_path(ops, dtype, M, N1, N2, splits, family):
    """C += A^T B with fp32 atomics across the m-splits, colsum_a / colsum_b, and the transposed store: exact whatever the split count"""
    pc = 8 if dtype == BF else 4
    lda, ldb = (N1 + pc - 1) // pc * pc, (N2 + pc - 1) // pc * pc
    A, B = ints((M, N1), -3, 3, dtype, 31), ints((M, N2), -3, 3, dtype, 32)
    Ap, Bp = pad_cols(A, lda, 99), pad_cols(B, ldb, 99)                        # the padding columns are never part of the product
    ref = integral(A.double().t() @ B.double())
    ldc = N2 + 4
    Cw, cs = torch.full((N1 + 1, ldc), 3.0, device=dev()), torch.full((N1 + 1,), 3.0, device=dev())
    tn(Ap, Bp, Cw, M, N1, N2, colsum_a=cs, splits=splits)
    ran(family)
    exact(Cw[:N1, :N2], ref + 3.0, "C += A^T B")
    exact(cs[:N1], integral(A.double().sum(0)) + 3.0, "colsum_a")
    assert (Cw[N1] == 3.0).all() and (Cw[:, N2:] == 3.0).all() and float(cs[N1]) == 3.0, "wrote outside N1 x N2"
    Ct, cb = torch.full((N2 + 1, N1 + 4), 3.0, device=dev()), torch.full((N2 + 1,), 3.0, device=dev())
    tn(Ap, Bp, Ct, M, N1, N2, colsum_b=cb, splits=splits, trans_c=1)
    ran(family)
    exact(Ct[:N2, :N1], ref.t() + 3.0, "trans_c")
    exact(cb[:N2], integral(B.double().sum(0)) + 3.0, "colsum_b")
    assert (Ct[N2] == 3.0).all() and (Ct[:, N1:] == 3.0).all() and float(cb[N2]) == 3.0


def _tn_token_subrange(dtype, Bsz, rows, stride, off, N1, N2, family):
    from mvlt_amd._lib import rowmap
    A, B = ints((Bsz * stride, N1), -3, 3, dtype, 33), ints((Bsz * (stride + 5), N2), -3, 3, dtype, 34)
    sa, sb = phys_rows(Bsz, rows, stride, off), phys_rows(Bsz, rows, stride + 5, off + 2)
    ref = integral(A[sa].double().t() @ B[sb].double())
    Cw, cs = torch.zeros(N1, N2, device=dev()), torch.zeros(N1, device=dev())
    tn(A, B, Cw, Bsz * rows, N1, N2, a_map=rowmap(rows, stride, off), b_map=rowmap(rows, stride + 5, off + 2), colsum_a=cs)
    ran(family)
    exact(Cw, ref, "token sub-ranges")
    exact(cs, A[sa].double().sum(0), "colsum_a")
    return Cw


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("rows,off", [(100, 0), (23, 100)])
def test_gemm_tn_token_subrange(ops, dtype, rows, off):
    _tn_token_subrange(dtype, 3, rows, 123, off, 72, 200, tn_dma(72, 200, 0) if dtype == BF else "gemm_tn_kernel<float, 128>")


@pytest.mark.parametrize("hw,T,Cw", FLAKY_STAGES)
def test_gemm_tn_token_subrange_step_geometry(ops, hw, T, Cw):
    """the row geometry of the 256 px / T = 320 step, fp32 operands, three runs with identical bits"""
    fam = "gemm_tn_kernel<float, 64>" if Cw <= 64 else "gemm_tn_kernel<float, 128>"
    for rows, off in ((hw, 0), (T, hw)):
        runs = [_tn_token_subrange(F32, 2, rows, hw + T, off, Cw, Cw, fam) for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("r,h_out,w_out,Cin,Cout", [(2, 3, 5, 16, 72), (4, 2, 3, 16, 40), (8, 3, 2, 16, 136)])
def test_gemm_tn_patch_gather_and_taps(ops, dtype, r, h_out, w_out, Cin, Cout):
    """b_map mode 1 (non-square grid, text tokens behind the image) with the plain [out][tap][cin] output and with c_taps = 4 / 16 / 64: logical column tap*c_seg + c
    lands at c*c_taps + tap, nn.Conv2d's [out][cin][kh][kw]"""
    from mvlt_amd._lib import patchmap
    Bsz, T = 3, 7
    w_in, hw_in = r * w_out, r * h_out * r * w_out
    tokens, K, M = hw_in + T, r * r * Cin, Bsz * h_out * w_out
    X, dY = ints((Bsz * tokens, Cin), -3, 3, dtype, 35), ints((M, Cout), -3, 3, dtype, 36)
    pm = patchmap(r, w_in, tokens, h_out * w_out, w_out, Cin)
    ref = integral(dY.double().t() @ gather_patch(X, Bsz, r, h_out, w_out, tokens).double())       # [Cout][tap][cin]
    if dtype == BF:
        fam = tn_dma(Cout, K, 1)
    else:
        fam = f"gemm_tn_kernel<float, {64 if K <= 64 else 128}>"
    dW, cs = torch.full((Cout + 1, K), 3.0, device=dev()), torch.zeros(Cout, device=dev())
    tn(dY, X, dW, M, Cout, K, b_map=pm, colsum_a=cs, splits=2)
    ran(fam)
    exact(dW[:Cout], ref + 3.0, "patch gather")
    exact(cs, dY.double().sum(0), "colsum_a")
    assert (dW[Cout] == 3.0).all()
    dWt = torch.full((Cout + 1, K), 3.0, device=dev())
    tn(dY, X, dWt, M, Cout, K, b_map=pm, splits=2, taps=r * r, seg=Cin)
    ran(fam)
    exact(dWt[:Cout], ref.reshape(Cout, r * r, Cin).permute(0, 2, 1).reshape(Cout, K) + 3.0, "c_taps")
    assert (dWt[Cout] == 3.0).all()


CONV3_TN = [(4, 16, 64, 64, "conv3_wgrad_kernel<16>"), (8, 8, 64, 128, "conv3_wgrad_kernel<8>"), (2, 32, 128, 64, "conv3_wgrad_kernel<32>"), (1, 64, 64, 64, "conv3_wgrad_kernel<64>"),
            (5, 12, 16, 72, "gemm_tn_dma_kernel<128, 128, 2, 2, false>"), (5, 12, 8, 40, "gemm_tn_dma_kernel<64, 64, 2, 4, false>"),
            # three 64-pixel k-tiles per image (the middle one's halo rows are its neighbours' pixels), two output and two channel slices: n_o n_c = 4
            (24, 8, 128, 128, "conv3_wgrad_kernel<8>"), (12, 16, 128, 128, "conv3_wgrad_kernel<16>"), (6, 32, 128, 128, "conv3_wgrad_kernel<32>"),
            (3, 64, 128, 128, "conv3_wgrad_kernel<64>")]


@pytest.mark.parametrize("h,w,Cin,Cout,family", CONV3_TN)
def test_gemm_tn_conv3x3_gather(ops, h, w, Cin, Cout, family):
    """b_map mode 2 on a rectangular grid with text tokens behind the pixels (they hold 99 and are never read): the LDS-halo kernel at its four widths, the generic
    gather, fp32 operands on the generic kernel, and c_taps = 9 (which the halo kernel does not carry: the generic gather then)"""
    from mvlt_amd._lib import conv3map
    Bsz, T = 3, 5
    tokens, M, K = h * w + T, Bsz * h * w, 9 * Cin
    X, dY = ints((Bsz, tokens, Cin), -3, 3, BF, 37), ints((M, Cout), -3, 3, BF, 38)
    X[:, h * w:] = 99
    bm = conv3map(h, w, tokens, Cin)
    ref = integral(dY.double().t() @ gather_3x3(X, Bsz, h, w, tokens).double())
    for dtype in (BF, F32):
        dW = torch.full((Cout + 1, K), 3.0, device=dev())
        tn(dY.to(dtype), X.to(dtype), dW, M, Cout, K, b_map=bm)
        ran(family if dtype == BF else "gemm_tn_kernel<float, 128>")
        exact(dW[:Cout], ref + 3.0, f"conv3x3 weight gradient {dtype}")
        assert (dW[Cout] == 3.0).all()
    dWt = torch.full((Cout + 1, K), 3.0, device=dev())
    tn(dY, X, dWt, M, Cout, K, b_map=bm, taps=9, seg=Cin)
    ran(tn_dma(Cout, K, 2))
    exact(dWt[:Cout], ref.reshape(Cout, 9, Cin).permute(0, 2, 1).reshape(Cout, K) + 3.0, "c_taps 9")


@pytest.mark.parametrize("M,N1,N2,ldc,family", [(200, 72, 100, 104, "gemm_tn_dma_kernel<64, 64, 3, 4, false>"), (1000, 500, 264, 272, "gemm_tn_dma_kernel<128, 128, 3, 2, false>"),
                                                (129, 30522, 72, 72, "gemm_tn_dma_kernel<128, 128, 3, 2, false>")])
def test_gemm_tn_overwrite(ops, M, N1, N2, ldc, family):
    """c_overwrite: C = A^T B by one m-split and plain stores.  C holds a sentinel first: afterwards every element is the reference, the guard row and the guard columns
    keep the sentinel; the bias gradient still accumulates."""
    lda = (N1 + 7) // 8 * 8
    A, B = ints((M, N1), -3, 3, BF, 39), ints((M, N2), -3, 3, BF, 40)
    ldb = (N2 + 7) // 8 * 8
    Ap, Bp = pad_cols(A, lda, 99), pad_cols(B, ldb, 99)
    ref = integral(A.double().t() @ B.double())
    Cw, cs = torch.full((N1 + 1, ldc), 7.0, device=dev()), torch.full((N1,), 1.0, device=dev())
    tn(Ap, Bp, Cw, M, N1, N2, ldc=ldc, colsum_a=cs, overwrite=True)
    ran(family)
    exact(Cw[:N1, :N2], ref, "c_overwrite")
    assert (Cw[N1] == 7.0).all() and (Cw[:, N2:] == 7.0).all()
    exact(cs, A.double().sum(0) + 1.0, "colsum_a")
    from mvlt_amd._lib import rowmap                                           # mapped rows (the header allows them): a token sub-range of both operands
    rows, stride, off, Bsz = M // 4, M // 4 + 9, 4, 3
    A2, B2 = ints((Bsz * stride, lda), -3, 3, BF, 41), ints((Bsz * stride, ldb), -3, 3, BF, 42)
    sel = phys_rows(Bsz, rows, stride, off)
    Cw = torch.full((N1 + 1, ldc), 7.0, device=dev())
    tn(A2, B2, Cw, Bsz * rows, N1, N2, ldc=ldc, a_map=rowmap(rows, stride, off), b_map=rowmap(rows, stride, off), overwrite=True)
    ran(family.replace(", 3, ", ", 0, ", 1))
    exact(Cw[:N1, :N2], integral(A2[sel][:, :N1].double().t() @ B2[sel][:, :N2].double()), "c_overwrite, mapped rows")
    assert (Cw[N1] == 7.0).all() and (Cw[:, N2:] == 7.0).all()


@pytest.mark.parametrize("Cw,M", [(64, 64 * 9 + 17), (128, 64 * 9 + 40), (64, 130), (128, 4224)])
def test_gemm_tn_fused_input_gradient(ops, Cw, M):
    """dgrad_out: dW += dY^T X, db += colsum(dY) and dX = dY W from one pass over dY; the bf16 dX is the exact product rounded once, in a row-strided view whose
    neighbours keep their sentinel"""
    dY, X = ints((M, Cw), -3, 3, BF, 43), ints((M, Cw), -3, 3, BF, 44)
    WT = ints((Cw, Cw), -3, 3, BF, 45)                                         # W^T [in][out]
    dW, db = torch.full((Cw, Cw), 3.0, device=dev()), torch.zeros(Cw, device=dev())
    wide = torch.full((M + 1, 2 * Cw), 7.0, device=dev(), dtype=BF)
    for splits in (0, 3):
        dW.fill_(3.0), db.zero_(), wide.fill_(7.0)
        tn(dY, X, dW, M, Cw, Cw, colsum_a=db, splits=splits, dgrad=(WT, wide[:, Cw:]))
        ran("gemm_tn_dma_kernel<64, 64, 3, 4, true>" if Cw == 64 else "gemm_tn_dma_kernel<128, 128, 3, 2, true>")
        exact(dW, integral(dY.double().t() @ X.double()) + 3.0, "dW")
        exact(db, dY.double().sum(0), "db")
        exact(wide[:M, Cw:], integral(dY.double() @ WT.double().t()), "dX")
        assert (wide[:, :Cw] == 7.0).all() and (wide[M] == 7.0).all()


def _partial_operands(M, N1, N2, swap, gather=None):
    """A sparse +-1 (n1 % P == m % P, P = M / 128: exactly 128 nonzero rows per column, at least one nonzero per row) against a dense B in {+-1, +-2}, or the roles
    swapped: |partial sum| <= sum |a| |b| <= 128 x 2 = 256 for ANY subset of the rows, so every bf16 partial tile holds its integer exactly"""
    P = (M + 127) // 128

    def dense(n, seed):
        v = ints((M, n), 0, 3, F32, seed)
        return (torch.where(v < 2, v - 2, v - 1)).to(BF)                       # {-2, -1, 1, 2}
    if not swap:
        return sparse_pm1(M, N1, P, BF, 46), dense(N2, 47)
    return dense(N1, 48), sparse_pm1(M, N2, P, BF, 49)


TN_PARTIAL = [  # route, M, N1, N2, family of the GEMM
    ("a", 16384, 1024, 1024, "gemm_tn_p8_kernel<4, 2, 2, true, false, false>"),
    ("a", 49152, 512, 2048, "gemm_tn_p8_kernel<4, 2, 2, true, false, false>"),
    ("a", 45056, 1280, 320, "gemm_tn_p8_kernel<3, 3, 2, true, true, false>"),        # 192 x 320 tiles, the last row tile ragged
    ("a", 45056, 320, 1280, "gemm_tn_p8_kernel<3, 3, 2, false, true, true>"),        # ... with swapped operands
    ("a", 49152, 1152, 320, "gemm_tn_p8_kernel<3, 3, 2, true, false, false>"),
    ("b", 5000, 200, 136, "gemm_tn_dma_kernel<128, 128, 3, 2, false>"),              # ragged tiles, a ragged last k-tile and a short last split
    ("b", 28672, 320, 320, "gemm_tn_dma_kernel<128, 128, 3, 2, false>"),
    ("b", 8192, 64, 768, "gemm_tn_dma_kernel<64, 128, 3, 3, false>"),                # text_embed1's 64 x 768
]


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("route,M,N1,N2,family", TN_PARTIAL)
def test_gemm_tn_partial_tiles(ops, route, M, N1, N2, family, swap):
    """bf16 partial tiles + the ordered fold on the 8-phase kernel (a) and the 128-wide kernel (b): the immediate fold, the deferred fold behind tn_fold_flush, several
    deferring launches sharing one scratch and the atomic path (no scratch) all equal the integer reference bit for bit"""
    A, B = _partial_operands(M, N1, N2, swap)
    assert float((A.abs().double().t() @ B.abs().double()).max()) <= 256
    ref = integral(A.double().t() @ B.double())
    sa = integral(A.double().sum(0))
    scratch = torch.empty(96 * 1024 * 1024, device=dev(), dtype=BF)

    def run(**kw):
        Cw, cs = torch.full((N1 + 1, N2), 3.0, device=dev()), torch.zeros(N1 + 8, device=dev())
        tn(A, B, Cw, M, N1, N2, colsum_a=cs[:N1], **kw)
        return Cw, cs

    def check(Cw, cs, what):
        exact(Cw[:N1], ref + 3.0, what)
        exact(cs[:N1], sa, what + ", colsum_a")
        assert (Cw[N1] == 3.0).all() and (cs[N1:] == 0).all(), "wrote past the last row"

    Cw, cs = run(partials=scratch)
    ran("tn_fold_kernel")
    check(Cw, cs, "immediate fold")
    Cw, cs = run(partials=scratch, defer=True)
    ran(family)
    assert (Cw == 3.0).all(), "a deferring launch touched C before the flush"
    ops.tn_fold_flush(scratch)
    ran("tn_fold_multi_kernel")
    check(Cw, cs, "deferred fold")
    three = [run(partials=scratch, defer=True) for _ in range(3)]
    ops.tn_fold_flush(scratch)
    ran("tn_fold_multi_kernel")
    for i, (Cw, cs) in enumerate(three):
        check(Cw, cs, f"shared scratch, launch {i}")
    Cw, cs = run()
    ran("gemm_tn_dma_kernel<")
    check(Cw, cs, "atomic path")


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("h,w,Bsz,Cin,Cout,family", [(32, 32, 4, 64, 64, "conv3_wgrad_kernel<32>"), (16, 16, 16, 64, 128, "conv3_wgrad_kernel<16>"),
                                                     # three k-tiles per image, 22 images = 66 k-tiles = 4 splits of 17: a split ends inside an image
                                                     (24, 8, 22, 128, 128, "conv3_wgrad_kernel<8>"), (12, 16, 22, 128, 128, "conv3_wgrad_kernel<16>"),
                                                     (6, 32, 22, 128, 128, "conv3_wgrad_kernel<32>"), (3, 64, 22, 128, 128, "conv3_wgrad_kernel<64>")])
def test_gemm_tn_partial_tiles_conv3x3(ops, h, w, Bsz, Cin, Cout, family, swap):
    """route (c): the conv3x3 weight-gradient kernel with >= 4 m-splits.  The bound of 256 is asserted on the gathered operand."""
    from mvlt_amd._lib import conv3map
    M, K = Bsz * h * w, 9 * Cin
    A, Bx = _partial_operands(M, Cout, Cin, swap)
    G = gather_3x3(Bx, Bsz, h, w, h * w)
    assert float((A.abs().double().t() @ G.abs().double()).max()) <= 256
    ref = integral(A.double().t() @ G.double())
    bm = conv3map(h, w, h * w, Cin)
    scratch = torch.empty(16 * 1024 * 1024, device=dev(), dtype=BF)

    def run(**kw):
        Cw = torch.full((Cout + 1, K), 3.0, device=dev())
        tn(A, Bx, Cw, M, Cout, K, b_map=bm, **kw)
        return Cw

    def check(Cw, what):
        exact(Cw[:Cout], ref + 3.0, what)
        assert (Cw[Cout] == 3.0).all()

    Cw = run(partials=scratch)
    ran("tn_fold_kernel")
    check(Cw, "immediate fold")
    Cw = run(partials=scratch, defer=True)
    ran(family)
    ops.tn_fold_flush(scratch)
    ran("tn_fold_multi_kernel")
    check(Cw, "deferred fold")
    three = [run(partials=scratch, defer=True) for _ in range(3)]
    ops.tn_fold_flush(scratch)
    for i, Cw in enumerate(three):
        check(Cw, f"shared scratch, launch {i}")
    Cw = run()
    ran(family)
    check(Cw, "atomic path")


def test_gemm_tn_bf16_past_2_24_rows(ops):
    """M >= 2^24 is where the dispatcher leaves the LDS-DMA kernel for the generic one with bf16 operands.  A is nonzero in every 16th row only: |C| <= 2^20 x 9."""
    M, N = 1 << 24, 8
    blk = 4096
    a, b = ints((blk, N), -3, 3, BF, 50), ints((blk, N), -3, 3, BF, 51)
    a[torch.arange(blk, device=dev()) % 16 != 0] = 0
    A, B = a.repeat(M // blk, 1), b.repeat(M // blk, 1)
    ref = integral((a.double().t() @ b.double()) * (M // blk))
    Cw, cs = torch.zeros(N, N, device=dev()), torch.zeros(N, device=dev())
    tn(A, B, Cw, M, N, N, colsum_a=cs)
    ran("gemm_tn_kernel<__hip_bfloat16, 64>")
    exact(Cw, ref, "C")
    exact(cs, integral(a.double().sum(0) * (M // blk)), "colsum_a")


# ================================================================== reductions and glue kernels
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("Bsz", [1, 2, 17, 33])
def test_batch_sum(ops, dtype, Bsz):
    """the batch is split over 16 thread groups (B below, at and above 16 and 32); R * C / 8 = 185 items: the last workgroup is part empty; rows from `split` on are ADDED
    to acc2, for split = 0, inside and = R"""
    R, Cd, ld, extra = 37, 40, 48, 3
    assert (R * Cd // 8) % 16 != 0
    x = ints((Bsz, R + extra, ld), -3, 3, dtype, 52)
    want = integral(x[:, :R, :Cd].double().sum(0))
    out = torch.full((R + 1, Cd), 7.0, device=dev())
    ops.batch_sum(x, out, Bsz, R, Cd, R + extra, ld)
    ran("batch_sum_kernel<")
    exact(out[:R], want, "batch_sum")
    assert (out[R] == 7.0).all()
    for split in (0, 30, R):
        out = torch.full((R + 1, Cd), 7.0, device=dev())
        acc = torch.full((R - split + 1, Cd), 5.0, device=dev())
        ops.batch_sum(x, out, Bsz, R, Cd, R + extra, ld, acc2=acc, split=split)
        exact(out[:split], want[:split], f"rows below split {split}")
        assert (out[split:] == 7.0).all(), "rows from split on belong to acc2"
        exact(acc[: R - split], want[split:] + 5.0, f"acc2, split {split}")
        assert (acc[R - split] == 5.0).all()


@pytest.mark.parametrize("hw,T,Cw", FLAKY_STAGES)
def test_batch_sum_step_geometry(ops, hw, T, Cw):
    """the pos-embed gradients of the 256 px / T = 320 step (B = 2): image rows stored, text rows added to acc2; three runs, identical bits"""
    x = ints((2, hw + T, Cw), -3, 3, F32, 53)
    want = integral(x.double().sum(0))
    runs = []
    for _ in range(3):
        out, acc = torch.full((hw + T, Cw), 7.0, device=dev()), torch.full((T, Cw), 5.0, device=dev())
        ops.batch_sum(x, out, 2, hw + T, Cw, hw + T, Cw, acc2=acc, split=hw)
        exact(out[:hw], want[:hw], "image rows")
        exact(acc, want[hw:] + 5.0, "text rows")
        assert (out[hw:] == 7.0).all()
        runs.append(torch.cat([out, acc]))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("copies", [1, 4, 31, 32, 64, 256, 300])
def test_fold_copies(ops, copies):
    """dst[dst_index[j]] += sum_k arena[k * stride + j] over [j0, j1), those arena elements zeroed again: the narrow kernel below 32 copies, the wide one from 32 on"""
    j0, j1, stride = 13, 13 + 333, 400
    assert (j1 - j0) % 64 != 0
    arena = ints((copies, stride), -3, 3, F32, 54)
    if copies > 1:
        arena[copies // 2] = 0                                                 # (a copy no workgroup wrote)
    before = arena.clone()
    g = torch.Generator(device="cpu").manual_seed(55)
    index = (torch.randperm(stride, generator=g) * 2 + 1).to(torch.int32).to(dev())            # a permutation into the odd slots of dst
    dst = ints(2 * stride + 2, -9, 9, F32, 56)
    want = dst.double().clone()
    want[index[j0:j1].long()] += integral(before[:, j0:j1].double().sum(0))
    ops.fold_copies(arena, copies, stride, index, j0, j1, dst)
    ran("fold_copies_wide_kernel" if copies >= 32 else "fold_copies_kernel")
    exact(dst, want, "dst")
    assert (arena[:, j0:j1] == 0).all(), "the folded range must be zero again"
    assert torch.equal(arena[:, :j0], before[:, :j0]) and torch.equal(arena[:, j1:], before[:, j1:]), "the arena outside [j0, j1) was touched"


@pytest.mark.parametrize("rows", [1, 777])
def test_add_column_sums(ops, rows):
    from mvlt_amd import _lib as L
    cols, ld = 136, 144
    x = ints((rows, ld), -3, 3, F32, 57)
    want = integral(x[:, :cols].double().sum(0))
    for n0 in (0, cols // 2, cols):
        d0, d1 = torch.full((n0 + 1,), 3.0, device=dev()), torch.full((cols - n0 + 1,), 5.0, device=dev())
        L.check(L.lib.mvlt_add_column_sums(x.data_ptr(), rows, cols, ld, d0.data_ptr(), n0, None if n0 == cols else d1.data_ptr(), L.stream_ptr()), "mvlt_add_column_sums")
        ran("add_column_sums_kernel")
        exact(d0[:n0], want[:n0] + 3.0, f"dst0, n0 = {n0}")
        assert float(d0[n0]) == 3.0 and float(d1[cols - n0]) == 5.0
        if n0 < cols:
            exact(d1[: cols - n0], want[n0:] + 5.0, f"dst1, n0 = {n0}")
        else:
            assert (d1 == 5.0).all()


@pytest.mark.parametrize("M,Cd,ldz", [(5000, 64, 72), (777, 6, 6), (3001, 192, 192), (1, 40, 40)])
def test_col_stats_and_bn_finalize_sums(ops, M, Cd, ldz):
    """col_stats adds the column sums and sums of squares; bn_finalize sums the copies: with M a power of two in its argument the mean it stores is that sum, scaled exactly"""
    z = ints((M, ldz), -8, 8, F32, 58)
    s, ss = torch.full((Cd + 1,), 3.0, device=dev()), torch.full((Cd + 1,), 5.0, device=dev())
    ops.col_stats(z, ldz, M, Cd, s, ss)
    ran("col_reduce")
    zz = z[:, :Cd].double()
    exact(s[:Cd], integral(zz.sum(0)) + 3.0, "sum")
    exact(ss[:Cd], integral((zz * zz).sum(0)) + 5.0, "sumsq")
    assert float(s[Cd]) == 3.0 and float(ss[Cd]) == 5.0
    for copies in (1, 4, 16):
        cs, cq = ints((copies, Cd), -1000, 1000, F32, 59), ints((copies, Cd), 0, 1000, F32, 60)
        mean, rstd = torch.empty(Cd + 1, device=dev()).fill_(7.0), torch.empty(Cd, device=dev())
        ops.bn_finalize(cs, cq, 4096, Cd, 1e-5, 0.1, mean, rstd, copies=copies)
        ran("bn_finalize_kernel")
        exact(mean[:Cd] * 4096.0, integral(cs.double().sum(0)), f"mean x M, {copies} copies")
        assert float(mean[Cd]) == 7.0


def test_head_grad_prep(ops):
    for Bsz, n in ((256, 2), (64, 48), (37, 122), (300, 250)):
        n_pad = (n + 7) // 8 * 8
        dlog = ints((Bsz, n), -3, 3, F32, 61 + n)
        want = integral(dlog.double().sum(0))
        for dt in (BF, F32):
            dl = torch.full((Bsz + 1, n_pad), 9.0, device=dev(), dtype=dt)
            b1, b2 = torch.full((n + 1,), 1.0, device=dev()), torch.full((n + 1,), 2.0, device=dev())
            ops.head_grad_prep(dlog, dl[:Bsz], b1, b2)
            ran("head_grad_prep_kernel<")
            assert torch.equal(dl[:Bsz, :n], dlog.to(dt)) and (dl[:Bsz, n:] == 0).all() and (dl[Bsz] == 9.0).all()
            exact(b1[:n], want + 1.0, "db1")
            exact(b2[:n], want + 2.0, "db2")
            assert float(b1[n]) == 1.0 and float(b2[n]) == 2.0
            b1.fill_(1.0)
            ops.head_grad_prep(dlog, dl[:Bsz], b1, None)
            exact(b1[:n], want + 1.0, "db1 alone")


def _ln_dbeta(ops, dtype, rows, Cd, copies, dy_map, n_phys, seed):
    """dbeta = sum of the dy rows the map selects: exact for integer dy whatever gamma, x, mean and rstd are"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dy = ints((n_phys, Cd), -3, 3, dtype, seed)
    x = torch.randn(rows, Cd, generator=g).to(dev())
    gamma, mean, rstd = torch.randn(Cd, generator=g).to(dev()), torch.randn(rows, generator=g).to(dev()), torch.rand(rows, generator=g).to(dev()) + 0.5
    dx = torch.empty(rows, Cd, device=dev())
    stride = 2 * Cd + 24                                                       # copy_stride > 2 C: dgamma | dbeta | a gap that must stay zero
    arena = torch.zeros(max(copies, 1), stride, device=dev())
    ops.layernorm_bwd(dy, x, dx, gamma, mean, rstd, rows, Cd, Cd, Cd, Cd, dgamma=arena[0, :Cd], dbeta=arena[0, Cd:], dy_map=dy_map, copies=copies, copy_stride=stride)
    ran("ln_bwd_kernel<")
    assert (arena[:, 2 * Cd:] == 0).all(), "wrote between the copies"
    dst = torch.full((2 * Cd + 1,), 3.0, device=dev())
    index = torch.arange(2 * Cd, device=dev(), dtype=torch.int32)
    ops.fold_copies(arena, max(copies, 1), stride, index, 0, 2 * Cd, dst)
    assert (arena == 0).all() and float(dst[2 * Cd]) == 3.0
    return dst[Cd: 2 * Cd]


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("copies", [1, 4, 64, 256])
@pytest.mark.parametrize("Cd", [64, 128, 320, 512, 768])
def test_layernorm_bwd_dbeta(ops, dtype, Cd, copies):
    """rows chosen per width so that one launch has fewer workgroups than 4 and 64 copies and the other more (256 copies: the cap on the workgroups); mapped dy as the
    schedule uses it: rowmap(HW, N, 0) for the image rows and rowmap(T, N, HW) for the text rows"""
    from mvlt_amd._lib import rowmap
    per_wg = {64: 128, 128: 64, 320: 32, 512: 16, 768: 16}[Cd]                 # rows per workgroup of 1024 threads (launch_bwd in csrc/norm.hip)
    for Bsz, HW, T in ((2, per_wg + 1, 5), (3, 34 * per_wg + 1, 9)):              # 3 workgroups, and 103 (capped to the copies from 64 copies on)
        N = HW + T
        for rows, off, seed in ((HW, 0, 62), (T, HW, 63)):
            dyfull = ints((Bsz * N, Cd), -3, 3, dtype, seed)
            want = integral(dyfull[phys_rows(Bsz, rows, N, off)].double().sum(0))
            got = _ln_dbeta(ops, dtype, Bsz * rows, Cd, copies, rowmap(rows, N, off), Bsz * N, seed)
            exact(got, want + 3.0, f"dbeta, B {Bsz} rows {rows} offset {off}")


@pytest.mark.parametrize("hw,T,Cw", FLAKY_STAGES)
def test_layernorm_bwd_dbeta_step_geometry(ops, hw, T, Cw):
    """the norm backward of the 256 px / T = 320 step (B = 2, fp32), image rows and text rows, three runs with identical bits"""
    from mvlt_amd._lib import rowmap
    N = hw + T
    for rows, off, seed in ((hw, 0, 64), (T, hw, 65)):
        dyfull = ints((2 * N, Cw), -3, 3, F32, seed)
        want = integral(dyfull[phys_rows(2, rows, N, off)].double().sum(0))
        runs = [_ln_dbeta(ops, F32, 2 * rows, Cw, 256, rowmap(rows, N, off), 2 * N, seed) for _ in range(3)]
        exact(runs[0], want + 3.0, f"dbeta rows {rows} offset {off}")
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_cast_bf16_every_rounding_case(ops):
    """every fp32 pattern whose low half is 0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001 or 0xFFFF (393 216 values): exact, both directions of a tie, subnormals, +-Inf, +-0, NaN"""
    hi = torch.arange(65536, dtype=torch.int64)[:, None] << 16
    lo = torch.tensor([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64)[None, :]
    bits = (hi | lo).reshape(-1)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    src = bits.view(F32).to(dev())
    assert src.numel() == 393216
    dst = torch.zeros(src.numel() + 4, device=dev(), dtype=BF)
    ops.cast_bf16(src, dst, src.numel())
    ran("cast_f32_bf16_kernel")
    want = src.to(BF)
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(dst[:-4]), nan), "NaN must stay NaN and nothing else become one"
    bad = (dst[:-4].view(torch.int16) != want.view(torch.int16)) & ~nan
    assert not bad.any(), f"{int(bad.sum())} wrong; first fp32 patterns {[hex(int(b) & 0xFFFFFFFF) for b in bits.to(dev())[bad][:8]]}"
    assert (dst[-4:] == 0).all()


def test_loss_compose(ops):
    losses = [torch.tensor([v], device=dev()) for v in (0.75, 2.5, 0.125, 3.0, 1.5)]
    weights = [1.0, 0.5, 2.0, 0.25, 10.0]
    for off in (None, 0, 1, 2, 3, 4):
        ls = [None if i == off else t for i, t in enumerate(losses)]
        terms = [0.0 if i == off else float(t) * w for i, (t, w) in enumerate(zip(losses, weights))]
        out, total = torch.full((7,), 9.0, device=dev()), torch.full((2,), 9.0, device=dev())
        ops.loss_compose(ls, weights, out, total)
        ran("loss_compose_kernel")
        assert out.tolist() == [sum(terms)] + terms + [9.0] and total.tolist() == [sum(terms), 9.0] and float(out[0]) == float(total[0])


@pytest.mark.parametrize("dtype", [BF, F32])
def test_gather_scatter_rows(ops, dtype):
    from mvlt_amd._lib import rowmap
    Bsz, rows, stride, off, Cd, ld = 3, 50, 61, 7, 72, 80
    src = ints((Bsz * stride, ld), -99, 99, dtype, 66)
    g = torch.Generator(device="cpu").manual_seed(67)
    idx = torch.randperm(Bsz * rows, generator=g)[:77].to(torch.int32).to(dev())
    phys = phys_rows(Bsz, rows, stride, off)[idx.long()]
    out = torch.full((78, Cd), 7.0, device=dev(), dtype=dtype)
    ops.gather_rows(src, idx, out, 77, Cd, ld, src_map=rowmap(rows, stride, off))
    ran("gather_rows_kernel<")
    assert torch.equal(out[:77], src[phys, :Cd]) and (out[77] == 7.0).all()
    plain = torch.full((78, Cd), 7.0, device=dev(), dtype=dtype)
    ops.gather_rows(src, idx, plain, 77, Cd, ld)
    assert torch.equal(plain[:77], src[idx.long(), :Cd])
    for accumulate in (False, True):
        dst = ints((Bsz * stride, ld), -99, 99, dtype, 68)
        want = dst.clone()
        want[phys, :Cd] = (want[phys, :Cd] + out[:77]) if accumulate else out[:77]
        ops.scatter_rows(out, idx, dst, 77, Cd, ld, dst_map=rowmap(rows, stride, off), accumulate=accumulate)
        ran("scatter_rows_kernel<")
        assert torch.equal(dst, want), f"scatter_rows accumulate={accumulate}"


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("R,Cc", [(77, 130), (33, 31), (64, 64)])
def test_transpose_cast(ops, dtype, R, Cc):
    w = ints((R, Cc), -200, 200, F32, 69)
    ld = R + 3
    out = torch.full((Cc + 1, ld), 7.0, device=dev(), dtype=dtype)
    ops.transpose_cast(w, out, R, Cc, ld)
    ran("transpose_cast_kernel<")
    assert torch.equal(out[:Cc, :R], w.t().to(dtype)) and (out[:Cc, R:] == 7.0).all() and (out[Cc] == 7.0).all()

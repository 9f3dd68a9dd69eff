"""CPU: the premises of tests/mim_cases.py -- the inputs, references and dispatch mirrors that tests/test_mim_edges_gpu.py judges csrc/mim.hip by.  No GPU,
no mvlt_amd import."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mim_cases as mc

BF, F32, F16 = mc.BF, mc.F32, mc.F16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32_sum_in_order(v, order):
    acc = np.zeros(v.shape[1], dtype=np.float32)
    for r in order:
        acc = (acc + v[r]).astype(np.float32)
    return acc


@pytest.mark.parametrize("builder,M", [("integer", 4096), ("integer", 257), ("offset16", 4096), ("constant", 300)])
def test_sums_are_exact_in_any_order(builder, M):
    """every partial sum of z and z^2 is an integer below 2^24 (constant columns: the three representable ones), so fp32 sums are exact in any order"""
    z = {"integer": lambda: mc.bn_integer_columns(M, 8), "offset16": lambda: mc.bn_offset_columns(M, 8, 16.0),
         "constant": lambda: mc.bn_constant_columns(M, 8)}[builder]()
    if builder == "constant":
        assert [float(z[:, k].unique()) for k in range(5)] == [0.0, 3.0, -4.0, float(np.float32(0.1)), 4097.0]
        # 4097: the kernel squares in fp32, fl(4097^2) = 2^13 x 2049 = 4097^2 - 1; every multiple of it and of 4097 up to 4096 of them is representable
        sq = float(np.float32(4097.0) * np.float32(4097.0))
        assert sq == 4097.0 ** 2 - 1 == 2 ** 13 * 2049 and sq - 4097.0 ** 2 < -mc.EPS
        assert all(float(np.float32(sq * k)) == sq * k and float(np.float32(4097.0 * k)) == 4097.0 * k for k in range(1, 4097))
        z = z[:, [0, 1, 2, 5, 6]]
    assert torch.equal(z, z.round()) and float((z.double() ** 2).sum(0).max()) < 2 ** 24
    zn = z.numpy()
    ref1, ref2 = z.double().sum(0).numpy(), (z.double() ** 2).sum(0).numpy()
    for order in (range(M), reversed(range(M)), np.random.default_rng(0).permutation(M)):
        order = list(order)
        assert np.array_equal(f32_sum_in_order(zn, order).astype(np.float64), ref1)
        assert np.array_equal(f32_sum_in_order(zn * zn, order).astype(np.float64), ref2)


def test_one_pass_variance_inside_its_contract():
    """the CORRECT one-pass finalize (s1 / M, s2 / M - m m, rsqrt) in float32 on exact sums: inside the 1e-3 rstd bar at offset 16 (mean^2 / var ~ 2e3),
    and how far it is at offset 255 (~ 5e5; recorded in docs/mim_edges.md, asserted nowhere)"""
    for offset, inside in ((16.0, True), (255.0, None)):
        z = mc.bn_offset_columns(4096, 64, offset)
        ref = mc.bn_stats_ref(z)
        m, var, rstd = mc.onepass_f32(z)
        rel = ((rstd.double() - ref.rstd) / ref.rstd).abs().max().item()
        ratio = (ref.mean ** 2 / ref.var).mean().item()
        print(f"offset {offset}: mean^2 / var {ratio:.3g}, one-pass fp32 rstd error {rel:.3g} relative ({rel / mc.TOL[F32]:.3g} bars)")
        assert torch.equal(m.double(), ref.mean.float().double())
        if inside:
            assert 1e3 < ratio < 4e3 and rel < mc.TOL[F32]
    # constant columns: var is 0 (or a rounding off zero, clamped) and rstd is 1 / sqrt(eps) within the bar
    m, var, rstd = mc.onepass_f32(mc.bn_constant_columns(300, 8))
    assert bool((var[:5] >= 0).all()) and ((rstd[:5].double() * math.sqrt(mc.f32(mc.EPS)) - 1).abs().max() < mc.TOL[F32])


def test_running_statistics_rule_is_batchnorm2d():
    M, C = 37, 5
    z = mc.bn_scaled_columns(M, C).double()
    bn = torch.nn.BatchNorm2d(C, eps=mc.f32(mc.EPS), momentum=mc.f32(mc.MOMENTUM)).double().train()
    rm0, rv0 = torch.linspace(-1, 1, C).double(), torch.linspace(0.5, 2, C).double()
    bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
    y = bn(z.t().reshape(1, C, M, 1))
    ref = mc.bn_stats_ref(z)
    rm, rv = mc.bn_running_ref(rm0, rv0, ref.mean, ref.var, M)
    assert torch.allclose(rm, bn.running_mean, rtol=1e-7, atol=0) and torch.allclose(rv, bn.running_var, rtol=1e-7, atol=0)
    want = mc.bn_norm_ref(z, ref.mean, ref.rstd, bn.weight.detach(), bn.bias.detach())
    assert torch.allclose(want, y.detach().reshape(C, M).t(), rtol=1e-9, atol=1e-9)
    # backward against autograd of the defining formula
    zr = z.clone().requires_grad_(True)
    g = torch.linspace(0.5, 1.5, C).double()
    dy = torch.randn(M, C, generator=mc.gen(1)).double()
    (((zr - zr.mean(0)) * (zr.var(0, unbiased=False) + mc.f32(mc.EPS)).rsqrt() * g) * dy).sum().backward()
    s = mc.bn_bwd_sums_ref(dy, z, ref.mean, ref.rstd)
    assert torch.allclose(mc.bn_dz_ref(dy, z, ref.mean, ref.rstd, g, s.s1, s.s2), zr.grad, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("n,s", [(1, 1), (1, 2), (1, 8), (2, 2), (3, 2), (5, 3), (8, 2), (8, 8), (32, 8), (72, 4)])
def test_resize_matrix(n, s):
    """rows of U sum to 1, at most two taps each, the window holds every tap; U matches F.interpolate(align_corners=True) in float64; U^T is its adjoint"""
    U, win = mc.resize_matrix(n, s)
    assert torch.allclose(U.sum(1), torch.ones(n * s, dtype=torch.float64), rtol=0, atol=1e-15)
    assert int((U != 0).sum(1).max()) <= 2 and bool(win[U != 0].all())
    x = torch.randn(1, 1, n, 1, dtype=torch.float64, generator=mc.gen(n))
    want = F.interpolate(x, size=(n * s, 1), mode="bilinear", align_corners=True).reshape(-1)
    assert torch.allclose(U @ x.reshape(-1), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("H,W,s", [(1, 1, 2), (1, 4, 8), (2, 3, 2), (3, 5, 3), (7, 8, 2), (5, 1, 8), (4, 4, 1)])
def test_resize_references(H, W, s):
    B, C = 2, 3
    x = mc.resize_random(B, H, W, C).double()
    r = mc.resize_ref(x, H, W, s)
    want = F.interpolate(x.permute(0, 3, 1, 2), size=(H * s, W * s), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert torch.allclose(r.y, want, rtol=1e-12, atol=1e-12)
    g = mc.resize_random(B, H * s, W * s, C, seed=1).double()
    a = mc.resize_adj_ref(g, H, W, s)
    assert abs(float((r.y * g).sum() - (x * a.dx).sum())) <= 1e-12 * float((r.mag * g.abs()).sum())          # <U x, g> = <x, U^T g>
    assert bool((r.mag >= r.y.abs() - 1e-15).all()) and bool((a.mag >= a.dx.abs() - 1e-15).all()) and bool((r.slack >= 0).all())
    # the ramp: the resize of an affine map is affine, last row and column included
    ramp = mc.resize_ramp(B, H, W, C)
    assert torch.allclose(mc.resize_ref(ramp, H, W, s).y, mc.resize_ramp_ref(B, H, W, C, s), rtol=1e-13, atol=1e-12)
    # deltas: forward and adjoint give the same tap set
    for iy, ix in mc.delta_points(H, W):
        foot = mc.resize_ref(mc.resize_delta(1, H, W, 1, iy, ix), H, W, s).y[0, :, :, 0]
        for oy, ox in mc.delta_points(H * s, W * s):
            taps = mc.resize_adj_ref(mc.resize_delta_out(1, H * s, W * s, 1, oy, ox), H, W, s).dx[0, :, :, 0]
            assert float(taps[iy, ix]) == float(foot[oy, ox])


def test_coordinate_slack_covers_fp32_coordinates():
    """|fl(o * fl((n - 1) / (n s - 1))) - o (n - 1) / (n s - 1)| <= coord_slack(n) for every size the GPU file uses"""
    for n, s in [(n, 2) for n in mc.SWEEP] + [(8, 8), (32, 8), (64, 4), (72, 4), (5, 3), (64, 8)]:
        no = n * s
        if no == 1:
            continue
        r = np.float32(n - 1) / np.float32(no - 1)
        o = np.arange(no)
        got = (o.astype(np.float32) * r).astype(np.float64)
        assert np.abs(got - o * (n - 1) / (no - 1)).max() <= mc.coord_slack(n)


def test_five_tap_window_covers_the_footprint_in_fp32():
    """upsample_bwd_row_s_kernel<., 2>: its window oy_lo .. oy_lo + 4, emulated in float32 for every H up to 512 -- whatever has a non-zero fp32 weight on iy and lies
    outside the window is a weight the forward gives but the adjoint drops: none above the coordinate slack (the last output row may land 1 ulp short of H - 1)"""
    for H in list(range(1, 130)) + [192, 224, 256, 384, 512]:
        for iy, lo, rows, miss in mc.window_s_f32(H, 2):
            assert miss <= mc.coord_slack(H), (H, iy, lo, rows, miss)
            assert len(rows) >= 1


def test_boundary_targets_hit_their_branch_points():
    H, W, s = 3, 2, 2
    x = mc.resize_random(2, H, W, 3) * 1.5
    target, dealt = mc.l1_boundary_target(x, H, W, s)
    assert sorted(set(dealt.abs().reshape(-1).tolist())) == sorted(mc.L1_DIFFS) and bool((dealt < 0).any()) and bool((dealt > 0).any())
    ref = mc.l1_ref(x, target, H, W, s)
    assert float((ref.d - dealt).abs().max()) <= 2.0 ** -24 * 1.1e4                    # the target is rounded to fp32: |d| is the dealt value to half an ulp of it
    a = dealt.abs()
    assert bool((a < 1).any()) and bool((a == 1).any()) and bool((a > 1).any()) and float(a.max()) == 1e4
    # both branches agree at the branch point, and the gradient is the clamp
    assert 0.5 * 1.0 * 1.0 == 1.0 - 0.5
    g = torch.autograd.functional.jacobian(lambda d: F.smooth_l1_loss(d, torch.zeros_like(d), reduction="sum"), ref.d.reshape(-1)[:50])
    assert torch.allclose(g, ref.d.reshape(-1)[:50].clamp(-1, 1))
    xt = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    loss = F.smooth_l1_loss(F.interpolate(xt, scale_factor=s, mode="bilinear", align_corners=True), target.double(), reduction="sum")
    loss.backward()
    assert math.isclose(float(loss.detach()), float(ref.loss_sum), rel_tol=1e-12)
    assert torch.allclose(xt.grad.permute(0, 2, 3, 1) / ref.d.numel(), ref.dx, rtol=1e-10, atol=1e-15)


def test_products_survive_the_narrow_types():
    for n in (2, 3):                     # ew_mul: n factors and the integer `out` it accumulates onto
        fac = mc.product_integers(50, 12, n + 1)
        p = math.prod(fac[:n]) + fac[n]
        assert all(torch.equal(f, f.to(dt).float()) and bool((f != 0).all()) for f in fac for dt in (BF, F16))
        assert torch.equal(p, p.round()) and float(p.abs().max()) <= 4 ** n + 4 and torch.equal(p, p.to(BF).float()) and torch.equal(p, p.to(F16).float())
    g, a, b, c = mc.product_integers(50, 12, 4)         # ew_mul3_bwd: dy times two of the factors
    for p in (g * b * c, g * a * c, g * a * b):
        assert float(p.abs().max()) <= 64 and torch.equal(p, p.to(BF).float())


# ------------------------------------------------------------------------------------------------ every shape reaches the branch claimed for it
def test_statistics_shapes_reach_their_branches():
    for C in mc.STATS_WIDTHS:
        assert mc.stats_kernel(C, C + 8) == ("col_reduce4_kernel", (0, 1024, F32, F32))
        cq = C // 4
        assert (64 % cq != 0) == (C in (100, 192))
        rpp = 1024 // cq
        counts = mc.stats_row_counts(C)
        step = 4 * rpp
        assert {1, 3, step - 1, step + 1, 4096} <= set(counts) and max(rpp - 1, 1) in counts
        assert mc.reduce_rows_per_wg(step + 1, C, 1024) == step and mc.reduce_rows_per_wg(step - 1, C, 1024) == step       # the seam is where the counts say
        assert mc.reduce_rows_per_wg(4096, C, 1024) == step * max(1, -(-16 // step))
    for C, ld, base in mc.STATS_SCALAR:
        assert mc.stats_kernel(C, ld, 4 * base) == ("col_reduce_kernel", (0,))
    assert mc.bwd_reduce_kernel(260, 264, 264, F32, F32) is None and mc.bwd_reduce_kernel(6, 6, 6, BF, F32) is None
    for C, nt in mc.RED8:
        for dy in (BF, F32):
            assert mc.bwd_reduce_kernel(C, 2 * C + 8, C + 8, dy, F16, dy_off=C * (2 if dy is BF else 4)) == ("col_reduce8_kernel", (nt, dy), nt)
        rpp, rows, wgs = mc.red8_rows(mc.red8_rows(1, C, nt)[1] + 1, C, nt)
        assert wgs == 2 and rows % (4 * rpp) == 0
    for C, nt in ((32, 512), (100, 1024)):
        for dy in (BF, F32):
            for z in (F16, F32):
                assert mc.bwd_reduce_kernel(C, 2 * C + 8, C + 8, dy, z, dy_off=C * (2 if dy is BF else 4)) == ("col_reduce4_kernel", (1, nt, dy, z), nt)
    assert mc.bwd_reduce_kernel(6, 13, 7, F32, F32, dy_off=24) == ("col_reduce_kernel", (1,), 256)


def test_resize_and_l1_shapes_reach_their_branches():
    assert mc.upsample_fwd_kernel(1, 4, 32, 3, 8, 8, 0, F32, True)[0] == "upsample_fwd_nchw4_kernel"
    assert mc.upsample_fwd_kernel(1, 3, 2, 3, 2, 8, 0, F32, True)[0] == "upsample_fwd_nchw4_kernel"
    assert mc.upsample_fwd_kernel(1, 3, 5, 3, 3, 8, 0, F32, True)[0] == "upsample_fwd_nchw_kernel"
    assert mc.upsample_fwd_kernel(1, 2, 72, 3, 4, 8, 0, F32, True)[0] == "upsample_fwd_nchw_kernel" and 72 * 4 > mc.NT
    assert mc.upsample_bwd_kernel(1, 2, 72, 3, 4, 0, 8, F32, BF, True) == ("upsample_bwd_nchw_kernel", (BF,))
    assert mc.upsample_bwd_kernel(1, 4, 32, 3, 8, 0, 8, F32, F32, True) == ("upsample_bwd_nchw4_kernel", (F32,))
    assert mc.upsample_bwd_kernel(1, 3, 5, 4, 2, 12, 12, F32, BF, False) is None and mc.upsample_bwd_kernel(1, 3, 5, 3, 2, 5, 5, BF, F32, False) is None
    assert mc.upsample_bwd_kernel(1, 3, 5, 4, 3, 12, 12, BF, F32, False) == ("upsample_bwd_row_kernel", (BF,))
    assert mc.upsample_bwd_kernel(1, 3, 5, 3, 2, 5, 5, F32, F32, False) == ("upsample_bwd_kernel", ())
    assert mc.l1_fwd_trips(11, 3, 64, 8) == (16896, 2) and mc.l1_fwd_trips(2, 3, 4, 8)[1] == 1 and mc.l1_fwd_trips(1, 3, 3, 2)[0] % 8 == 2
    assert mc.l1_ok(64, 4) and mc.l1_ok(1, 8) and not mc.l1_ok(72, 4) and not mc.l1_ok(5, 3)


def test_dispatch_mirrors_name_every_instantiation_of_the_source():
    """every MVLT_LAUNCH of csrc/mim.hip names a kernel the mirrors of mim_cases.py (or the GPU file, by literal) know"""
    src = open(os.path.join(ROOT, "mvlt_amd", "csrc", "mim.hip")).read()
    launched = set(re.findall(r"MVLT_LAUNCH\(\(?(\w+_kernel)", src))
    known = {"col_reduce_kernel", "col_reduce4_kernel", "col_reduce8_kernel", "bn_finalize_kernel", "bn_norm_kernel", "bn_norm8_kernel", "bn_fin_norm8_kernel",
             "bn_bwd_apply_kernel", "bn_bwd_apply8_kernel", "ew_mul_kernel", "ew_mul3_bwd_kernel", "upsample_fwd_kernel", "upsample_fwd_row_kernel",
             "upsample_fwd_nchw_kernel", "upsample_fwd_nchw4_kernel", "upsample_bwd_kernel", "upsample_bwd_row_kernel", "upsample_bwd_row_s_kernel",
             "upsample_bwd_nchw_kernel", "upsample_bwd_nchw4_kernel", "upsample_l1_fwd_kernel", "upsample_l1_bwd_kernel"}
    assert launched == known, launched ^ known
    gpu = open(os.path.join(ROOT, "tests", "test_mim_edges_gpu.py")).read() + open(os.path.join(ROOT, "tests", "mim_cases.py")).read()
    for k in known:
        assert f'"{k}"' in gpu, k

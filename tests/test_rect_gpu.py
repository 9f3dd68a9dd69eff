"""GPU: rectangular (B, 3, H, W) inputs, H != W, each side a multiple of 32 -- the reference's own rule.

Kernel level: every kernel that takes a spatial shape, at tall and wide grids (8 x 6, 6 x 8, 12 x 4 and their x2 / x4 / x8 parents, plus
the widths the LDS-halo convolutions are specialised for), against fp32 torch on the same data, with the tolerances of the square
tests in tests/test_kernels_gpu.py and tests/test_batchprep_gpu.py.
Model level (the pattern of tests/test_highres_gpu.py: oracle run live on filler weights): pvlt_tiny with every head, batch 2, both compute
dtypes, at 256 x 192 / T = 128 (tall, LDS-resident attention), 192 x 320 / T = 128 (wide) and 512 x 384 / T = 160 (M = 352: streamed
attention); the model pinned to the reference's own numbers at 256 x 192 (tests/golden/rect_tiny256x192.npz); the refusals; the engine
loop, the prefetcher with on-device batch preparation and evaluate_vl on rectangular batches.
Bounds (north_star, as in test_highres_gpu.py): eval outputs 1e-3 max-abs / max-abs (fp32) and 2e-2 relative L2 (bf16; the ITM logits
through their class probabilities); gradients of one train step 2e-4 (fp32) / 8e-2 (bf16)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import batchprep_oracle as BP
from oracle import pvlt_oracle as O
from oracle.hostinfo import usable_cores
from tests.golden.make_golden_rect import NAME, rect_batch

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
TOL = {F32: 1e-3, BF: 2e-2}
GTOL = {F32: 2e-4, BF: 8e-2}
LT = dict(mlm=1, itm=1, t2i=1, cls=1)
CASES = {"256x192_T128": (256, 192, 128), "192x320_T128": (192, 320, 128), "512x384_T160": (512, 384, 160)}
B, SEED, DP = 2, 23, 0.1
_ORACLE = {}
GRIDS = [(8, 6), (6, 8), (12, 4)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def maxrel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rnd(*shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dev()).to(dtype)


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as _ops
    return _ops


# =============================================================================================== kernel level
@pytest.mark.parametrize("gin,hout,wout,C,skip", [(7, 8, 6, 512, 1), (14, 12, 16, 320, 0), (28, 12, 4, 128, 0), (56, 64, 48, 64, 0), (56, 48, 80, 64, 0),
                                                  (56, 392, 8, 64, 0), (7, 2, 98, 512, 1)])
def test_pos_embed_resize_to_a_rectangle(ops, gin, hout, wout, C, skip):
    """mvlt_resize_bilinear_tokens and _multi, forward and adjoint, square source grid -> hout x wout, against F.interpolate(mode='bilinear')
    and its autograd (tolerances of test_pos_embed_resize_matches_interpolate)"""
    param = rnd(1, gin * gin + skip, C, dtype=F32)
    pe = param[:, skip:][0]
    pr = param.clone().requires_grad_(True)
    t = pr[:, skip:].reshape(1, gin, gin, C).permute(0, 3, 1, 2)
    ref = F.interpolate(t, size=(hout, wout), mode="bilinear").reshape(1, C, hout * wout).permute(0, 2, 1)[0]
    dy = rnd(hout * wout, C, dtype=F32, seed=7)
    ref.backward(dy)
    out = torch.empty(hout * wout, C, device=dev())
    ops.resize_bilinear_tokens(pe, out, gin, gin, hout, wout, C)
    assert (out - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()
    g = torch.zeros_like(param)
    g[:, :skip] = 3.0
    ops.resize_bilinear_tokens(dy, g[:, skip:][0], gin, gin, hout, wout, C, adjoint=True)
    assert maxrel(g[:, skip:], pr.grad[:, skip:]) < 1e-5
    assert skip == 0 or float(g[0, 0, 0]) == 3.0
    # the batched launch: this job beside a second one of another shape (transposed target)
    pe2 = rnd(gin * gin, 64, dtype=F32, seed=9)
    ref2 = F.interpolate(pe2.reshape(1, gin, gin, 64).permute(0, 3, 1, 2), size=(wout, hout), mode="bilinear").reshape(64, wout * hout).t()
    o1, o2 = torch.empty_like(out), torch.empty(wout * hout, 64, device=dev())
    ops.resize_bilinear_tokens_multi([(pe, o1, gin, gin, hout, wout, C), (pe2, o2, gin, gin, wout, hout, 64)])
    assert torch.equal(o1, out)
    assert (o2 - ref2).abs().max().item() <= 2e-6 * ref2.abs().max().item()
    g1, g2 = torch.zeros(gin * gin, C, device=dev()), torch.zeros(gin * gin, 64, device=dev())
    dy2 = rnd(wout * hout, 64, dtype=F32, seed=11)
    ops.resize_bilinear_tokens_multi([(dy, g1, gin, gin, hout, wout, C), (dy2, g2, gin, gin, wout, hout, 64)], adjoint=True)
    assert maxrel(g1, pr.grad[0, skip:]) < 1e-5
    p2 = pe2.clone().requires_grad_(True)
    F.interpolate(p2.reshape(1, gin, gin, 64).permute(0, 3, 1, 2), size=(wout, hout), mode="bilinear").reshape(64, wout * hout).t().backward(dy2)
    assert maxrel(g2, p2.grad) < 1e-5


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("H,W", [(32, 24), (24, 32), (48, 16), (256, 192), (192, 320), (64, 1360), (32, 1368)])      # the last two: at and past the strip kernel's LDS gate
def test_patchify_rectangles(ops, dtype, H, W):
    Bsz, k = 2, 4
    img = torch.rand(Bsz, 3, H, W, device=dev())
    P = torch.full((Bsz * (H // k) * (W // k) + 1, 3 * k * k), 7.0, device=dev(), dtype=dtype)
    ops.patchify(img, P[:-1], Bsz, 3, H, W, k)
    ref = F.unfold(img, kernel_size=k, stride=k).transpose(1, 2).reshape(-1, 3 * k * k)          # rows (b, oi, oj), columns (c, di, dj)
    if dtype == F32:
        assert torch.equal(P[:-1], ref)
    else:
        assert maxrel(P[:-1].float(), ref) < TOL[dtype]
    assert (P[-1] == 7.0).all()


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("r", [2, 4, 8])
@pytest.mark.parametrize("ho,wo", GRIDS)
def test_patch_gather_gemm_rectangles(ops, dtype, r, ho, wo):
    """kernel == stride conv through the patch row map (forward), its scatter adjoint and its weight gradient, on an (r ho) x (r wo) grid with text rows
    behind the image rows, against F.conv2d (tolerances of test_gemm_nt_patch_gather_and_scatter / test_gemm_tn_conv_weight_layout)"""
    from mvlt_amd._lib import patchmap
    Bsz, T, Cin, Cout = 2, 5, 64, 128
    Hin, Win = r * ho, r * wo
    HWi, K, M = Hin * Win, r * r * Cin, Bsz * ho * wo
    X = rnd(Bsz, HWi + T, Cin, dtype=dtype)
    Wc = rnd(Cout, Cin, r, r, dtype=dtype, seed=1, scale=0.1)
    bias = rnd(Cout, dtype=F32, seed=2)
    Wk = Wc.permute(0, 2, 3, 1).reshape(Cout, K).contiguous()
    pm = patchmap(r, Win, HWi + T, ho * wo, wo, Cin)
    out = torch.empty(M, Cout, device=dev(), dtype=dtype)
    ops.gemm_nt(X, Wk, out, M, Cout, K, Cin, K, Cout, a_map=pm, bias=bias)
    img = X[:, :HWi].float().transpose(1, 2).reshape(Bsz, Cin, Hin, Win)
    ref = F.conv2d(img, Wc.float(), bias, stride=r).flatten(2).transpose(1, 2).reshape(M, Cout)
    assert maxrel(out.float(), ref) < TOL[dtype]
    dY = rnd(M, Cout, dtype=dtype, seed=3)
    dX = torch.zeros(Bsz, HWi + T, Cin, device=dev(), dtype=dtype)
    ops.gemm_nt(dY, Wk.t().contiguous(), dX, M, K, Cout, Cout, Cout, Cin, c_map=pm)
    imgr = img.clone().requires_grad_(True)
    Wg, bg = Wc.float().clone().requires_grad_(True), torch.zeros(Cout, device=dev(), requires_grad=True)
    y = F.conv2d(imgr, Wg, bg, stride=r).flatten(2).transpose(1, 2).reshape(M, Cout)
    (y * dY.float()).sum().backward()
    assert maxrel(dX[:, :HWi].float(), imgr.grad.reshape(Bsz, Cin, HWi).transpose(1, 2)) < TOL[dtype]
    assert dX[:, HWi:].abs().max().item() == 0.0
    dW = torch.zeros(Cout, Cin, r, r, device=dev(), dtype=F32)
    cs = torch.zeros(Cout, device=dev(), dtype=F32)
    ops.gemm_tn(dY, X, dW.view(Cout, K), M, Cout, K, Cout, Cin, K, b_map=pm, colsum=cs, taps=r * r, seg=Cin)
    assert maxrel(dW, Wg.grad) < TOL[dtype]
    assert maxrel(cs, bg.grad) < TOL[dtype]


# generic gathers (8 x 6, 6 x 8, 12 x 4, 32 x 24, 24 x 40) and the LDS-halo kernels' widths (16 / 32 / 64; 8 for the weight gradient) at heights != width
@pytest.mark.parametrize("h,w,Cin,Cout,Bsz,tokens_extra", [(8, 6, 64, 64, 2, 0), (6, 8, 64, 128, 3, 5), (12, 4, 128, 64, 2, 128), (32, 24, 64, 64, 2, 0), (24, 40, 64, 64, 1, 0),
                                                           (24, 32, 192, 192, 2, 0), (12, 32, 64, 64, 3, 128), (4, 32, 128, 64, 2, 0), (8, 16, 64, 64, 3, 0),
                                                           (48, 16, 128, 128, 2, 128), (6, 64, 64, 64, 2, 0), (16, 64, 64, 192, 1, 0), (24, 8, 64, 64, 3, 0),
                                                           (64, 32, 64, 64, 1, 0), (40, 16, 64, 128, 1, 0)])
def test_conv3x3_gemms_rectangles(ops, h, w, Cin, Cout, Bsz, tokens_extra):
    """conv3map GEMM forward (plain, column-statistics and accumulate epilogues), input gradient (the same gather with flipped taps) and weight
    gradient on an h x w grid against F.conv2d(padding=1) (tolerances of test_conv3x3_nt_lds_halo / test_conv3x3_wgrad_lds_halo)"""
    from mvlt_amd._lib import conv3map
    tokens_in = h * w + tokens_extra
    X = rnd(Bsz, tokens_in, Cin, dtype=BF)
    Wk = rnd(Cout, 9 * Cin, dtype=BF, scale=0.05, seed=3)                     # [out][tap][cin]
    M = Bsz * h * w
    amap = conv3map(h, w, tokens_in, Cin)
    img = X[:, : h * w].float().reshape(Bsz, h, w, Cin).permute(0, 3, 1, 2)
    Wc = Wk.float().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
    ref = F.conv2d(img, Wc, None, padding=1).permute(0, 2, 3, 1).reshape(M, Cout)
    out = torch.empty(M, Cout, device=dev(), dtype=F32)
    ops.gemm_nt(X, Wk, out, M, Cout, 9 * Cin, Cin, 9 * Cin, Cout, a_map=amap)
    assert maxrel(out, ref) < TOL[BF]
    st = torch.zeros(2, 4, Cout, device=dev())
    out2 = torch.empty_like(out)
    ops.gemm_nt(X, Wk, out2, M, Cout, 9 * Cin, Cin, 9 * Cin, Cout, a_map=amap, col_sum=st[0], col_sumsq=st[1], col_copies=4)
    assert maxrel(out2, ref) < TOL[BF]
    assert maxrel(st[0].sum(0), out2.sum(0)) < 1e-4 and maxrel(st[1].sum(0), (out2 * out2).sum(0)) < 1e-4
    base = rnd(M, Cout, dtype=F32, seed=5)
    acc = base.clone()
    ops.gemm_nt(X, Wk, acc, M, Cout, 9 * Cin, Cin, 9 * Cin, Cout, a_map=amap, R=acc)
    assert maxrel(acc, ref + base) < TOL[BF]
    # input gradient: gather dz over the same grid with flipped, transposed taps (mim.py bn_conv_bwd)
    dz = rnd(M, Cout, dtype=BF, seed=2)
    Wf = Wc.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).to(BF).contiguous()      # [cin][flipped tap][out]
    dx = torch.empty(M, Cin, device=dev(), dtype=F32)
    ops.gemm_nt(dz, Wf, dx, M, Cin, 9 * Cout, Cout, 9 * Cout, Cin, a_map=conv3map(h, w, h * w, Cout))
    imgr = img.clone().requires_grad_(True)
    Wg = torch.zeros(Cout, Cin, 3, 3, device=dev(), requires_grad=True)
    y = F.conv2d(imgr, Wc, None, padding=1) + F.conv2d(img, Wg, None, padding=1)
    (y.permute(0, 2, 3, 1).reshape(M, Cout) * dz.float()).sum().backward()
    assert maxrel(dx, imgr.grad.permute(0, 2, 3, 1).reshape(M, Cin)) < TOL[BF]
    # weight gradient
    dW = torch.zeros(Cout, 9 * Cin, device=dev(), dtype=F32)
    ops.gemm_tn(dz, X, dW, M, Cout, 9 * Cin, Cout, Cin, 9 * Cin, b_map=amap)
    refw = Wg.grad.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    assert maxrel(dW, refw) < TOL[BF]
    assert ((dW.double() - refw.double()).norm() / refw.double().norm()).item() < 5e-3


@pytest.mark.parametrize("Bsz,H,W,C,s,nchw,out_dtype", [(2, 8, 6, 64, 2, False, F32), (3, 6, 8, 192, 2, False, BF), (2, 12, 4, 128, 2, False, BF), (2, 16, 12, 64, 2, False, F32),
                                                        (2, 8, 6, 3, 8, True, F32), (2, 6, 8, 3, 8, True, F32), (1, 12, 4, 3, 8, True, F32), (2, 32, 24, 3, 8, True, F32),
                                                        (2, 24, 40, 3, 8, True, F32), (1, 64, 48, 3, 8, True, F32), (1, 196, 4, 3, 8, True, F32), (1, 5, 7, 6, 3, False, F32),
                                                        (1, 7, 5, 3, 3, True, F32)])
def test_upsample_fwd_bwd_rectangles(ops, Bsz, H, W, C, s, nchw, out_dtype):
    """mvlt_upsample_fwd / _bwd at x2 (pixel-major) and x8 (NCHW), H != W, against F.interpolate(align_corners=True) and its autograd
    (tolerances of test_upsample_fwd_bwd)"""
    x = rnd(Bsz * H * W, C, dtype=F32)
    xt = x.view(Bsz, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = F.interpolate(xt, scale_factor=s, mode="bilinear", align_corners=True)
    Ho, Wo = H * s, W * s
    if nchw:
        got = torch.empty(Bsz, C, Ho, Wo, device=dev(), dtype=F32)
        ops.upsample_fwd(x, C, Bsz, H, W, C, s, got, 0, nchw=True)
    else:
        out = torch.empty(Bsz * Ho * Wo, C, device=dev(), dtype=out_dtype)
        ops.upsample_fwd(x, C, Bsz, H, W, C, s, out, C)
        got = out.float().view(Bsz, Ho, Wo, C).permute(0, 3, 1, 2)
    assert maxrel(got, ref.detach()) < (1e-5 if out_dtype == F32 else TOL[BF])
    g = rnd(Bsz, C, Ho, Wo, dtype=F32, seed=3)
    ref.backward(g)
    dy = g.contiguous() if nchw else g.permute(0, 2, 3, 1).reshape(Bsz * Ho * Wo, C).contiguous()
    base = rnd(Bsz * H * W, C, dtype=F32, seed=5)
    dx = base.clone()
    ops.upsample_bwd(dy, 0 if nchw else C, nchw, Bsz, H, W, C, s, dx, C, accumulate=True)
    want = base + xt.grad.permute(0, 2, 3, 1).reshape(Bsz * H * W, C)
    assert maxrel(dx, want) < 1e-5
    if not nchw and C % 4 == 0:
        dyh = dy.to(BF)
        dxa, dxb = torch.zeros(Bsz * H * W, C, device=dev()), torch.zeros(Bsz * H * W, C, device=dev())
        ops.upsample_bwd(dyh, C, False, Bsz, H, W, C, s, dxa, C)
        ops.upsample_bwd(dyh.float(), C, False, Bsz, H, W, C, s, dxb, C)
        assert torch.equal(dxa, dxb)
    if nchw:
        dx16 = torch.zeros(Bsz * H * W, 8, device=dev(), dtype=BF)
        ops.upsample_bwd(dy, 0, True, Bsz, H, W, C, s, dx16, 8)
        assert maxrel(dx16[:, :C].float(), want - base) < TOL[BF]
        assert (dx16[:, C:] == 0).all()


@pytest.mark.parametrize("Bsz,H,W,out_dtype", [(2, 32, 24, BF), (2, 24, 32, F32), (3, 8, 6, F32), (1, 12, 4, F32), (1, 196, 4, BF), (2, 64, 32, F32)])
def test_upsample_smooth_l1_fused_rectangles(ops, Bsz, H, W, out_dtype):
    """the fused x8 upsample + SmoothL1 against a (B, 3, 8H, 8W) target (tolerances of test_upsample_smooth_l1_fused)"""
    C, s = 3, 8
    assert ops.upsample_l1_ok(W, s)
    x = rnd(Bsz * H * W, C, dtype=F32, scale=1.5)
    target = rnd(Bsz, C, H * s, W * s, dtype=F32, seed=3)
    xt = x.view(Bsz, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = F.smooth_l1_loss(F.interpolate(xt, scale_factor=s, mode="bilinear", align_corners=True), target)
    acc = torch.zeros(1, device=dev())
    ops.upsample_l1_fwd(x, C, Bsz, H, W, C, s, target, acc)
    assert abs(acc.item() / target.numel() - ref.item()) <= 1e-5 * abs(ref.item())
    (ref * 3.0).backward()
    want = xt.grad.permute(0, 2, 3, 1).reshape(Bsz * H * W, C)
    dx = torch.zeros(Bsz * H * W, 8, device=dev(), dtype=out_dtype)
    ops.upsample_l1_bwd(x, C, Bsz, H, W, C, s, target, torch.full((1,), 3.0, device=dev()), dx, 8)
    assert maxrel(dx[:, :C].float(), want) < (1e-5 if out_dtype == F32 else TOL[BF])
    assert (dx[:, C:] == 0).all()


@pytest.mark.parametrize("H,W,ratio,mode", [(256, 192, 0.5, "exact"), (256, 192, 0.5, "reference"), (192, 320, 0.75, "exact"), (192, 320, 0.5, "reference"),
                                            (1568, 32, 0.5, "exact"), (32, 1568, 0.5, "reference"), (96, 64, 0.25, "exact")])
def test_batch_prep_rectangles_bit_exact(H, W, ratio, mode):
    """grid_mask_flags / grid_mask_apply (and the token masking beside them) with gh != gw, bit-exact against oracle/batchprep_oracle.py; exactly
    int(ratio * gh * gw) masked patches per sample in "exact" mode"""
    from mvlt_amd.batchprep import DeviceBatchPrep
    Bsz, T, seed, sample0 = 3, 32, 77, 1000
    gh, gw = H // 16, W // 16
    rs = np.random.RandomState(H + W)
    image = rs.rand(Bsz, 3, H, W).astype(np.float32)
    ori = rect_batch(9, Bsz, 32, 32, T)["ori_input_ids"].numpy()
    out = DeviceBatchPrep(seed, mask_ratio=ratio, mode=mode)(torch.from_numpy(image).to(dev()), torch.from_numpy(ori).to(dev()), sample0=sample0)
    torch.cuda.synchronize()
    want = BP.prepare_batch(seed, sample0, image, ori, int(ratio * gh * gw), 0 if mode == "exact" else 1)
    assert tuple(out["patch_flags"].shape) == (Bsz, gh, gw) and tuple(out["masked_images"].shape) == (Bsz, 3, H, W)
    assert np.array_equal(out["patch_flags"].cpu().numpy(), want["patch_flags"])
    assert np.array_equal(out["masked_images"].cpu().numpy(), want["masked_images"])
    assert np.array_equal(out["input_ids"].cpu().numpy(), want["input_ids"]) and np.array_equal(out["mlm_labels"].cpu().numpy(), want["mlm_labels"])
    if mode == "exact":
        assert (out["patch_flags"].reshape(Bsz, -1).sum(1) == int(ratio * gh * gw)).all()


# =============================================================================================== model level
def setup(T, dtype, seed=SEED, dp=DP):
    from mvlt_amd import pvlt
    cfg = O.Cfg("pvlt_tiny", LT, 224, 768, T, dp)
    sd = O.filled_state_dict(cfg, seed)
    model = pvlt.pvlt_tiny(pretrained=True, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None,
                           drop_path_rate=dp, drop_rate=0.0, num_classes=1000, in_chans=3, compute_dtype=dtype)
    model.load_state_dict(sd, strict=True)
    model.cuda(dev())
    return model, cfg, sd


def out_err(k, o, v, dtype):
    o, v = o.detach().double().cpu(), v.detach().double().cpu()
    if dtype == F32:
        return ((o - v).abs().max() / v.abs().max().clamp_min(1e-30)).item()
    if k == "itm_logits":                               # B x 2 numbers near cancellation: their class probabilities (test_model_gpu.py)
        return (o.softmax(-1) - v.softmax(-1)).abs().max().item()
    return ((o - v).norm() / v.norm().clamp_min(1e-30)).item()


def oracle_eval(name, sd, cfg, batch):
    if ("eval", name) not in _ORACLE:
        taps = {}
        torch.set_num_threads(usable_cores())
        with torch.no_grad():
            _ORACLE[("eval", name)] = (O.forward(sd, cfg, batch["image"], batch["input_ids"], taps=taps), taps)
    return _ORACLE[("eval", name)]


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("name", list(CASES))
def test_eval_forward_matches_oracle(parity, name, dtype):
    H, W, T = CASES[name]
    model, cfg, sd = setup(T, dtype)
    batch = rect_batch(SEED, B, H, W, T)
    model.eval()
    with torch.no_grad():
        out = model(batch["image"].to(dev()), batch["input_ids"].to(dev()))
    torch.cuda.synchronize()
    ref, _ = oracle_eval(name, sd, cfg, batch)
    bad = {}
    for k, v in ref.items():
        assert v is not None and out[k] is not None, k
        assert tuple(out[k].shape) == tuple(v.shape), (k, out[k].shape, v.shape)
        assert torch.isfinite(out[k].float()).all(), k
        e = out_err(k, out[k], v, dtype)
        if not parity(f"out/{k}", e, TOL[dtype]):
            bad[k] = e
    assert tuple(out["t2i_logits"].shape) == (B, 3, H, W)
    assert len(ref) == 5 and not bad, (name, str(dtype), bad)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("name", list(CASES))
def test_pyramid_features_match_oracle(parity, name, dtype):
    """forward_pyramid_features_vl: (B, C_i, H / (4 * 2^i), W / (4 * 2^i)) maps and (B, T, C_i) text features against the oracle's stage outputs"""
    H, W, T = CASES[name]
    model, cfg, sd = setup(T, dtype)
    batch = rect_batch(SEED, B, H, W, T)
    model.eval()
    with torch.no_grad():
        img_feats, text_feats = model.forward_pyramid_features_vl(batch["image"].to(dev()), batch["input_ids"].to(dev()))
    torch.cuda.synchronize()
    _, taps = oracle_eval(name, sd, cfg, batch)
    bad = {}
    for i in range(4):
        assert tuple(img_feats[i].shape) == (B, model.dims[i], H // (4 * 2 ** i), W // (4 * 2 ** i)), img_feats[i].shape
        assert img_feats[i].is_contiguous() and tuple(text_feats[i].shape) == (B, T, model.dims[i])
        for k, got in ((f"img_feat{i+1}", img_feats[i]), (f"text_feat{i+1}", text_feats[i])):
            assert tuple(got.shape) == tuple(taps[k].shape), k
            e = out_err(k, got.float(), taps[k], dtype)
            if not parity("tap/" + k, e, TOL[dtype]):
                bad[k] = e
    assert not bad, (name, str(dtype), bad)


def _check_grads(parity, model, grads, out, batch, dtype, what):
    # the ITM head's bias gradients are batch sums of signed per-pair residuals that cancel: on the bf16 path they are gated against the
    # un-cancelled scale, as test_model_gpu.py::test_train_step_parity and test_highres_gpu.py do -- no other exemption
    cancel = {}
    if dtype == BF:
        pr = out["itm_logits"].detach().float().reshape(B, 2).softmax(-1).cpu().numpy().astype(np.float64)
        a_b = pr[:, 0] - (batch["itm_labels"].reshape(-1).numpy() == 0)
        c_itm = max(1.0, float(np.sqrt((a_b ** 2).sum()) / max(1e-12, abs(a_b.sum()))))
        cancel = {"itm_head.linear.bias": c_itm, "itm_head.linear_bias": c_itm, "itm_head_embed.1.bias": c_itm}
    gtol = GTOL[dtype]
    bad, n = {}, 0
    for k, p in model.named_parameters():
        ref = grads.get(k)
        if ref is None or ref.double().norm().item() < 1e-7:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        n += 1
        c_k = cancel.get(k, 1.0)
        refn = ref.double().norm().item()
        en = abs(p.grad.double().norm().item() - refn) / (refn * c_k)
        ef = ((p.grad.detach().double().cpu() - ref.double()).norm() / ref.double().norm()).item() / c_k
        if not (parity("grad-norm/" + k, en, gtol) & parity("grad-full/" + k, ef, gtol)):
            bad[k] = (en, ef)
    assert n > 50
    assert not bad, (what, str(dtype), len(bad), sorted(bad.items(), key=lambda kv: -kv[1][1])[:10])


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("name", list(CASES))
def test_train_step_matches_oracle(parity, name, dtype):
    """one train-mode step on the grid-masked image with injected dropout / DropPath masks, through the engine's fused masked-row MLM path:
    losses and every parameter gradient against the oracle's autograd"""
    from mvlt_amd.engine import compute_losses
    from tests.golden.make_golden import make_masks
    H, W, T = CASES[name]
    model, cfg, sd = setup(T, dtype)
    batch = rect_batch(SEED, B, H, W, T)
    step_idx = 1
    masks = make_masks(cfg, B, T, SEED + step_idx)
    model.train()
    model.injected_masks = masks
    db = {k: v.to(dev()) for k, v in batch.items()}
    out = model(db["masked_images"], db["input_ids"], mlm_labels=db["mlm_labels"])
    assert "mlm_loss" in out
    total, parts = compute_losses(out, db["image"], db["mlm_labels"], db["itm_labels"], db["sup_cls_labels"], db["sub_cls_labels"])
    total.backward()
    torch.cuda.synchronize()
    if ("train", name) not in _ORACLE:
        sdg = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running_" not in k) else v) for k, v in sd.items() if k != O.TIED[0]}
        sdg[O.TIED[0]] = sdg[O.TIED[1]]
        torch.set_num_threads(usable_cores())
        lo, _ = O.step_loss(sdg, cfg, batch, step_idx, train=True, masks=masks, bn_out={})
        lo["total_loss"].backward()
        _ORACLE[("train", name)] = ({k: float(v) for k, v in lo.items()}, {k: v.grad for k, v in sdg.items() if v.is_floating_point() and v.grad is not None})
    lo, grads = _ORACLE[("train", name)]
    ls = dict(parts, total_loss=total)
    for k, ref in lo.items():
        assert parity(f"loss/{k}", abs(float(ls[k]) - ref) / max(1.0, abs(ref)), TOL[dtype]), (k, float(ls[k]), ref)
    _check_grads(parity, model, grads, out, batch, dtype, name)


# ------------------------------------------------------------------ against the reference's own numbers (no hop through the oracle)
def _sample(t, n):
    f = t.detach().reshape(-1).to(torch.float32).cpu()
    stride = max(1, f.numel() // n) | 1
    return f[::stride][:n].numpy()


def _err(a, b, dtype):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    if dtype == F32:
        return np.abs(a - b).max() / max(1e-6, np.abs(b).max())
    return np.linalg.norm(a - b) / max(1e-12, np.linalg.norm(b))


def _golden(golden_dir, dtype):
    g = np.load(os.path.join(golden_dir, NAME + ".npz"))
    seed, Bg, H, W, T = (int(v) for v in g["meta"][:5])
    model, cfg, sd = setup(T, dtype, seed=seed, dp=float(g["meta"][5]))
    return g, model, cfg, rect_batch(seed, Bg, H, W, T), seed


@pytest.mark.parametrize("dtype", [F32, BF])
def test_eval_forward_matches_the_reference_fixture(golden_dir, parity, dtype):
    """the metrics of tests/test_model_gpu.py::test_eval_forward_parity on the 256 x 192 fixture"""
    g, model, cfg, batch, seed = _golden(golden_dir, dtype)
    model.eval()
    model._taps = {}
    with torch.no_grad():
        out = model(batch["image"].to(dev()), batch["input_ids"].to(dev()))
    torch.cuda.synchronize()
    tol, bad = TOL[dtype], {}
    for k in g.files:
        if k.startswith("eval/tap/") and k.endswith("/sample"):
            tap = k.split("/")[2]
            if not parity(f"tap/{tap}", _err(_sample(model._taps[tap], 1024), g[k], dtype), tol):
                bad[k] = 1
        if k.startswith("eval/out/") and k.endswith("/sample"):
            key = k.split("/")[2]
            assert tuple(out[key].shape) == tuple(g[f"eval/out/{key}/shape"]), key
            if dtype == BF and key == "itm_logits":
                continue
            if not parity(f"out/{key}", _err(_sample(out[key].float(), 4096), g[k], dtype), tol):
                bad[k] = 1
        if k.startswith("eval/full/"):
            key = k.split("/")[2]
            o = out[key].float().cpu()
            if dtype == BF and key == "itm_logits":
                e = (o.double().softmax(-1) - torch.from_numpy(g[k]).double().softmax(-1)).abs().max().item()
            else:
                e = _err(o.numpy(), g[k], dtype)
            if not parity(f"full/{key}", e, tol):
                bad[k] = e
    rows = out["mlm_logits"].reshape(-1, 30522)[torch.from_numpy(g["masked_positions"]).to(dev())].float().cpu()
    if not parity("mlm_top8", _err(rows.topk(8, dim=-1)[0].numpy(), g["eval/mlm/top8_val"], dtype), tol):
        bad["mlm_top8"] = 1
    if not parity("t2i_grid", _err(out["t2i_logits"][:, :, ::16, ::16].float().cpu().numpy(), g["eval/t2i/grid"], dtype), tol):
        bad["t2i_grid"] = 1
    assert not bad, (str(dtype), bad)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_train_step_matches_the_reference_fixture(golden_dir, parity, dtype):
    """losses, gradient norms and strided gradient samples of the reference's own train step at 256 x 192 (gates of test_train_step_parity:
    2e-4 / 8e-4 on the fp32 path, 8e-2 / 3.2e-1 on the bf16 path, the three ITM bias tensors against their un-cancelled scale)"""
    from mvlt_amd.engine import compute_losses
    from tests.golden.make_golden import make_masks
    g, model, cfg, batch, seed = _golden(golden_dir, dtype)
    step_idx = int(g["meta"][6])
    Bg, T = batch["input_ids"].shape
    model.train()
    model.injected_masks = make_masks(cfg, Bg, T, seed + step_idx)
    db = {k: v.to(dev()) for k, v in batch.items()}
    out = model(db["masked_images"], db["input_ids"], mlm_labels=db["mlm_labels"])
    total, parts = compute_losses(out, db["image"], db["mlm_labels"], db["itm_labels"], db["sup_cls_labels"], db["sub_cls_labels"])
    total.backward()
    torch.cuda.synchronize()
    ls = dict(parts, total_loss=total)
    for k in ("loss_mlm", "loss_itm", "loss_sup_cls", "loss_sub_cls", "loss_t2i", "total_loss"):
        ref = float(g[f"train{step_idx}/loss/{k}"])
        assert parity(f"loss/{k}", abs(float(ls[k]) - ref) / max(1.0, abs(ref)), TOL[dtype]), (k, float(ls[k]), ref)
    cancel = {}
    if dtype == BF:
        pr = out["itm_logits"].detach().float().reshape(Bg, 2).softmax(-1).cpu().numpy().astype(np.float64)
        a_b = pr[:, 0] - (batch["itm_labels"].reshape(-1).numpy() == 0)
        c_itm = max(1.0, float(np.sqrt((a_b ** 2).sum()) / max(1e-12, abs(a_b.sum()))))
        cancel = {"itm_head.linear.bias": c_itm, "itm_head.linear_bias": c_itm, "itm_head_embed.1.bias": c_itm}
    gtol, bad, n = GTOL[dtype], {}, 0
    for k, p in model.named_parameters():
        gk = f"train{step_idx}/grad/{k}/norm"
        if gk not in g.files or float(g[gk]) < 1e-7:
            continue
        refn, ref_s = float(g[gk]), g[f"train{step_idx}/grad/{k}/sample"]
        assert p.grad is not None, k
        n += 1
        c_k = cancel.get(k, 1.0)
        es = float(np.abs(_sample(p.grad, 32) - ref_s).max() / max(np.abs(ref_s).max(), 1e-3 * refn / max(1.0, p.numel() ** 0.5))) / c_k
        if not (parity("grad-norm/" + k, abs(p.grad.double().norm().item() - refn) / (refn * c_k), gtol) & parity("grad-sample/" + k, es, 4 * gtol)):
            bad[k] = es
    assert n > 50 and not bad, (str(dtype), len(bad), sorted(bad.items(), key=lambda kv: -kv[1])[:10])


# ------------------------------------------------------------------ refusals
def test_side_not_a_multiple_of_32_is_refused_before_any_launch():
    from mvlt_amd._lib import last_kernel
    model, cfg, sd = setup(16, F32)
    model.eval()
    ids = torch.zeros(1, 16, dtype=torch.long, device=dev())
    with torch.no_grad():
        model(torch.zeros(1, 3, 64, 32, device=dev()), ids)       # a valid rectangle first: last_kernel() then names its last launch
    torch.cuda.synchronize()
    before = last_kernel()
    for H, W in ((448, 112), (112, 448)):
        with pytest.raises(AssertionError) as e:
            with torch.no_grad():
                model(torch.zeros(1, 3, H, W, device=dev()), ids)
        assert "448" in str(e.value) and "112" in str(e.value)
    assert last_kernel() == before


@pytest.mark.parametrize("dtype", [F32, BF])
def test_896x224_is_refused_like_the_reference(dtype):
    """stage 2 has 112 x 28 = 3136 patches, stage 1's constructor count: the reference hands it the 784-row embedding unresized and fails on the shapes"""
    T = 16
    model, cfg, sd = setup(T, dtype)
    img = torch.zeros(1, 3, 896, 224)
    ids = torch.zeros(1, T, dtype=torch.long)
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            O.forward(sd, cfg, img, ids)
    model.eval()
    with pytest.raises(RuntimeError, match="unresized"):
        with torch.no_grad():
            model(img.to(dev()), ids.to(dev()))
    torch.cuda.synchronize()


def test_1568x32_uses_the_square_embedding_row_for_row(parity):
    """stage 1 has 392 x 8 = 3136 patches = 56 x 56: the reference adds the square embedding unresized, row for row; batch 1, eval, fp32"""
    H, W, T = 1568, 32, 16
    model, cfg, sd = setup(T, F32)
    batch = rect_batch(SEED, 1, H, W, T)
    model.eval()
    with torch.no_grad():
        out = model(batch["image"].to(dev()), batch["input_ids"].to(dev()))
        ref = O.forward(sd, cfg, batch["image"], batch["input_ids"])
    torch.cuda.synchronize()
    for k, v in ref.items():
        assert tuple(out[k].shape) == tuple(v.shape), k
        assert parity(f"out/{k}", out_err(k, out[k], v, F32), TOL[F32]), k


# ------------------------------------------------------------------ engine and callers
class _Loader:
    """list-of-dicts loader that also injects the iteration's dropout / DropPath draws into the model (tests/test_engine_gpu.py)"""

    def __init__(self, model, batches, masks):
        self.model, self.batches, self.masks = model, batches, masks

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for it, b in enumerate(self.batches):
            self.model.injected_masks = self.masks[it]
            yield b


@pytest.mark.parametrize("dtype", [F32, BF])
def test_engine_loop_at_256x192(parity, dtype):
    """`train_one_epoch_vl` imported the way reference main_vl.py:198 does, two iterations (clean image, then grid-masked) at 256 x 192: finite
    losses; on the fp32 path the epoch averages match the oracle's loop (as test_highres_gpu.py::test_engine_loop_at_512px)"""
    import engine_grid_masking as E
    from mvlt_amd.engine import BF16Scaler
    from mvlt_amd.optim import FusedAdamW
    from tests.golden.make_golden import make_masks
    H, W, T, iters, lr, wd = 256, 192, 128, 2, 1e-4, 0.05
    model, cfg, sd = setup(T, dtype, seed=SEED + 1)
    batches = [rect_batch(SEED + 100 * it, B, H, W, T) for it in range(iters)]
    masks = [make_masks(cfg, B, T, SEED + it) for it in range(iters)]
    opt = FusedAdamW(model, lr=lr, weight_decay=wd)
    args = types.SimpleNamespace(loss_type=cfg.loss_type)
    seen = []
    fwd = model.forward
    model.forward = lambda im, ids, **kw: (seen.append((tuple(im.shape), float(im.float().mean()))), fwd(im, ids, **kw))[1]
    res = E.train_one_epoch_vl(model, None, _Loader(model, batches, masks), opt, dev(), 0, BF16Scaler(), None, None, None, True, False, args)
    model.forward = fwd
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in res.values()), res
    for it, (shape, mean) in enumerate(seen):
        want = batches[it]["masked_images" if it % 2 == 1 else "image"].mean().item()
        assert shape == (B, 3, H, W) and abs(mean - want) < 1e-5, (it, shape, mean, want)
    if dtype != F32:
        return
    torch.set_num_threads(usable_cores())
    hist, _ = O.train_loop(sd, cfg, batches, masks, lr, wd)
    for k in hist[0]:
        ref = sum(h[k] for h in hist) / iters
        assert parity(f"epoch-avg/{k}", abs(res[k] - ref) / max(1.0, abs(ref)), TOL[F32]), (k, res[k], ref)


def test_prefetcher_with_device_prep_on_a_256x192_loader():
    from mvlt_amd.batchprep import DeviceBatchPrep, DevicePrefetcher
    H, W, T, Bsz = 256, 192, 32, 3
    batches = [rect_batch(40 + i, Bsz, H, W, T) for i in range(3)]
    slim = [{k: v for k, v in b.items() if k not in ("masked_images", "input_ids", "mlm_labels")} for b in batches]
    got = list(DevicePrefetcher(slim, dev(), prep=DeviceBatchPrep(21, 0.5, "exact")))
    assert len(got) == 3
    for i, g_ in enumerate(got):
        assert tuple(g_["masked_images"].shape) == tuple(g_["image"].shape) == (Bsz, 3, H, W)
        assert tuple(g_["patch_flags"].shape) == (Bsz, 16, 12)
        want = BP.prepare_batch(21, i * Bsz, batches[i]["image"].numpy(), batches[i]["ori_input_ids"].numpy(), int(0.5 * 16 * 12), 0)
        assert np.array_equal(g_["patch_flags"].cpu().numpy(), want["patch_flags"])
        assert np.array_equal(g_["masked_images"].cpu().numpy(), want["masked_images"])
        assert np.array_equal(g_["input_ids"].cpu().numpy(), want["input_ids"]) and np.array_equal(g_["mlm_labels"].cpu().numpy(), want["mlm_labels"])
        assert g_["mlm_count"] == len(want["mlm_positions"]) and np.array_equal(g_["mlm_positions"].cpu().numpy(), want["mlm_positions"])


@pytest.mark.parametrize("dtype", [F32, BF])
def test_eval_callers_on_rectangular_batches(parity, dtype):
    """evaluate_vl on one 256 x 192 batch: its six keys, finite; t2i_psnr against compute_psnr on the oracle's t2i_logits.  A relative error e of the
    prediction moves the mse by at most ~2e, i.e. the PSNR by 10 log10(1 + 2e) ~ 8.7 e dB: 0.01 dB at 1e-3 (fp32), 0.2 dB at 2e-2 (bf16) -- the bounds of
    tests/test_eval_gpu.py.  evaluate_retrieval on `images_101` of shape (1, 101, 3, H, W) and evaluate_recognition run unchanged."""
    from mvlt_amd.evaluate import compute_psnr, evaluate_recognition, evaluate_retrieval, evaluate_vl
    H, W, T = 256, 192, 32
    model, cfg, sd = setup(T, dtype, dp=0.0)
    batch = rect_batch(SEED, B, H, W, T)
    res = evaluate_vl([batch], model, dev(), types.SimpleNamespace(loss_type=LT))
    assert set(res) >= {"mlm_acc", "itm_acc", "sup_cls_acc", "sub_cls_acc", "t2i_psnr", "total_loss"}
    assert all(np.isfinite(res[k]) for k in ("mlm_acc", "itm_acc", "sup_cls_acc", "sub_cls_acc", "t2i_psnr", "total_loss")), res
    torch.set_num_threads(usable_cores())
    with torch.no_grad():
        ref = O.forward(sd, cfg, batch["masked_images"], batch["ori_input_ids"])
    want = compute_psnr(ref["t2i_logits"], batch["image"])
    assert parity("vl/t2i_psnr(dB)", abs(res["t2i_psnr"] - want), 0.01 if dtype == F32 else 0.2), (res["t2i_psnr"], want)
    n = 101
    cand = rect_batch(SEED + 1, n, 64, 32, T)
    item = dict(images_101=cand["image"][:1].repeat(n, 1, 1, 1)[None], ori_input_ids_101=cand["ori_input_ids"][None], info_list=[dict(img_name=str(j)) for j in range(n)])
    assert tuple(item["images_101"].shape) == (1, n, 3, 64, 32)
    r = evaluate_retrieval([item], model, dev(), types.SimpleNamespace(eval_retrieval_tir=True, eval_retrieval_itr=False))
    assert set(r) == {"acc@1", "acc@5", "acc@10"} and all(np.isfinite(v) for v in r.values())
    rec = evaluate_recognition([dict(images=batch["image"], ori_input_ids=batch["ori_input_ids"], sup_cls_labels=batch["sup_cls_labels"],
                                     sub_cls_labels=batch["sub_cls_labels"], info_list=[str(j) for j in range(B)])], model, dev(), types.SimpleNamespace())
    assert len(rec["sup_cls_preds"]) == B and len(rec["sub_cls_preds"]) == B

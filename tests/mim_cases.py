"""Test infrastructure: inputs, float64 references, bars and the host dispatch (re-derived) of the MIM decoder kernel tests
(tests/test_mim_edges_gpu.py; the premises are pinned on the CPU by tests/test_mim_cases_cpu.py).  The kernels: csrc/mim.hip -- train-mode
BatchNorm over pixel-major [M, C] matrices, the align_corners=True bilinear resizes and their adjoints, the fused upsample + SmoothL1 loss and
the feature products.

Plain torch, on whatever device the operands live on.  Every reference is float64 and is computed from the operands AS THE KERNEL READS THEM
(an fp16 z or a bf16 dy is rounded first and widened afterwards; statistics a kernel is handed are the fp32 values it is handed).  N(0,1) data
under one global maximum hides whole classes of wrong kernels; each builder below says which one it is there to expose.
"""
import functools
import math
import types

import torch

BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
# the project's parity bars (tests/test_kernels_gpu.py); an fp16 output: the fp32 bar plus half an fp16 ulp
TOL = {F32: 1e-3, BF: 2e-2, F16: 1e-3 + 2.0 ** -11}
NS = types.SimpleNamespace
EPS, MOMENTUM = 1e-5, 0.1                       # nn.BatchNorm2d defaults (reference libs/vl_heads.py BasicConv2d)
NT, RNT, RWGS = 256, 1024, 256                 # csrc/mim.hip: threads of the element-wise kernels / of the vectorised reductions, their workgroups

# ---- shapes shared by the GPU file and the CPU premises
STATS_WIDTHS = (4, 8, 64, 100, 192, 256)       # col_reduce4_kernel<0, 1024>; 100 and 192: 64 % (C / 4) != 0, the non-shuffle branch
STATS_SCALAR = ((6, 8, 0), (64, 72, 1))        # (C, ld, element offset of the base): col_reduce_kernel<0> by C % 4 and by a misaligned base
COPIES = (1, 4, 16)
RED8 = ((64, 512), (192, 768), (128, 1024), (256, 1024))          # col_reduce8_kernel<NT>: (C, NT)
SWEEP = (1, 2, 3, 4, 5, 7, 8)                  # every (H, W) of the scale-2 resize sweep
L1_DIFFS = (0.0, 0.5, 1.0 - 2.0 ** -10, 1.0, 1.0 + 2.0 ** -10, 1.5, 1e4)
CONSTANTS = (0.0, 3.0, -4.0, 0.1, 4097.0)


def tol(*dtypes):
    """a case is judged against the bar of the narrowest dtype it WRITES (operands are read as stored, their rounding is in the reference)"""
    return TOL[BF] if BF in dtypes else TOL[F16] if F16 in dtypes else TOL[F32]


def f32(v):
    """a Python float as the C ABI passes it (float)"""
    return float(torch.tensor(v, dtype=F32))


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ================================================================================================ the host dispatch of csrc/mim.hip, re-derived
def vec4_ok(C, ld, byte_off=0):
    return C % 4 == 0 and C <= 256 and ld % 4 == 0 and byte_off % 16 == 0


def reduce_rows_per_wg(M, C, nt, wgs=RWGS):
    step = 4 * (nt // (C // 4))
    rows = (M + wgs - 1) // wgs
    return (rows + step - 1) // step * step


def stats_kernel(C, ld, byte_off=0):
    """mvlt_col_stats -> (kernel, template arguments)"""
    return ("col_reduce4_kernel", (0, RNT, F32, F32)) if vec4_ok(C, ld, byte_off) else ("col_reduce_kernel", (0,))


def stats_row_counts(C, nt=RNT):
    """M in {1, 3, rpp - 1, rows_per_wg - 1, rows_per_wg + 1, 4096}: one row, fewer rows than one pass, one idle row slot, one row short of a full
    workgroup (the 4x-unrolled loop ends one pass early, the tail takes three), a second workgroup of one row, several workgroups"""
    rpp = nt // (C // 4)
    step = 4 * rpp
    return tuple(sorted({1, 3, max(rpp - 1, 1), step - 1, step + 1, 4096}))


def bwd_reduce_kernel(C, lddy, ldz, dydt, zdt, dy_off=0, z_off=0, stats_aligned=True):
    """mvlt_bn_bwd_reduce -> (kernel, template arguments, threads) or None where it refuses; *_off: byte offsets of the bases"""
    if not 0 < C <= 256:
        return None
    dy_vec = vec4_ok(C, lddy, dy_off) if dydt is F32 else (C % 4 == 0 and lddy % 4 == 0 and dy_off % 8 == 0)
    z_vec = vec4_ok(C, ldz, z_off) if zdt is F32 else (C % 4 == 0 and ldz % 4 == 0 and z_off % 8 == 0)
    if dydt is BF and not (dy_vec and z_vec):
        return None
    if z_vec and dy_vec and stats_aligned:
        nt = 512 if C <= 64 else 1024
        wide = zdt is F16 and C % 64 == 0 and ldz % 8 == 0 and z_off % 16 == 0 and dy_off % 16 == 0 and lddy % (8 if dydt is BF else 4) == 0
        if wide:
            nt8 = 512 if C == 64 else 768 if C == 192 else 1024
            return ("col_reduce8_kernel", (nt8, dydt), nt8)
        return ("col_reduce4_kernel", (1, nt, dydt, zdt), nt)
    if dydt is not F32 or zdt is not F32:
        return None
    return ("col_reduce_kernel", (1,), NT)


def red8_rows(M, C, nt8):
    """(rows per pass, rows per workgroup, workgroups) of col_reduce8_kernel"""
    rpp8 = (nt8 // 64 // (C // 64)) * 8
    rows8 = (M + RWGS - 1) // RWGS
    rows8 = (rows8 + 4 * rpp8 - 1) // (4 * rpp8) * (4 * rpp8)
    return rpp8, rows8, (M + rows8 - 1) // rows8


def norm_kernel(C, ldz, zdt, y32dt, ld32, y16dt, ld16):
    """mvlt_bn_norm with 16-byte aligned tensors -> (kernel, template arguments) or None where it refuses; y32dt / y16dt None: output absent"""
    if C % 4 or ldz % 4 or (y32dt is None and y16dt is None) or (y32dt is not None and ld32 % 4) or (y16dt is not None and ld16 % 4):
        return None
    op_bf = y16dt is None or y16dt is BF
    if zdt is F16 and not op_bf:
        return None
    if zdt is F16 and C % 8 == 0 and ldz % 8 == 0 and (y16dt is None or ld16 % 8 == 0):
        if y32dt is F16:
            return ("bn_norm8_kernel", (F16,)) if ld32 % 8 == 0 else None
        return ("bn_norm8_kernel", (F32,))
    if y32dt is F16:
        return None
    if zdt is F16:
        return ("bn_norm_kernel", (BF, F16))
    return ("bn_norm_kernel", (BF, F32)) if op_bf else ("bn_norm_kernel", (F32, F32))


def apply_kernel(C, lddy, ldz, lddz, dydt, zdt, dzdt):
    """mvlt_bn_bwd_apply with 16-byte aligned tensors -> (kernel, template arguments, elements per thread)"""
    if zdt is F16 and dzdt is not BF:
        return None
    if zdt is F16 and C % 8 == 0 and ldz % 8 == 0 and lddz % 8 == 0 and lddy % (8 if dydt is BF else 4) == 0:
        return ("bn_bwd_apply8_kernel", (dydt,), 8)
    return ("bn_bwd_apply_kernel", (dzdt, dydt, zdt), 4)


APPLY_ALL = (("bn_bwd_apply8_kernel", (BF,)), ("bn_bwd_apply8_kernel", (F32,)),
             ("bn_bwd_apply_kernel", (BF, BF, F16)), ("bn_bwd_apply_kernel", (BF, F32, F16)), ("bn_bwd_apply_kernel", (BF, BF, F32)),
             ("bn_bwd_apply_kernel", (BF, F32, F32)), ("bn_bwd_apply_kernel", (F32, BF, F32)), ("bn_bwd_apply_kernel", (F32, F32, F32)))


def grid_for(work, cap=8192):
    return min(max((work + NT - 1) // NT, 1), cap)


def upsample_fwd_kernel(B, H, W, C, s, ldx, ldo, odt, nchw):
    """mvlt_upsample_fwd with 16-byte aligned tensors"""
    if nchw and odt is not F32:
        return None
    if nchw and W <= 64 and (W * s) % 4 == 0 and W * s <= 256:
        return ("upsample_fwd_nchw4_kernel", ())
    if nchw:
        return ("upsample_fwd_nchw_kernel", ())
    if C % 4 == 0 and ldx % 4 == 0 and ldo % 4 == 0:
        return ("upsample_fwd_row_kernel", (odt,))
    return ("upsample_fwd_kernel", (odt,))


def upsample_bwd_kernel(B, H, W, C, s, lddy, lddx, dydt, dxdt, nchw):
    """mvlt_upsample_bwd with 16-byte aligned tensors"""
    if dydt is BF:
        if nchw or dxdt is not F32 or C % 4 or lddy % 4 or lddx % 4:
            return None
        return ("upsample_bwd_row_s_kernel", (BF, 2)) if s == 2 else ("upsample_bwd_row_kernel", (BF,))
    if dxdt is BF and not nchw:
        return None
    if nchw and W * s * 4 <= 64 * 1024:
        return ("upsample_bwd_nchw4_kernel" if (W * s) % 4 == 0 and W * s <= 256 else "upsample_bwd_nchw_kernel", (dxdt,))
    if dxdt is BF:
        return None
    if not nchw and C % 4 == 0 and lddy % 4 == 0 and lddx % 4 == 0:
        return ("upsample_bwd_row_s_kernel", (F32, 2)) if s == 2 else ("upsample_bwd_row_kernel", (F32,))
    return ("upsample_bwd_kernel", ())


def l1_ok(W, s):
    return W <= 64 and (W * s) % 4 == 0 and W * s <= 256


def l1_fwd_trips(B, C, H, s):
    """(plane rows, trips the grid-stride loop of upsample_l1_fwd_kernel's busiest workgroup takes)"""
    nrows = B * C * H * s
    groups = (nrows + 7) // 8
    return nrows, (groups + 2047) // 2048


# ================================================================================================ float64 references: BatchNorm
def bn_stats_ref(z, eps=EPS):
    """-> namespace(s1, s2, abs1, mean, var (biased), rstd); abs1 = sum |z| per column: what s1 is a sum OF (s2 is its own sum of absolute terms)"""
    z = z.double()
    M = z.shape[0]
    s1, s2 = z.sum(0), (z * z).sum(0)
    mean = s1 / M
    var = ((z - mean) ** 2).sum(0) / M
    return NS(s1=s1, s2=s2, abs1=z.abs().sum(0), mean=mean, var=var, rstd=(var + f32(eps)).rsqrt(), M=M)


def bn_running_ref(rm, rv, mean, var, M, momentum=MOMENTUM):
    """nn.BatchNorm2d's update: momentum blend, the running variance takes the UNBIASED batch variance (M / (M - 1); M = 1 keeps the biased one,
    where torch itself refuses to train)"""
    m = f32(momentum)
    unb = var * (M / (M - 1)) if M > 1 else var
    return (1 - m) * rm.double() + m * mean.double(), (1 - m) * rv.double() + m * unb.double()


def bn_norm_ref(z, mean, rstd, gamma, beta):
    return (z.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()


def bn_bwd_sums_ref(dy, z, mean, rstd):
    """-> namespace(s1 = sum dy, s2 = sum dy x_hat, abs1, abs2) per column"""
    dy = dy.double()
    xh = (z.double() - mean.double()) * rstd.double()
    t = dy * xh
    return NS(s1=dy.sum(0), s2=t.sum(0), abs1=dy.abs().sum(0), abs2=t.abs().sum(0), xh=xh)


def bn_dz_ref(dy, z, mean, rstd, gamma, s1, s2):
    """dz = gamma rstd (dy - s1 / M - x_hat s2 / M) from the sums the apply kernel is handed"""
    M = z.shape[0]
    xh = (z.double() - mean.double()) * rstd.double()
    return gamma.double() * rstd.double() * (dy.double() - s1.double() / M - xh * s2.double() / M)


# ---- bars
def bar_rows(ref, t):
    """per element, t x max |ref| over the element's row"""
    return t * ref.abs().amax(-1, keepdim=True)


def bar_cols(abs_sum, t):
    """per column, t x the column's sum of absolute terms"""
    return t * abs_sum


# ================================================================================================ BatchNorm builders
def bn_integer_columns(M, C, seed=0):
    """integers in [-8, 8]: sum and sumsq are exact in fp32 in ANY order while M <= 2^24 / 64, so s1 / s2 must be bit-equal to the float64 sums: a
    reduction that drops, doubles or misplaces one row or one column (workgroup seams, the 4x-unrolled tail, the idle row slots at C = 100 / 192) is
    off by an integer.  mean must then be fl(s1 / M) exactly."""
    return torch.randint(-8, 9, (M, C), generator=gen(100 + seed)).to(F32)


def bn_constant_columns(M, C, seed=0):
    """columns 0..4 hold the constants 0, 3, -4, 0.1 (not representable: s2 / M - m^2 is a rounding off zero) and 4097 (C >= 5; fl(4097^2) = 4097^2 - 1 and every
    sum is exact at M <= 4096, so s2 / M - m^2 is -1 where the multiply-subtract is fused and 0 where it is not: a finalize without the clamp at 0 takes the
    root of -1 + eps there and gives NaN, with it the variance is the true 0), the others integers; a finalize without eps gives inf; y of a constant column is
    beta, its dz is finite and within bar"""
    z = bn_integer_columns(M, C, seed)
    for k, v in enumerate(CONSTANTS[: min(len(CONSTANTS), C)]):
        z[:, k] = v
    return z


def bn_offset_columns(M, C, offset=16.0, seed=0):
    """values offset - 1, offset, offset + 1 with 14 of 16 rows AT the offset (variance ~ 1/8): mean^2 / var ~ 2e3 at 16, ~ 5e5 at 255.  Every
    partial sum is exact in fp32 at M <= 4096, so what is measured is the one-pass variance s2 / M - m^2 itself, inside its contract at 16 (asserted)
    and at its limit at 255 (recorded in docs/mim_edges.md)"""
    r = torch.randint(0, 16, (M, C), generator=gen(200 + seed))
    return (offset + (r == 0).to(F32) - (r == 1).to(F32)).to(F32)


def bn_scaled_columns(M, C, seed=0):
    """N(0,1) columns scaled by 1e-3 .. 1e3 (and shifted by a tenth of the scale): under one global maximum a wrong small column is invisible; every
    bar is per column / per row"""
    f = 10.0 ** (torch.arange(C) % 7 - 3).to(F32)
    return (torch.randn(M, C, generator=gen(300 + seed)) + 0.1) * f


def bn_single_row_dy(M, C, row, seed=0):
    """dy zero except in one row (first, last, either side of a rows_per_wg seam): s1 is that row, s2 that row times ITS x_hat -- a reduction that drops or
    doubles the row, or an apply that takes a neighbour column's statistics, is off by a whole term"""
    dy = torch.zeros(M, C)
    dy[row] = torch.randint(1, 5, (C,), generator=gen(400 + seed)).to(F32)
    return dy


def seam_rows(M, rows_per_wg):
    return sorted({r for r in (0, M - 1, rows_per_wg - 1, rows_per_wg) if 0 <= r < M})


def onepass_f32(z):
    """numpy float32 emulation of the kernels' finalize on exact sums: m = s1 / M, var = max(s2 / M - m m, 0), rstd = 1 / sqrt(var + eps)
    -> (mean, var, rstd) float32"""
    import numpy as np
    zz = z.double().numpy()
    M = np.float32(zz.shape[0])
    zf = zz.astype(np.float32)
    s1, s2 = zz.sum(0).astype(np.float32), (zf * zf).astype(np.float64).sum(0).astype(np.float32)       # the kernels square in fp32
    m = (s1 / M).astype(np.float32)
    var = np.maximum((s2 / M).astype(np.float32) - (m * m).astype(np.float32), np.float32(0)).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt((var + np.float32(EPS)).astype(np.float32))).astype(np.float32)
    return torch.from_numpy(m), torch.from_numpy(var), torch.from_numpy(rstd)


# ================================================================================================ resize: float64 matrices
@functools.lru_cache(maxsize=None)
def resize_matrix(n, s):
    """-> (U [n s, n] float64, window [n s, n] bool).  U: the align_corners=True bilinear weights, from integer arithmetic (src = o (n - 1) / (n s - 1),
    split into floor and remainder exactly).  window: |src - i| <= 1, the closed footprint -- where a weight computed from an fp32 coordinate may be
    non-zero at all"""
    no = n * s
    U = torch.zeros(no, n, dtype=torch.float64)
    win = torch.zeros(no, n, dtype=torch.bool)
    for o in range(no):
        num, den = (o * (n - 1), no - 1) if no > 1 else (0, 1)
        i0, rem = divmod(num, den)
        i1 = min(i0 + 1, n - 1)
        w = rem / den
        U[o, i0] += 1.0 - w
        U[o, i1] += w
        for i in range(n):
            win[o, i] = abs(num - i * den) <= den
    return U, win


def coord_slack(n):
    """largest error of an fp32 source coordinate o * r, r = fl((n - 1) / (n s - 1)): three roundings of a value below n - 1 (int -> float is exact)"""
    return 4.0 * max(n - 1, 1) * 2.0 ** -24


def resize_ref(x, H, W, s):
    """x [B, H, W, C] -> namespace(y [B, Ho, Wo, C] = Uy X Ux^T, mag = |Uy| |X| |Ux|^T, slack): slack bounds, element by element, what the fp32
    coordinates may move the result by (a weight moves by at most coord_slack, and only inside the closed footprint; the product of the two axes' weights by
    the two first-order terms and their product)"""
    (Uy, By), (Ux, Bx) = resize_matrix(H, s), resize_matrix(W, s)
    Uy, Ux, By, Bx = (t.to(x.device) for t in (Uy, Ux, By.double(), Bx.double()))
    xd, xa = x.double(), x.double().abs()
    f = lambda A, X, Bm: torch.einsum("oh,bhwc,pw->bopc", A, X, Bm)
    dy, dx = coord_slack(H), coord_slack(W)          # |w'y w'x - wy wx| <= |dwy| wx + wy |dwx| + |dwy| |dwx|
    return NS(y=f(Uy, xd, Ux), mag=f(Uy, xa, Ux), slack=dy * f(By, xa, Ux) + dx * f(Uy, xa, Bx) + dy * dx * f(By, xa, Bx))


def resize_adj_ref(g, H, W, s):
    """g [B, Ho, Wo, C] -> namespace(dx [B, H, W, C] = Uy^T G Ux, mag = |U|^T |G| |U|, slack)"""
    (Uy, By), (Ux, Bx) = resize_matrix(H, s), resize_matrix(W, s)
    Uy, Ux, By, Bx = (t.to(g.device) for t in (Uy, Ux, By.double(), Bx.double()))
    gd, ga = g.double(), g.double().abs()
    f = lambda A, G, Bm: torch.einsum("oh,bopc,pw->bhwc", A, G, Bm)
    dy, dx = coord_slack(H), coord_slack(W)
    return NS(dx=f(Uy, gd, Ux), mag=f(Uy, ga, Ux), slack=dy * f(By, ga, Ux) + dx * f(Uy, ga, Bx) + dy * dx * f(By, ga, Bx))


def bar_resize(ref, t):
    """forward: per element, t x max |ref| over the pixel's channels (its row in the pixel-major matrix), plus the coordinate slack"""
    return t * ref.y.abs().amax(-1, keepdim=True) + ref.slack


def bar_adjoint(ref, t):
    """adjoint: per element, t x (|U|^T |g| |U|), plus the coordinate slack"""
    return t * ref.mag + ref.slack


def resize_delta(B, H, W, C, iy, ix):
    """a single 1 (in every channel) at input pixel (iy, ix): the output IS the pixel's footprint, weight by weight -- a forward that clamps x1 / y1
    wrongly at the last row or column, or mixes up rx and ry on a rectangle, puts weight where there is none"""
    x = torch.zeros(B, H, W, C)
    x[:, iy, ix] = 1.0
    return x


def resize_delta_out(B, Ho, Wo, C, oy, ox):
    """a single 1 at output pixel (oy, ox) of dy: the adjoint is that pixel's (at most four) taps -- with resize_delta it pins the exact tap set; a
    fixed-width tap window that stops short of the footprint loses the tap outright"""
    g = torch.zeros(B, Ho, Wo, C)
    g[:, oy, ox] = 1.0
    return g


def delta_points(H, W):
    """corners, border midpoints and one interior point"""
    ys, xs = sorted({0, H // 2, H - 1}), sorted({0, W // 2, W - 1})
    return [(y, x) for y in ys for x in xs]


def resize_ramp(B, H, W, C, a=3, b=-2, c=5):
    """x = a iy + b ix + c (+ channel): the align_corners resize of an affine map is affine, so the result is known in closed form everywhere,
    the last row and column included: y[oy, ox] = a oy (H-1)/(Ho-1) + b ox (W-1)/(Wo-1) + c"""
    iy, ix = torch.arange(H).view(1, H, 1, 1), torch.arange(W).view(1, 1, W, 1)
    return (a * iy + b * ix + c + torch.arange(C).view(1, 1, 1, C) + torch.zeros(B, 1, 1, 1)).to(F32)


def resize_ramp_ref(B, H, W, C, s, a=3, b=-2, c=5):
    Ho, Wo = H * s, W * s
    ry = (H - 1) / (Ho - 1) if Ho > 1 else 0.0
    rx = (W - 1) / (Wo - 1) if Wo > 1 else 0.0
    oy, ox = torch.arange(Ho, dtype=torch.float64).view(1, Ho, 1, 1), torch.arange(Wo, dtype=torch.float64).view(1, 1, Wo, 1)
    return a * oy * ry + b * ox * rx + c + torch.arange(C, dtype=torch.float64).view(1, 1, 1, C) + torch.zeros(B, 1, 1, 1, dtype=torch.float64)


def resize_random(B, H, W, C, seed=0):
    return torch.randn(B, H, W, C, generator=gen(500 + seed))


def window_s_f32(H, S=2):
    """numpy float32 emulation of upsample_bwd_row_s_kernel<., S>'s tap window for every input row iy of an H-row image: -> list of
    (iy, oy_lo, rows with a non-zero fp32 weight on iy, largest fp32 weight outside [oy_lo, oy_lo + 2 S])"""
    import numpy as np
    Ho = H * S
    ry = np.float32(H - 1) / np.float32(Ho - 1) if Ho > 1 else np.float32(0)
    out = []
    for iy in range(H):
        lo = max(0, int(np.floor(np.float32(iy - 1) / ry))) if ry > 0 else 0
        rows, miss = [], 0.0
        for oy in range(Ho):
            fy = np.float32(oy) * ry
            y0 = int(fy)
            y1 = min(y0 + 1, H - 1)
            wy = np.float32(fy - np.float32(y0))
            w = float((np.float32(1) - wy if y0 == iy else 0.0) + (wy if y1 == iy else 0.0))
            if w != 0.0:
                rows.append(oy)
                if not lo <= oy <= lo + 2 * S:
                    miss = max(miss, w)
        out.append((iy, lo, rows, miss))
    return out


# ================================================================================================ fused upsample + SmoothL1
def l1_ref(x, target, H, W, s, gscale=1.0):
    """x [B, H, W, C], target NCHW [B, C, Ho, Wo] -> namespace(loss_sum, abs_sum, dx [B, H, W, C] = d(mean SmoothL1) / dx x gscale, adj)"""
    r = resize_ref(x, H, W, s)
    d = r.y - target.double().permute(0, 2, 3, 1)
    a = d.abs()
    per = torch.where(a < 1.0, 0.5 * d * d, a - 0.5)
    g = d.clamp(-1.0, 1.0) * (f32(gscale) / d.numel())
    adj = resize_adj_ref(g, H, W, s)
    return NS(loss_sum=per.sum(), abs_sum=per.sum(), dx=adj.dx, adj=adj, pred=r, d=d)


def l1_boundary_target(x, H, W, s, seed=0):
    """target = the float64 prediction -+ {0, 0.5, 1 - 2^-10, 1, 1 + 2^-10, 1.5, 1e4}, dealt over the pixels: both SmoothL1 branches on either side of
    |d| = 1 and, at 1e4, the backward's clamp (an unclamped gradient is off by a factor of 1e4) -> (target NCHW fp32, the difference dealt to each pixel)"""
    pred = resize_ref(x, H, W, s).y
    k = torch.randint(0, 2 * len(L1_DIFFS), pred.shape, generator=gen(600 + seed))
    diffs = torch.tensor(L1_DIFFS, dtype=torch.float64)
    d = diffs[k % len(L1_DIFFS)] * torch.where(k < len(L1_DIFFS), 1.0, -1.0).double()
    return (pred - d).permute(0, 3, 1, 2).contiguous().to(F32), d


# ================================================================================================ products
def product_integers(M, C, n, seed=0):
    """n integer factors in [-4, 4] \\ {0} plus an integer `out` to accumulate onto: every product (|.| <= 256 for dy a b c) and the sum are exact
    in fp32 AND survive a bf16 or fp16 round trip, so each output must be bit-equal to the integer reference -- never to another launch of the kernel"""
    g = gen(700 + seed)
    fac = []
    for _ in range(n):
        v = torch.randint(1, 5, (M, C), generator=g) * (2 * torch.randint(0, 2, (M, C), generator=g) - 1)
        fac.append(v.to(F32))
    return fac

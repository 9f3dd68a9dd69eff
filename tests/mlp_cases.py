"""Test infrastructure: operands, float64 references and bounds of the exact fused-MLP tests (tests/test_mlp_exact_gpu.py; the premises are pinned on
the CPU by tests/test_mlp_cases_cpu.py).  The kernels: csrc/mlp_fused.hip (mlp_fused_kernel), csrc/mlp_pipe.hip (mlp_pipe_kernel), csrc/mlp_wgrad.hip
(mlp_wgrad_kernel, mlp_wgrad2_kernel) -- which of them a launch gets is decided in csrc/mlp_plan.h --, the GELU
epilogues of the NT GEMMs (csrc/gemm_common.h: nt_epilogue_lean) and gelu_bwd.  Plain torch on the CPU, no GPU and no library.  The argument is written down in docs/mlp_exact.md.

Every pre-activation is SATURATED: an integer h with |h| >= SAT.  For a unit that is on (h >= SAT) every GELU form of the tree gives Phi and GELU' within
2^-9 of 1, so the bf16 tile the kernels keep holds h (forward) and dG (backward) exactly and the MLP is two integer GEMMs.  For a unit that is off
(h <= -SAT) the table and erf forms give exactly 0 and the clamped polynomials at most EPS_PHI / EPS_DG: the reference treats the unit as 0 and the case
carries, per output element, the bound of what the off units may add.  All operands are small integers, all sums integers (or halves, under a DropPath
factor of 0.5) below 2^24: the reference must be met bit for bit wherever the bound is 0.
"""
import functools
import types

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NS = types.SimpleNamespace
LIM = float(2 ** 24)
SAT = 16                  # smallest |h| of any case.  (>= 8 is what the polynomial, table and erf forms need; from |h| >= 14 the Gaussian term of the erf derivative,
                          #  exp(-h^2 / 2) <= 2.7e-43, is below fp32 as well, so that the fp32 erf epilogues are exact on BOTH sides.)
# |Phi~(h)| and |GELU'~(h)| of an off unit, for every form in csrc/common.h: the true values at the polynomials' clamps, Phi(-3.985) = 3.4e-5 and
# |GELU'(-4)| = 5.0e-4, plus the documented fit errors 3e-5 and 9.5e-5, with margin.  From the functions and the design bounds, not from a run.
EPS_PHI = 1e-4
EPS_DG = 1e-3
FACTORS = (1.0, 2.0, 0.0, 0.5)          # the DropPath factors of the scaled weight-gradient cases, cycled over the samples


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def sparse_pm1(M, N, P, seed):
    """[M, N] float64 with +-1 exactly where n % P == m % P (sparse_pm1 of tests/test_exact_gpu.py on the CPU): ceil(N / P) nonzeros per row, at most
    ceil(rows / P) per column of any range of consecutive rows"""
    sign = torch.randint(0, 2, (M, N), generator=gen(seed)).double() * 2 - 1
    return sign * (torch.arange(M)[:, None] % P == torch.arange(N)[None, :] % P)


def sparse_w(rows, cols, keep, seed):
    """[rows, cols] float64 weights from {-2, -1, 1, 2}, one entry in `keep` kept (the others 0)"""
    g = gen(seed)
    v = torch.randint(0, 4, (rows, cols), generator=g)
    v = torch.where(v < 2, v - 2, v - 1).double()
    return v * (torch.randint(0, keep, (rows, cols), generator=g) == 0)


def off_units(hid):
    """the hidden units switched off: the even positions of the even 32-unit slices and the odd positions of the odd ones -- every slice, every position of
    a lane's 4 / 8 consecutive units and every 16-unit tile has units of both kinds"""
    j = torch.arange(hid)
    return (j + j // 32) % 2 == 0


def planned(which, C, hid, M, *, h_out=False, rps=0):
    """what ops.mlp_plan names for a launch of this shape ("fwd" / "bwd_dx" / "bwd_dw"; rps: rows_per_scale of a row_scale, 0 for none): the struct of
    include/mvlt_hip_plan.h, .name the kernel.  None where the library is not loadable (these modules otherwise need neither it nor a GPU).  The pointers
    are placeholders: the plan never follows one."""
    try:
        from mvlt_amd import _lib as L, ops
    except (ImportError, OSError):
        return None
    a = L.MlpArgs(x=0x100, dy=0x200, w1=0x300, wb=0x400, wc=0x500, b1=0x600, b2=0x700, residual=0x800, out=0x900, h_out=0xa00 if h_out else None,
                  dw1=0xb00, db1=0xc00, dw2=0xd00, db2=0xe00, row_scale=0xf00 if rps else None, rows_per_scale=rps, M=M, C=C, hid=hid)
    return ops.mlp_plan(which, a)


def wgrad_split(C, hid, M):
    """the token splits of a weight-gradient launch.  This RESTATES the split arithmetic of choose_dw (csrc/mlp_plan.h) and exists only to prove that a
    case reaches the loop it is meant to reach: 64-token tiles per split, splits, rows per split.  Where the library is loadable the plan must say the same."""
    ny = hid // 128
    splits = ((512 if C == 64 else 256) + ny - 1) // ny
    splits = (splits + 7) // 8 * 8
    mtiles = (M + 63) // 64
    splits = max(1, min(splits, mtiles))
    m_per_split = (mtiles + splits - 1) // splits * 64
    splits = (M + m_per_split - 1) // m_per_split
    p = planned("bwd_dw", C, hid, M)
    assert p is None or (p.m_per_split, p.splits, p.ny, p.grid) == (m_per_split, splits, ny, 8 * ((splits + 7) // 8) * ny)
    return NS(tiles=m_per_split // 64, splits=splits, m_per_split=m_per_split, idle=8 * ((splits + 7) // 8) - splits)


def reference(c, *, x=None, swap=None, srow=None):
    """the seven outputs in float64 with every off unit at 0 and every on unit the identity.  The keyword arguments perturb the computation the way a wrong
    kernel would (the CPU test's proof that the comparison notices): another x, two hidden units of G exchanged, other per-row factors."""
    x = c.x.double() if x is None else x
    srow = c.srow if srow is None else srow
    dy, w1, w2 = c.dy.double(), c.w1.double(), c.w2.double()
    h = x @ w1.t() + c.b1.double()
    on = (h > 0).double()
    G = h * on
    if swap is not None:
        G = G.clone()
        G[:, list(swap)] = G[:, list(swap)[::-1]]
    out = (G @ w2.t() + c.b2.double()) * srow + c.res.double()
    dG = dy @ w2
    dx = ((dG * on) @ w1) * srow
    dys = dy * srow
    dHs = (dys @ w2) * on
    return NS(out=out, h=h, dx=dx, dw1=dHs.t() @ x, db1=dHs.sum(0), dw2=dys.t() @ G, db2=dys.sum(0), G=G, dG=dG, dHs=dHs, dys=dys, on=on)


def build(C, hid, M, *, off, factors=None, rps=0, Py=16, keep=4, seed=0):
    """one case: operands as the kernels read them (bf16 x, dy, W1, W2; fp32 b1, b2, residual, factors), the reference and the off-unit bounds.
    x has C / 16 nonzeros per row, dy C / Py; b1 = +-(SAT + max |x W1^T|), so that SAT <= |h| <= SAT + 2 max |x W1^T|."""
    x, dy = sparse_pm1(M, C, 16, seed + 1), sparse_pm1(M, C, Py, seed + 2)
    w1, w2 = sparse_w(hid, C, keep, seed + 3), sparse_w(C, hid, keep, seed + 4)
    mag = SAT + float((x @ w1.t()).abs().max())
    b1 = torch.full((hid,), mag, dtype=F64)
    if off:
        b1[off_units(hid)] = -mag
    b2 = torch.randint(-9, 10, (C,), generator=gen(seed + 5)).double()
    res = torch.randint(-5, 6, (M, C), generator=gen(seed + 6)).double()
    c = NS(C=C, hid=hid, M=M, off=off, rps=rps, x=x.to(BF), dy=dy.to(BF), w1=w1.to(BF), w2=w2.to(BF), b1=b1.float(), b2=b2.float(), res=res.float())
    if factors is None:
        c.scale, c.srow = None, torch.ones(M, 1, dtype=F64)
    else:
        assert rps > 0 and len(factors) == (M + rps - 1) // rps
        c.scale = torch.tensor(factors, dtype=F32)
        c.srow = c.scale.double().repeat_interleave(rps)[:M, None]
    r = c.ref = reference(c)
    offm = 1.0 - r.on
    hP, gD = r.h.abs() * offm * EPS_PHI, r.dG.abs() * offm * EPS_DG            # what an off unit's G and dH may be instead of 0
    c.bound = NS(out=(hP @ w2.abs().t()) * c.srow, h=None, dx=(gD @ w1.abs()) * c.srow, dw1=(gD * c.srow).t() @ x.abs(), db1=(gD * c.srow).sum(0),
                 dw2=(dy.abs() * c.srow).t() @ hP, db2=None)
    return c


def split_partials(c):
    """the partial tiles of dW1 / dW2 one token split leaves (the round-6 path stores them as bf16), for every split of the launch"""
    sp, r = wgrad_split(c.C, c.hid, c.M), c.ref
    xs = c.x.double()
    for z in range(sp.splits):
        rows = slice(z * sp.m_per_split, min(c.M, (z + 1) * sp.m_per_split))
        yield z, r.dHs[rows].t() @ xs[rows], r.dys[rows].t() @ r.G[rows]


def bf16_exact(t):
    return torch.equal(t.float().to(BF).double(), t)


def compare(got, ref64, bound=None, what=""):
    """fp32 got: |got - ref| <= bound elementwise (no bound, or 0 there: equal); bf16 got: the same against the reference rounded once to nearest-even,
    which with a bound becomes half a bf16 ulp of the reference on top.  A failure names (row, col, got, want)."""
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    g = got.double()
    if got.dtype == F32:
        want, slack = ref64, torch.zeros_like(ref64)
    else:
        assert got.dtype == BF, got.dtype
        want, slack = ref64.float().to(BF).double(), torch.zeros_like(ref64)
        if bound is not None:                               # half an ulp of 8 significant bits: 2^(floor(log2 |ref|) - 8)
            want = ref64
            slack = torch.ldexp(torch.ones_like(ref64), torch.frexp(ref64)[1] - 9) * (ref64 != 0)
    if bound is not None:
        slack = slack + bound.to(ref64.device)
    bad = ~((g - want).abs() <= slack)                      # (a NaN is bad)
    if not bool(bad.any()):
        return
    bad2 = bad.reshape(bad.shape[0], -1) if bad.dim() > 1 else bad.reshape(-1, 1)
    g2, w2 = g.reshape(bad2.shape), want.reshape(bad2.shape)
    idx = bad2.nonzero()
    first = [(int(r), int(k), float(g2[r, k]), float(w2[r, k])) for r, k in idx[:8].tolist()]
    raise AssertionError(f"{what}: {int(bad2.sum())} of {bad2.numel()} elements wrong; first (row, col, got, want): {first}; rows {int(idx[:, 0].min())}.."
                         f"{int(idx[:, 0].max())}, cols {int(idx[:, 1].min())}..{int(idx[:, 1].max())}")


# ---------------------------------------------------------------------------------------------------------------- the cases
# forward and input gradient: (hid, h_out) -> kernel family
FWD_GEOMS = ((64, False, "mlp_fused_kernel"), (128, False, "mlp_pipe_kernel"), (192, False, "mlp_pipe_kernel"), (192, True, "mlp_fused_kernel"))
# M, rows_per_scale, factors: one row; a second 32-row wave with one row; a second workgroup with one row (the last sample short); four samples of 50 rows
FWD_ROWS = ((1, 0, None), (33, 33, (2.0,)), (129, 50, (0.5, 2.0, 1.0)), (200, 50, (2.0, 0.0, 0.5, 1.0)))
FWD_CASES = [(C, hid, h_out, fam, M, rps, fac, off) for C in (64, 128) for hid, h_out, fam in FWD_GEOMS for M, rps, fac in FWD_ROWS for off in (False, True)]


@functools.lru_cache(maxsize=None)
def fwd_case(C, hid, M, rps, factors, off):
    return build(C, hid, M, off=off, factors=factors, rps=rps, Py=16, keep=8 if C == 128 or hid > 128 else 4, seed=100 + C + hid + M)       # sparser weights where more terms meet: dx <= 256, bounds <= 1/4


# weight gradients, tile-uniform factor (mlp_wgrad2_kernel): name, C, hid, M
WG_SINGLE = [(f"single-{C}-{M}", C, 128, M) for C in (64, 128) for M in (1, 63, 65)]
WG_MULTI = [("multi-tile-64-4241", 64, 1024, 4241), ("multi-tile-128-2193", 128, 1024, 2193), ("multi-tile-128-4177", 128, 1024, 4177)]
WG_CASES = [(name, C, hid, M, scaled) for name, C, hid, M in WG_SINGLE + WG_MULTI for scaled in (False, True)]
DROPPED_SPLIT = 1                       # the split of a scaled multi-tile case whose every tile is dropped


def wg_factors(C, hid, M):
    """rows_per_scale = 64, FACTORS cycled over the samples; with several tiles per split one whole split is dropped"""
    sp = wgrad_split(C, hid, M)
    f = [FACTORS[b % 4] for b in range((M + 63) // 64)]
    if sp.tiles > 1:
        for b in range(DROPPED_SPLIT * sp.tiles, (DROPPED_SPLIT + 1) * sp.tiles):
            f[b] = 0.0
    return tuple(f)


@functools.lru_cache(maxsize=None)
def wg_case(C, hid, M, scaled):
    # dy with ONE nonzero row per column and 64-token tile: a partial tile of dW2 sums at most `tiles` pre-activations (all of one sign on an all-on case)
    multi = wgrad_split(C, hid, M).tiles > 1
    return build(C, hid, M, off=not multi, factors=wg_factors(C, hid, M) if scaled else None, rps=64 if scaled else 0, Py=64, keep=8, seed=200 + C + M)


# weight gradients, factor per row (mlp_wgrad_kernel: rows_per_scale % 64 != 0): C, hid, rows_per_scale, factors
R2_CASES = [(C, hid, rps, fac) for C, hid in ((64, 256), (128, 128)) for rps, fac in (
    (100, (2.0, 0.5, 1.0)),
    (52, (1.0, 0.0, 0.5, 1.0, 2.0, 0.5, 1.0)),              # tile [256, 320): the tail of sample 4, all of sample 5, the head of sample 6 -- three different factors
    (20, tuple(FACTORS[b % 4] for b in range(13))))]        # four samples per tile


@functools.lru_cache(maxsize=None)
def r2_case(C, hid, rps, factors):
    return build(C, hid, rps * len(factors), off=True, factors=factors, rps=rps, Py=64, keep=8, seed=300 + C + rps)


def gemm_case(M, N, K, seed):
    """saturated operands of the GEMM GELU epilogues: A sparse +-1, W in [-2, 2], bias = +-(SAT + max |A W^T|) with the sign alternating over the columns
    in runs of 1, 2, 3: h = A W^T + bias, its activation G and, for act 2, the integer product v = A W^T against the pre-activation H = h"""
    A = sparse_pm1(M, K, 16, seed)
    W = torch.randint(-2, 3, (N, K), generator=gen(seed + 1)).double()
    return saturated(A, W)


def saturated(A, W):
    """gemm_case on given float64 operands (tests/gemm_inst_cases.py hands over a GATHERED A): the bias magnitude is SAT plus the maximum of this product"""
    N = W.shape[0]
    v = A @ W.t()
    mag = SAT + float(v.abs().max())
    n = torch.arange(N)
    sign = torch.where((n % 6 == 0) | (n % 6 == 2) | (n % 6 == 3), -1.0, 1.0).double()
    bias = sign * mag
    h = v + bias
    on = (h > 0).double()
    return NS(A=A, W=W, bias=bias.float(), v=v, h=h, on=on, G=h * on, dH=v * on, bound_G=h.abs() * (1 - on) * EPS_PHI, bound_dH=v.abs() * (1 - on) * EPS_DG)

"""GPU: the row-wise kernels -- csrc/norm.hip (LayerNorm forward / backward) and, in csrc/elementwise.hip, bert_embed_*, ce_fwd / ce_loss_finish /
ce_bwd and the two SmoothL1 kernels -- on inputs built to make one wrong formula or one dropped row an error of many bars, through every code path
the dispatch has, against the float64 references of tests/rowwise_cases.py.  The inputs' premises are pinned on the CPU by
tests/test_rowwise_cases_cpu.py.

Bars: the project's 1e-3 (fp32) / 2e-2 (bf16) -- the narrowest dtype a case reads or writes decides --, applied per row or per column instead of
against one global maximum:
  LayerNorm y     per element, TOL x max|ref| over the row           mean   TOL x max(|ref|, row std)        rstd   relative TOL
  LayerNorm dx    per element, 2 TOL x max|ref| over the row         dgamma, dbeta   TOL x the column's sum of absolute terms
  lse, loss mean  TOL x max(1, |ref|)
  dlogits         per element, TOL x gscale / max(count, 1), plus half a bf16 ulp of the element for bf16 output
  BERT dword / dpos rows   as LayerNorm dx, per table row            dtype0 as dgamma
Where the input makes the answer exact (constant rows, single-row dy, untouched rows, masked columns, SmoothL1 on eighths) the check is torch.equal.
A failure prints the case, the instantiation (mvlt_amd._lib.last_kernel()), row, column, the value got and the value wanted.

EVERY launch goes through the wrappers below: operands and results live in flat buffers filled with the sentinel 7.0, leading dimensions are larger
than C or V wherever the entry point takes one, one guard row sits behind every matrix and one guard element behind every vector; after the launch
every sentinel must be bit-identical (integer view).  ce_bwd zeroes the columns [V, ldd) by contract: exactly that is asserted, the guards sit behind ldd.

Instantiation -> the case that launches it and asserts its name:
  ln_fwd_fixed_kernel<T, TY, G, ITS, RU>   test_ln_fwd_every_instantiation, all four (T, TY): C 64 <8,1,2>  128 <16,1,2>  320 <8,5,1>  512 <16,4,1>  768 <32,3,1>
  ln_fwd_kernel<T, TY, G>                  test_ln_fwd_every_instantiation, all four (T, TY): C 8, 72 <8>  192 <16>  256 <32>  1000, 1024 <64>
  ln_bwd_kernel<T, TX, TDX, G, ITS, 1024>  test_ln_bwd_every_dtype_triple: all eight (T, TX, TDX) at C 320 <32,2>;
                                           test_ln_bwd_past_the_grid_stride_threshold: C 64, 8 <8,1>  72 <8,2>  128 <16,1>  256 <32,1>  320 <32,2>  512 <64,1>  768, 1024 <64,2>
  bert_embed_fwd_kernel<T, 768>, bert_embed_bwd_kernel<T, 768, 1024>    test_bert_embed, T = bf16 and float
  ce_loss_finish_kernel<T>                 every cross-entropy forward of this file, T = bf16 and float; ce_fwd_kernel<T> is launched by the same call under the
                                           same dtype switch right before it (the finish kernel is the last launch, so its name is the one that can be asked for)
  ce_bwd_kernel<T, TO>                     test_ce_data: all four (T, TO)
  smooth_l1_sum_kernel, smooth_l1_grad_kernel   test_smooth_l1_exact, test_smooth_l1_boundaries

Measured on an MI355X, worst error / bar per kernel and dtype (against the float64 reference; these are measurements and gate nothing):
  ln_fwd   y: bf16->bf16 0.195, fp32->bf16 0.190, fp32->fp32 0.027 (offset rows, C 1000), bf16->fp32 8.6e-6; mean 1.9e-4; rstd 3.4e-4;
           chained y2 0.19, mean2 2.0e-5, rstd2 1.1e-4                 (0.19 = the rounding of a bf16 output: 2^-9 of an element against 2e-2 of the row maximum)
  ln_bwd   dx 0.097 (bf16 dx), dx2 fp32 1.0e-4 / bf16 0.078; dgamma fp32 1.4e-4 / bf16 6.6e-6; dbeta fp32 7.7e-5 / bf16 1.1e-6
  bert     y fp32 2.8e-4 / bf16 0.19; mean 1.7e-5; rstd 1.4e-4; fp32 dword 1.2e-3, dpos 1.5e-4, dtype0 1.8e-4, dgamma 3.1e-3, dbeta 1.6e-4 (bf16 dy: all below 1.6e-4)
  ce       lse fp32 7.9e-5 / bf16 4.2e-6; loss mean fp32 1.7e-4 / bf16 2.8e-5; dlogits fp32->fp32 3.6e-3, bf16->fp32 1.6e-4, bf16 output 0.13
  sl1      exact cases bit-equal; boundaries loss_sum 1.5e-8, grad 4.5e-8 of a 2^-22 relative bar
(docs/rowwise_edges.md has the same figures as a table)
"""
import math

import pytest
import torch

from tests import rowwise_cases as rc

pytestmark = pytest.mark.gpu

BF, F32 = rc.BF, rc.F32
DT_ID = {BF: "bf16", F32: "fp32"}
SENTINEL = 7.0
INT_VIEW = {BF: torch.int16, F32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64}
PAIRS = [(BF, BF), (BF, F32), (F32, BF), (F32, F32)]
PAIR_IDS = [f"{DT_ID[a]}-{DT_ID[b]}" for a, b in PAIRS]
EPS = 1e-6


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as _ops
    return _ops


def last_kernel():
    from mvlt_amd._lib import last_kernel as lk
    return lk()


def rowmap(rmap):
    from mvlt_amd._lib import rowmap as make
    return make(*rmap) if rmap is not None else None


def ran(base, *targs):
    """the kernel launched last on this thread must be the instantiation base<targs>.  Instantiations over the bf16 element type come back mangled (the
    C++ runtime's demangler does not know that type): the template arguments are looked up in the mangled form then."""
    name = last_kernel()
    if not targs:
        assert name == base, f"meant to reach {base}, the library launched {name}"
    elif name.startswith("_Z"):
        enc = lambda t: "DF16b" if t is BF else "f" if t is F32 else f"Li{t}E"
        want = f"{len(base)}{base}I" + "".join(enc(t) for t in targs) + "E"
        assert want in name, f"meant to reach {base}{targs} ({want}), the library launched {name}"
    else:
        # (the same demangler reads the bf16 code "DF16b" as a fixed-point type and swallows the character behind it: <bf16, float, ...> comes back as
        # <bool _Accum, ...>; bf16 followed by anything else fails to parse and comes back mangled, the branch above)
        txt = lambda t: "float" if t is F32 else str(t)
        parts, i = [], 0
        while i < len(targs):
            pair = targs[i] is BF and i + 1 < len(targs) and targs[i + 1] is F32
            parts.append("bool _Accum" if pair else txt(targs[i]))
            i += 2 if pair else 1
        want = f"{base}<" + ", ".join(parts) + ">"
        assert name == want, f"meant to reach {want}, the library launched {name}"


# ------------------------------------------------------------------------------------------------ buffers and guards
def sentinels_intact(flat, dead, dtype, what):
    got = flat.view(INT_VIEW[dtype])[dead]
    want = torch.tensor([SENTINEL], dtype=dtype).view(INT_VIEW[dtype]).to(flat.device)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {got.numel()} sentinels overwritten; first at flat element "
                              f"{int(dead.nonzero()[bad[0, 0], 0])} of {dead.numel()}; last kernel {last_kernel()}")


class Mat:
    """[rows, C] inside a flat device buffer of sentinels: rows `ld` = C + pad apart, logical row r at the physical row of the mode-0 row map `rmap`
    (rows_per_batch, batch_stride, offset), one guard row behind the last physical row"""

    def __init__(self, rows, C, dtype, dense=None, fill=0.0, pad=8, rmap=None, nphys=None):
        self.C, self.ld, self.dtype, self.rmap = C, C + pad, dtype, rmap
        self.prow = rc.phys_rows(rows, rmap).to(dev())
        self.nphys = nphys or int(self.prow.max()) + 1
        self.t = torch.full(((self.nphys + 1) * self.ld,), SENTINEL, dtype=dtype, device=dev())
        self.m = self.t[: self.nphys * self.ld].view(self.nphys, self.ld)
        self.m[self.prow, :C] = dense.to(device=dev(), dtype=dtype) if dense is not None else fill

    def dense(self):
        return self.m[self.prow, : self.C]

    def check(self, what):
        dead = torch.ones(self.nphys + 1, self.ld, dtype=torch.bool, device=dev())
        dead[self.prow, : self.C] = False
        sentinels_intact(self.t, dead.view(-1), self.dtype, what)


class Vec:
    """n live elements (at `idx` of a `size`-element vector when given) and one guard element behind them"""

    def __init__(self, n, dense=None, fill=0.0, idx=None, size=None, dtype=F32):
        self.idx = (idx if idx is not None else torch.arange(n)).to(dev())
        self.size, self.dtype = (size or n) + 1, dtype
        self.t = torch.full((self.size,), SENTINEL, dtype=dtype, device=dev())
        self.t[self.idx] = dense.to(device=dev(), dtype=dtype) if dense is not None else fill

    def dense(self):
        return self.t[self.idx]

    def check(self, what):
        dead = torch.ones(self.size, dtype=torch.bool, device=dev())
        dead[self.idx] = False
        sentinels_intact(self.t, dead, self.dtype, what)


def check_all(what, **bufs):
    torch.cuda.synchronize()
    for name, b in bufs.items():
        if b is not None:
            b.check(f"{what}, {name}")


# ------------------------------------------------------------------------------------------------ judging
def judge(parity, name, what, got, ref, bar):
    """|got - ref| <= bar element by element (bar broadcasts: one per row, per column or per element); records the worst error / bar"""
    got = got.double()
    if got.dim() == 1:
        got, ref, bar = got[:, None], ref[:, None], (bar[:, None] if torch.is_tensor(bar) and bar.dim() == 1 else bar)
    bar = torch.as_tensor(bar, dtype=torch.float64, device=got.device).expand_as(got)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, math.inf))
    i = int(ratio.argmax())
    r, c = i // got.shape[1], i % got.shape[1]
    assert parity(f"{name}/{what}", ratio.max(), 1.0), (
        f"{what}: {name} row {r} column {c}: got {float(got[r, c])!r}, want {float(ref[r, c])!r}, bar {float(bar[r, c]):.3e} "
        f"({float(ratio[r, c]):.2f} bars); last kernel {last_kernel()}")


def exact(name, what, got, want):
    if got.dim() == 1:
        got, want = got[:, None], want[:, None]
    want = want.to(got.dtype).expand_as(got)
    if not torch.equal(got, want):
        bad = ((got != want) | torch.isnan(got)).nonzero()
        r, c = int(bad[0, 0]), int(bad[0, 1])
        raise AssertionError(f"{what}: {name} must be exact; {bad.shape[0]} elements differ, first at row {r} column {c}: got {float(got[r, c])!r}, "
                             f"want {float(want[r, c])!r}; last kernel {last_kernel()}")


def refused(call, *untouched):
    """an argument check that returns before any launch: MVLTError, the last kernel's name unchanged, nothing written"""
    from mvlt_amd._lib import MVLTError
    before = last_kernel()
    with pytest.raises(MVLTError):
        call()
    torch.cuda.synchronize()
    assert last_kernel() == before
    for t in untouched:
        assert bool((t == SENTINEL).all())


# ================================================================================================ LayerNorm forward
FWD_FIXED = {64: (8, 1, 2), 128: (16, 1, 2), 320: (8, 5, 1), 512: (16, 4, 1), 768: (32, 3, 1)}
FWD_WIDTHS = sorted(set(rc.LN_FIXED + rc.LN_GENERIC))


def ran_ln_fwd(C, xdt, ydt):
    if C in FWD_FIXED:
        ran("ln_fwd_fixed_kernel", xdt, ydt, *FWD_FIXED[C])
    else:
        ran("ln_fwd_kernel", xdt, ydt, rc.pick_group(C))


def fwd_row_counts(C):
    g, _, ru = FWD_FIXED.get(C, (rc.pick_group(C), 0, 1))
    groups = 256 // g
    return (1, groups - 1, groups * ru + 1)


def run_ln_fwd(ops, what, x, gamma, beta, eps, xdt, ydt, *, x_map=None, y_map=None, add=None, add_rows=0, chain=None, y_fill=0.0):
    """-> (namespace of dense device results y, mean, rstd[, y2, mean2, rstd2], float64 reference from the operands as stored)"""
    rows, C = x.shape
    xb, yb = Mat(rows, C, xdt, x, rmap=x_map), Mat(rows, C, ydt, rmap=y_map, fill=y_fill)
    mean, rstd = Vec(rows), Vec(rows)
    g, b = gamma.to(dev()), beta.to(dev())
    addb = Vec(add.numel(), add.reshape(-1)) if add is not None else None
    kw, y2 = {}, None
    if chain is not None:
        g2, b2, eps2 = chain[0].to(dev()), chain[1].to(dev()), chain[2]
        y2 = Mat(rows, C, BF, rmap=y_map)
        mean2, rstd2 = Vec(rows, idx=yb.prow, size=yb.nphys), Vec(rows, idx=yb.prow, size=yb.nphys)
        kw["chain"] = (g2, b2, eps2, y2.t, mean2.t, rstd2.t)
    ops.layernorm_fwd(xb.t, yb.t, g, b, rows, C, xb.ld, yb.ld, eps, mean=mean.t, rstd=rstd.t, add=addb.t if addb else None, add_rows=add_rows,
                      x_map=rowmap(x_map), y_map=rowmap(y_map), **kw)
    ran_ln_fwd(C, xdt, ydt)
    out = rc.NS(y=yb.dense(), mean=mean.dense(), rstd=rstd.dense())
    bufs = dict(x=xb, y=yb, mean=mean, rstd=rstd, add=addb)
    if chain is not None:
        bufs.update(y2=y2, mean2=mean2, rstd2=rstd2)
        out.y2, out.mean2, out.rstd2 = y2.dense(), mean2.dense(), rstd2.dense()
    check_all(what, **bufs)
    ref = rc.ln_fwd_ref(xb.dense(), g, b, eps, add=add.to(dev()) if add is not None else None, add_rows=add_rows,
                        chain=(g2, b2, eps2) if chain is not None else None)
    return out, ref


def judge_ln_fwd(parity, what, out, ref, xdt, ydt):
    t = rc.tol(xdt, ydt)
    tag = f"{DT_ID[xdt]}->{DT_ID[ydt]}"
    judge(parity, f"ln_fwd y {tag}", what, out.y, ref.y, rc.bar_y(ref.y, t))
    judge(parity, f"ln_fwd mean {tag}", what, out.mean, ref.mean, rc.bar_mean(ref, t))
    judge(parity, f"ln_fwd rstd {tag}", what, out.rstd, ref.rstd, t * ref.rstd)
    if hasattr(out, "y2"):
        t2 = rc.TOL[BF]
        second = rc.NS(mean=ref.mean2, std=ref.std2)
        judge(parity, f"ln_fwd y2 {tag}", what, out.y2, ref.y2, rc.bar_y(ref.y2, t2))
        judge(parity, f"ln_fwd mean2 {tag}", what, out.mean2, ref.mean2, rc.bar_mean(second, t))
        judge(parity, f"ln_fwd rstd2 {tag}", what, out.rstd2, ref.rstd2, t * ref.rstd2)


@pytest.mark.parametrize("xdt,ydt", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("C", FWD_WIDTHS)
def test_ln_fwd_every_instantiation(ops, parity, C, xdt, ydt):
    """scaled rows (eps carries weight in a third of them) at 1, GROUPS - 1 and GROUPS x RU + 1 rows: one row, one idle row group, and a second workgroup
    whose RU = 2 pair has a dead second row"""
    g, b = rc.ln_params(C)
    for rows in fwd_row_counts(C):
        what = f"C{C} rows{rows} scaled"
        out, ref = run_ln_fwd(ops, what, rc.ln_scaled_rows(rows, C, seed=rows), g, b, EPS, xdt, ydt)
        judge_ln_fwd(parity, what, out, ref, xdt, ydt)


@pytest.mark.parametrize("dt", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("C", FWD_WIDTHS)
def test_ln_fwd_offset_and_constant_rows(ops, parity, C, dt):
    g, b = rc.ln_params(C)
    rows = 200
    if C in rc.LN_OFFSET_WIDTHS:
        what = f"C{C} offset rows"
        out, ref = run_ln_fwd(ops, what, rc.ln_offset_rows(rows, C), g, b, EPS, dt, dt)
        judge_ln_fwd(parity, what, out, ref, dt, dt)
    what = f"C{C} constant rows"
    x = rc.ln_constant_rows(rows, C)
    out, ref = run_ln_fwd(ops, what, x, g, b, EPS, dt, dt)
    exact("y == beta", what, out.y, b.to(dev()).to(dt)[None, :])
    exact("mean == c", what, out.mean, x[:, 0].to(dev()))
    judge(parity, f"ln_fwd rstd {DT_ID[dt]}->{DT_ID[dt]}", what, out.rstd, torch.full_like(ref.rstd, rc.f32(EPS) ** -0.5), rc.tol(dt) * ref.rstd)


MAPPED = [(64, BF, F32), (128, F32, BF), (320, BF, BF), (512, F32, F32), (768, BF, F32), (72, BF, F32), (1000, F32, BF)]


@pytest.mark.parametrize("C,xdt,ydt", MAPPED, ids=[f"C{C}-{DT_ID[a]}-{DT_ID[b]}" for C, a, b in MAPPED])
def test_ln_fwd_add_and_row_maps(ops, parity, C, xdt, ydt):
    """"+ pos_embed" (row r takes add[r % add_rows]) into the image range and into the text range of a (B, HW + T, C) buffer, x read through a row map of
    its own; the widths of the fixed kernel chain the second LayerNorm (768 too)"""
    B, HW, T = 3, 20, 7
    g, b = rc.ln_params(C)
    chain = rc.ln_params(C, seed=5) + (1e-5,) if C in FWD_FIXED else None
    for n, off in ((HW, 0), (T, HW)):
        what = f"C{C} rows {off}..{off + n} of every {HW + T}"
        add = torch.randn(n, C, generator=rc.gen(3))
        out, ref = run_ln_fwd(ops, what, rc.ln_scaled_rows(B * n, C, seed=off), g, b, EPS, xdt, ydt, x_map=(n, n + 3, 2), y_map=(n, HW + T, off),
                              add=add, add_rows=n, chain=chain)
        judge_ln_fwd(parity, what, out, ref, xdt, ydt)


@pytest.mark.parametrize("C", rc.LN_FIXED)
def test_ln_fwd_chained_constant_rows(ops, parity, C):
    """gamma1 = 0, beta1 = 3: whatever x is, the first output is the constant row 3, so the chained norm must return mean2 == 3, rstd2 == 1 / sqrt(eps2) -- NOT
    1 / sqrt(eps) -- and y2 == beta2 bit for bit"""
    eps, eps2 = 1e-5, 1e-6
    g2, b2 = rc.ln_params(C, seed=1)
    what = f"C{C} chained constant rows"
    out, ref = run_ln_fwd(ops, what, rc.ln_scaled_rows(50, C), torch.zeros(C), torch.full((C,), 3.0), eps, F32, F32, y_map=(10, 13, 1), chain=(g2, b2, eps2))
    exact("y == beta1", what, out.y, torch.full((1, C), 3.0, device=dev()))
    exact("y2 == beta2", what, out.y2, b2.to(dev()).to(BF)[None, :])
    exact("mean2 == 3", what, out.mean2, torch.full((50,), 3.0, device=dev()))
    judge(parity, "ln_fwd rstd2 fp32->fp32", what, out.rstd2, torch.full_like(ref.rstd2, rc.f32(eps2) ** -0.5), rc.TOL[F32] * ref.rstd2)


GRID_STRIDE_FWD = [(8, 8192 * 32 + 5, F32, F32), (64, 8192 * 32 * 2 + 33, BF, BF)]


@pytest.mark.parametrize("C,rows,xdt,ydt", GRID_STRIDE_FWD, ids=["generic-C8", "fixed-C64"])
def test_ln_fwd_grid_stride(ops, parity, C, rows, xdt, ydt):
    """more rows than 8192 workgroups cover in one pass: the row loop of either kernel takes a second trip, ragged"""
    g, b = rc.ln_params(C)
    what = f"C{C} rows{rows}"
    out, ref = run_ln_fwd(ops, what, rc.ln_scaled_rows(rows, C), g, b, EPS, xdt, ydt)
    judge_ln_fwd(parity, what, out, ref, xdt, ydt)


@pytest.mark.parametrize("C", [1032, 12])
def test_ln_fwd_refuses_unsupported_widths(ops, C):
    rows = 5
    x, y = Mat(rows, C, F32, torch.randn(rows, C), pad=0 if C % 8 else 8), Mat(rows, C, F32, fill=SENTINEL, pad=0 if C % 8 else 8)
    g, b = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
    mean, rstd = Vec(rows, fill=SENTINEL), Vec(rows, fill=SENTINEL)
    refused(lambda: ops.layernorm_fwd(x.t, y.t, g, b, rows, C, x.ld, y.ld, EPS, mean=mean.t, rstd=rstd.t), y.t, mean.t, rstd.t)


# ================================================================================================ LayerNorm backward
TRIPLES = [(a, b, c) for a in (BF, F32) for b in (BF, F32) for c in (BF, F32)]
# (dy, x, dx) dtypes per width past the grid-stride threshold: the model's combinations, spread over the widths
BWD_DT = {64: (BF, F32, BF), 128: (BF, BF, BF), 320: (BF, F32, F32), 512: (F32, F32, F32), 768: (BF, F32, BF), 8: (F32, F32, F32), 72: (BF, BF, F32),
          256: (F32, BF, BF), 1024: (BF, F32, BF)}


def ran_ln_bwd(C, dts):
    g = rc.pick_group(C)
    ran("ln_bwd_kernel", *dts, g, 1 if g * 8 >= C else 2, 1024)


def run_ln_bwd(ops, what, dy, x, gamma, dts, *, maps=(None, None, None), base=None, copies=1, dx2_scales=None, rows_per_scale=0, eps=EPS):
    """-> (namespace dx, dgamma, dbeta[, dx2] dense on the device, float64 reference).  The backward is handed the fp32-rounded statistics of the float64
    forward and is judged against the reference that uses the same ones.  base: the pre-existing dx (accumulate); copies > 1: dgamma / dbeta land in an
    arena of `copies` x [dgamma | dbeta | 8 sentinels] and are folded by ops.fold_copies."""
    T, TX, TDX = dts
    rows, C = x.shape
    dyb, xb = Mat(rows, C, T, dy, rmap=maps[0]), Mat(rows, C, TX, x, rmap=maps[1])
    dxb = Mat(rows, C, TDX, base, rmap=maps[2], fill=SENTINEL if base is None else 0.0)
    g = gamma.to(dev())
    f = rc.ln_fwd_ref(xb.dense(), g, torch.zeros_like(g), eps)
    mean, rstd = Vec(rows, f.mean), Vec(rows, f.rstd)
    stride = 2 * C + 8
    live = (torch.arange(copies)[:, None] * stride + torch.arange(2 * C)[None, :]).reshape(-1)
    arena = Vec(live.numel(), idx=live, size=copies * stride)
    kw, dx2 = {}, None
    if dx2_scales is not None:
        dx2, sc = Mat(rows, C, T, fill=SENTINEL), Vec(len(dx2_scales), torch.tensor(dx2_scales))
        kw = dict(dx2=dx2.t, dx2_scale=sc.t, dx2_rows_per_scale=rows_per_scale, lddx2=dx2.ld)
    ops.layernorm_bwd(dyb.t, xb.t, dxb.t, g, mean.t, rstd.t, rows, C, dyb.ld, xb.ld, dxb.ld, dgamma=arena.t, dbeta=arena.t[C:],
                      dy_map=rowmap(maps[0]), x_map=rowmap(maps[1]), dx_map=rowmap(maps[2]), accumulate=base is not None,
                      copies=copies, copy_stride=stride, **kw)
    ran_ln_bwd(C, dts)
    check_all(what, dy=dyb, x=xb, dx=dxb, mean=mean, rstd=rstd, arena=arena, dx2=dx2)
    if copies > 1:
        folded = Vec(2 * C)
        ops.fold_copies(arena.t, copies, stride, torch.arange(2 * C, dtype=torch.int32, device=dev()), 0, 2 * C, folded.t)
        check_all(what + " fold", arena=arena, folded=folded)
        assert bool((arena.dense() == 0).all()), "fold_copies leaves the arena zeroed"
        cols = folded.dense()
    else:
        cols = arena.dense()
    out = rc.NS(dx=dxb.dense(), dgamma=cols[:C], dbeta=cols[C:], dx2=dx2.dense() if dx2 is not None else None)
    ref = rc.ln_bwd_ref(dyb.dense(), xb.dense(), g, mean.dense(), rstd.dense())
    if base is not None:
        ref.dx = ref.dx + base.to(dev()).to(TDX).double()
    return out, ref


def judge_ln_bwd(parity, what, out, ref, dts):
    t = rc.tol(*dts)
    tag = "/".join(DT_ID[d] for d in dts)
    judge(parity, f"ln_bwd dx {tag}", what, out.dx, ref.dx, rc.bar_dx(ref.dx, t))
    judge(parity, f"ln_bwd dgamma {tag}", what, out.dgamma, ref.dgamma, rc.bar_col(ref.abs_gamma, t))
    judge(parity, f"ln_bwd dbeta {tag}", what, out.dbeta, ref.dbeta, rc.bar_col(ref.abs_beta, t))


@pytest.mark.parametrize("dts", TRIPLES, ids=["-".join(DT_ID[d] for d in t) for t in TRIPLES])
def test_ln_bwd_every_dtype_triple(ops, parity, dts):
    C, rows = 320, 77
    g, _ = rc.ln_params(C)
    dy = torch.randn(rows, C, generator=rc.gen(2))
    for base in (None, torch.randn(rows, C, generator=rc.gen(3))):
        what = f"C{C} rows{rows} scaled{' accumulate' if base is not None else ''}"
        out, ref = run_ln_bwd(ops, what, dy, rc.ln_scaled_rows(rows, C), g, dts, base=base)
        judge_ln_bwd(parity, what, out, ref, dts)


PAST = [(C, 1) for C in rc.LN_BWD_WIDTHS] + [(320, 64), (320, 256), (768, 64), (64, 256)]


@pytest.mark.parametrize("C,copies", PAST, ids=[f"C{C}-copies{k}" for C, k in PAST])
def test_ln_bwd_past_the_grid_stride_threshold(ops, parity, C, copies):
    """one row more than 256 workgroups x (1024 / G) row groups take in one pass (a natural grid of 257, clipped to 256 or to `copies` = 64): the row loop
    runs again.  copies 1: atomics into one dgamma / dbeta; 64 / 256: a copy per workgroup, plain adds, folded afterwards.  Scaled rows: per-row dx over
    eight decades.  accumulate at every other width."""
    rows = rc.ln_bwd_threshold(C) + 1
    assert rows == {320: 8193, 768: 4097, 64: 32769}.get(C, rows)
    g, _ = rc.ln_params(C)
    dy = torch.randn(rows, C, generator=rc.gen(2))
    base = torch.randn(rows, C, generator=rc.gen(3)) if (C // 8) % 2 else None
    what = f"C{C} rows{rows} copies{copies}{' accumulate' if base is not None else ''}"
    out, ref = run_ln_bwd(ops, what, dy, rc.ln_scaled_rows(rows, C), g, BWD_DT[C], base=base, copies=copies)
    judge_ln_bwd(parity, what, out, ref, BWD_DT[C])


@pytest.mark.parametrize("dts", [(BF, F32, BF), (F32, F32, F32)], ids=["bf16", "fp32"])
@pytest.mark.parametrize("where", ["first", "last", "second_pass", "text_range"])
def test_ln_bwd_single_row_dy(ops, parity, where, dts):
    """dy non-zero in one row: dgamma / dbeta are that row's dy x_hat / dy, every other row's dx is exactly 0 and, with accumulate, keeps its bits"""
    C = 320
    if where == "text_range":                                     # the text rows of a (B, HW + T, C) buffer: dy, x and dx all mapped
        B, HW, T = 3, 20, 7
        rows, row, maps = B * T, T + 2, ((T, HW + T, HW),) * 3
    else:
        rows = rc.ln_bwd_threshold(C) + 40
        row, maps = {"first": 0, "last": rows - 1, "second_pass": rc.ln_bwd_threshold(C)}[where], (None, None, None)
    g, _ = rc.ln_params(C)
    dy, x = rc.ln_single_row_dy(rows, C, row), rc.ln_scaled_rows(rows, C, seed=1)
    others = torch.arange(rows, device=dev()) != row
    for base in (None, torch.randn(rows, C, generator=rc.gen(3))):
        what = f"single-row dy at {where} row {row} of {rows}{' accumulate' if base is not None else ''}"
        out, ref = run_ln_bwd(ops, what, dy, x, g, dts, maps=maps, base=base, copies=64 if where == "second_pass" else 1)
        judge_ln_bwd(parity, what, out, ref, dts)
        exact("dx of the other rows", what, out.dx[others], (base.to(dev()).to(dts[2]) if base is not None else torch.zeros(rows, C, device=dev()))[others])


@pytest.mark.parametrize("dt", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("off,n", [(0, 20), (20, 7)], ids=["image_range", "text_range"])
def test_ln_bwd_scaled_copy_through_row_maps(ops, parity, off, n, dt):
    """dx2 = (dx after accumulation) x scale[sample], scales {0, 1.25, 1}; dy, x and dx in the image / text range of a (B, HW + T, C) buffer"""
    B, C, N = 3, 128, 27
    rows = B * n
    g, _ = rc.ln_params(C)
    dts = (dt, F32, dt)
    base = torch.randn(rows, C, generator=rc.gen(3))
    what = f"dx2 rows {off}..{off + n} of every {N}"
    out, ref = run_ln_bwd(ops, what, torch.randn(rows, C, generator=rc.gen(2)), rc.ln_scaled_rows(rows, C), g, dts, maps=((n, N, off),) * 3, base=base,
                          dx2_scales=[0.0, 1.25, 1.0], rows_per_scale=n)
    judge_ln_bwd(parity, what, out, ref, dts)
    sc = torch.tensor([0.0, 1.25, 1.0], dtype=torch.float64, device=dev()).repeat_interleave(n)[:, None]
    want = ref.dx * sc
    judge(parity, f"ln_bwd dx2 {DT_ID[dt]}", what, out.dx2, want, rc.bar_dx(ref.dx, rc.tol(*dts)) * sc + (rc.bf16_half_ulp(want) if dt == BF else 0.0))
    exact("dx2 of the sample scaled by 0", what, out.dx2[:n], torch.zeros(n, C, device=dev()))


# ================================================================================================ BERT embedding
BERT_CASES = [(T, batch, "mixed") for T, batch in rc.BERT_SHAPES] + [(20, 40, "same"), (200, 33, "same"), (20, 40, "pad"), (1, 5, "pad")]


@pytest.mark.parametrize("dt", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("keep", [False, True], ids=["nodrop", "keep"])
@pytest.mark.parametrize("T,batch,layout", BERT_CASES, ids=[f"T{T}-B{b}-{l}" for T, b, l in BERT_CASES])
def test_bert_embed(ops, parity, T, batch, layout, keep, dt):
    """(20, 40): nsplit = 3; (200, 33): nsplit = 1 and three trips of the batch loop; (512, 2): T > 256; (1, 5): T = 1, rows no multiple of 4.  "same": every
    token one id (all atomics of dword on one row); "pad": dword exactly 0, everything else still right"""
    V, rows, eps, p = 1000, T * batch, 1e-12, 0.1
    tb = rc.bert_tables(V)
    ids = Vec(rows, rc.bert_ids(T, batch, V, layout).reshape(-1), dtype=torch.int64)
    word, pos = Mat(V, rc.HID, F32, tb.word, pad=0), Mat(512, rc.HID, F32, tb.pos, pad=0)
    typ, g, b = Vec(rc.HID, tb.type0), Vec(rc.HID, tb.gamma), Vec(rc.HID, tb.beta)
    kp = Mat(rows, rc.HID, torch.uint8, (torch.rand(rows, rc.HID, generator=rc.gen(8)) >= p), pad=0) if keep else None
    y, mean, rstd = Mat(rows, rc.HID, dt, pad=0, fill=SENTINEL), Vec(rows), Vec(rows)
    what = f"bert T{T} batch{batch} {layout} {'keep' if keep else 'no dropout'}"
    args = (ids.dense(), word.dense(), pos.dense(), typ.dense(), g.dense())
    ops.bert_embed_fwd(ids.t, word.m, pos.m, typ.t, g.t, b.t, kp.t if keep else None, p if keep else 0.0, y.t, mean.t, rstd.t, rows, T, eps)
    ran("bert_embed_fwd_kernel", dt, 768)
    check_all(what + " forward", ids=ids, word=word, pos=pos, type0=typ, gamma=g, beta=b, keep=kp, y=y, mean=mean, rstd=rstd)
    kd = kp.dense() if keep else None
    ref = rc.bert_fwd_ref(*args, b.dense(), eps, T, kd, p if keep else 0.0)
    t = rc.tol(dt)
    plain = rc.ln_fwd_ref(rc.bert_embed_x(*args[:4], T)[0], g.dense(), b.dense(), eps).y
    judge(parity, f"bert_fwd y {DT_ID[dt]}", what, y.dense(), ref.y, rc.bar_y(plain, t) * (1.0 / (1.0 - p) if keep else 1.0))
    judge(parity, f"bert_fwd mean {DT_ID[dt]}", what, mean.dense(), ref.mean, rc.bar_mean(ref, rc.TOL[F32]))
    judge(parity, f"bert_fwd rstd {DT_ID[dt]}", what, rstd.dense(), ref.rstd, rc.TOL[F32] * ref.rstd)
    # backward, handed the fp32-rounded statistics of the reference
    dy = Mat(rows, rc.HID, dt, torch.randn(rows, rc.HID, generator=rc.gen(9)), pad=0)
    mean, rstd = Vec(rows, ref.mean), Vec(rows, ref.rstd)
    dword, dpos = Mat(V, rc.HID, F32, pad=0), Mat(512, rc.HID, F32, pad=0)
    dtyp, dg, db = Vec(rc.HID), Vec(rc.HID), Vec(rc.HID)
    ops.bert_embed_bwd(dy.t, ids.t, word.m, pos.m, typ.t, g.t, kp.t if keep else None, p if keep else 0.0, mean.t, rstd.t, dword.t, dpos.t, dtyp.t, dg.t, db.t, rows, T)
    ran("bert_embed_bwd_kernel", dt, 768, 1024)
    check_all(what + " backward", dy=dy, ids=ids, word=word, pos=pos, type0=typ, gamma=g, keep=kp, mean=mean, rstd=rstd, dword=dword, dpos=dpos, dtype0=dtyp,
              dgamma=dg, dbeta=db)
    r = rc.bert_bwd_ref(dy.dense(), *args, mean.dense(), rstd.dense(), T, kd, p if keep else 0.0)
    tag = DT_ID[dt]
    judge(parity, f"bert_bwd dword {tag}", what, dword.dense(), r.dword, rc.bar_dx(r.dword, t))
    judge(parity, f"bert_bwd dpos {tag}", what, dpos.dense(), r.dpos, rc.bar_dx(r.dpos, t))
    judge(parity, f"bert_bwd dtype0 {tag}", what, dtyp.dense(), r.dtype0, rc.bar_col(r.abs_type0, t))
    judge(parity, f"bert_bwd dgamma {tag}", what, dg.dense(), r.dgamma, rc.bar_col(r.abs_gamma, t))
    judge(parity, f"bert_bwd dbeta {tag}", what, db.dense(), r.dbeta, rc.bar_col(r.abs_beta, t))
    exact("dword of PAD", what, dword.dense()[:1], torch.zeros(1, rc.HID, device=dev()))
    if layout == "pad":
        exact("dword", what, dword.dense(), torch.zeros(V, rc.HID, device=dev()))
        assert float(r.dpos[:T].abs().amax(-1).min()) > 0


# ================================================================================================ cross entropy
def run_ce(ops, parity, what, x, lab, dt, V, ld, *, outs=((F32, 0),), gscale=1.0, loss0=0.0, count0=0.0, count_for_grad=None, byte_offset=0, masked=False):
    """forward, then one backward per (dlogits dtype, ldd - ld) of `outs`, all judged here; -> (loss_sum, count) Vecs for further calls"""
    rows = x.shape[0]
    lg = Mat(rows, V, dt, x, pad=ld - V)
    if byte_offset:                                               # the same matrix 4 bytes into its buffer: off the 16-byte boundary the vector loads need
        assert dt == F32 and byte_offset == 4
        shifted = torch.full((lg.t.numel() + 1,), SENTINEL, dtype=dt, device=dev())
        shifted[1:] = lg.t
        lg.t = shifted[1:]
        lg.m = lg.t[: lg.nphys * lg.ld].view(lg.nphys, lg.ld)
        assert lg.t.data_ptr() % 16 == 4
    labels = Vec(rows, lab, dtype=torch.int64)
    lse, loss, count = Vec(rows), Vec(1, fill=loss0), Vec(1, fill=count0)
    ops.cross_entropy_fwd(lg.t, labels.t, lse.t, loss.t, count.t, rows, V, ld)
    ran("ce_loss_finish_kernel", dt)
    check_all(what + " forward", logits=lg, labels=labels, lse=lse, loss=loss, count=count)
    ref = rc.ce_ref(lg.dense(), labels.dense(), gscale=gscale, count=count_for_grad)
    t, tag = rc.tol(dt), DT_ID[dt]
    judge(parity, f"ce lse {tag}", what, lse.dense(), ref.lse, rc.bar_lse(ref.lse, t))
    n_got, n_want = float(count.dense()[0]), count0 + ref.count
    assert n_got == n_want, f"{what}: count {n_got}, want {n_want}; last kernel {last_kernel()}"
    mean_want = (loss0 + ref.loss_sum) / max(n_want, 1.0)
    judge(parity, f"ce loss mean {tag}", what, loss.dense() / max(n_want, 1.0), torch.tensor([mean_want], dtype=torch.float64, device=dev()),
          t * max(1.0, abs(mean_want)))
    if ref.count == 0:
        exact("loss_sum of an all-ignored batch", what, loss.dense(), torch.tensor([loss0], device=dev()))
    cnt = Vec(1, fill=float(count_for_grad)) if count_for_grad is not None else count
    gs = Vec(1, fill=gscale)
    lse_in = Vec(rows, ref.lse)                                   # the backward reads the reference's lse: judged on its own
    for odt, extra in outs:
        ldd = ld + extra
        dl = Mat(rows, ldd, odt, pad=0, fill=SENTINEL)
        w = f"{what} dlogits {DT_ID[odt]} ldd{ldd}"
        ops.cross_entropy_bwd(lg.t, labels.t, lse_in.t, gs.t, cnt.t, dl.t, rows, V, ld, ldd)
        ran("ce_bwd_kernel", dt, odt)
        check_all(w, logits=lg, labels=labels, lse=lse_in, gscale=gs, count=cnt, dlogits=dl)
        got = dl.dense()
        exact("padding columns [V, ldd)", w, got[:, V:], torch.zeros(rows, ldd - V, device=dev()))
        div = count_for_grad if count_for_grad is not None else n_want
        judge(parity, f"ce dlogits {tag}->{DT_ID[odt]}", w, got[:, :V], ref.dlogits, rc.bar_dlogits(ref.dlogits, rc.tol(dt, odt), gscale, div, odt))
        if masked:
            inf = torch.isinf(lg.dense())
            assert bool((got[:, :V][inf] == 0).all()), f"{w}: a masked column's gradient must be exactly +-0"
        if ref.count == 0:
            exact("dlogits of an all-ignored batch", w, got, torch.zeros(rows, ldd, device=dev()))
    return loss, count


ALL_OUTS = ((F32, 0), (BF, 8), (BF, 0), (F32, 8))
CE_IDS = [f"V{V}-ld{ld}" for V, ld in rc.CE_SHAPES]


@pytest.mark.parametrize("dt", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("V,ld", rc.CE_SHAPES, ids=CE_IDS)
def test_ce_data(ops, parity, V, ld, dt):
    """peaked rows at every place a maximum can arrive late, shifted rows (+-100), flat rows; both dlogits dtypes, ldd = ld and ld + 8"""
    rows = 6
    for peak in rc.CE_PEAKS:
        col = rc.ce_peak_column(peak, V)
        if col is not None:
            x, lab = rc.ce_peaked_rows(rows, V, col)
            run_ce(ops, parity, f"V{V} ld{ld} peak at {peak} = column {col}", x, lab, dt, V, ld, outs=ALL_OUTS if peak in ("V4", 0) else ((BF, 8),))
    for shift in (100.0, -100.0):
        x, lab = rc.ce_shifted_rows(rows, V, shift)
        run_ce(ops, parity, f"V{V} ld{ld} shifted by {shift}", x, lab, dt, V, ld, outs=((F32, 8), (BF, 0)))
    x, lab = rc.ce_flat_rows(rows, V)
    run_ce(ops, parity, f"V{V} ld{ld} flat", x, lab, dt, V, ld, outs=((F32, 0), (BF, 8)))


MASKED = [(V, ld, mode) for V, ld in rc.CE_SHAPES for mode in ("first4", "first8192", "random30")
          if not (mode == "first4" and V <= 4) and not (mode == "first8192" and V <= 8192)]


@pytest.mark.parametrize("dt", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("V,ld,mode", MASKED, ids=[f"V{V}-ld{ld}-{m}" for V, ld, m in MASKED])
def test_ce_masked_rows(ops, parity, V, ld, mode, dt):
    """-inf logits as F.cross_entropy takes them: a row with one finite logit has a finite, correct lse wherever the -inf columns lie, and the masked columns
    get a gradient of exactly +-0.  (A row of nothing but -inf and a label on a -inf column are outside the contract.)"""
    x, lab = rc.ce_masked_rows(6, V, mode)
    run_ce(ops, parity, f"V{V} ld{ld} masked {mode}", x, lab, dt, V, ld, outs=((F32, 0), (BF, 8)), masked=True)


@pytest.mark.parametrize("dt", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("rows", [1, 37, 1025 + 3])
@pytest.mark.parametrize("layout", ["column0", "last_column", "scalar_tail", "all_ignored", "none_ignored", "late_rows"])
def test_ce_rows_and_labels(ops, parity, layout, rows, dt):
    """V = 122 (V4 = 120: columns 120, 121 are the scalar tail), ld = 128.  1028 rows: the finish kernel's `r += 1024` loop; "late_rows": only rows >= 1024
    carry a label there (the last row elsewhere)"""
    V, ld = 122, 128
    x = 3 * torch.randn(rows, V, generator=rc.gen(rows))
    lab = rc.ce_labels(rows, V, seed=rows)
    r = torch.arange(rows)
    if layout == "column0":
        lab[:] = 0
    elif layout == "last_column":
        lab[:] = V - 1
    elif layout == "scalar_tail":
        lab[:] = 120
    elif layout == "all_ignored":
        lab[:] = -1
    elif layout == "late_rows":
        lab[r < min(1024, rows - 1)] = -1
    else:
        assert bool((lab >= 0).all())
    if layout in ("column0", "last_column", "scalar_tail"):
        lab[r % 3 == 1] = -1
    run_ce(ops, parity, f"V{V} rows{rows} labels {layout}", x, lab, dt, V, ld, outs=((F32, 0), (BF, 8)))


@pytest.mark.parametrize("dt", [BF, F32], ids=DT_ID.get)
def test_ce_accumulates_and_takes_a_foreign_count(ops, parity, dt):
    """loss_sum and count are ADDED to: two forwards into the same pair, starting from 3.5 and 2; gscale = 10 over a count of 7 that another call left"""
    V, ld = 123, 125
    xa, la = rc.ce_shifted_rows(37, V, 100.0, seed=1)
    la[::4] = -1
    loss, count = run_ce(ops, parity, "first call", xa, la, dt, V, ld, loss0=3.5, count0=2.0, gscale=10.0, count_for_grad=7, outs=((F32, 0), (BF, 8)))
    first, n1 = float(loss.dense()[0]), float(count.dense()[0])
    xb, lb = rc.ce_peaked_rows(5, V, 122, seed=2)
    lg, labels, lse = Mat(5, V, dt, xb, pad=ld - V), Vec(5, lb, dtype=torch.int64), Vec(5)
    ops.cross_entropy_fwd(lg.t, labels.t, lse.t, loss.t, count.t, 5, V, ld)
    check_all("second call", logits=lg, labels=labels, lse=lse, loss=loss, count=count)
    ref = rc.ce_ref(lg.dense(), labels.dense())
    assert float(count.dense()[0]) == n1 + 5
    want = first + ref.loss_sum
    judge(parity, f"ce loss mean {DT_ID[dt]}", "second call", loss.dense() / (n1 + 5), torch.tensor([want / (n1 + 5)], dtype=torch.float64, device=dev()),
          rc.tol(dt) * max(1.0, abs(want / (n1 + 5))))


@pytest.mark.parametrize("V,ld", [(122, 128), (8195, 8196)])
def test_ce_view_off_the_16_byte_boundary(ops, parity, V, ld):
    """fp32 logits that start 4 bytes into their buffer: ld is a multiple of 4, the base pointer is not 16-byte aligned -- the scalar fallback of both kernels"""
    x, lab = rc.ce_peaked_rows(6, V, V - 1)
    run_ce(ops, parity, f"V{V} ld{ld} view at +4 bytes", x, lab, F32, V, ld, outs=ALL_OUTS, byte_offset=4)


# ================================================================================================ SmoothL1
def run_sl1(ops, what, pred, target, gscale, loss0):
    n = pred.numel()
    p, t = Vec(n, pred), Vec(n, target)
    loss, gs, grad = Vec(1, fill=loss0), Vec(1, fill=gscale), Vec(n, fill=SENTINEL)
    ops.smooth_l1_fwd(p.t[:n], t.t[:n], loss.t)
    ran("smooth_l1_sum_kernel")
    ops.smooth_l1_bwd(p.t[:n], t.t[:n], gs.t, grad.t[:n])
    ran("smooth_l1_grad_kernel")
    check_all(what, pred=p, target=t, loss=loss, gscale=gs, grad=grad)
    return p, t, loss.dense(), grad.dense()


def test_smooth_l1_exact(ops):
    """7 x 2^20 + 148 elements (the 4x-unrolled main loop, its tail loop and a ragged last pass), differences on halves: every partial sum is exact in fp32 in
    any order, so loss_sum -- added to 1024.5 -- must be bit-equal; the gradient bit-equal to clamp(d, -1, 1) x (gscale x float32(1 / n)) in fp32"""
    pred, target = rc.sl1_exact()
    gscale = 10.0
    p, t, loss, grad = run_sl1(ops, "sl1 exact", pred, target, gscale, 1024.5)
    want = rc.sl1_ref(pred, target).loss_sum + 1024.5
    assert float(loss[0]) == want, f"loss_sum {float(loss[0])!r}, want {want!r} exactly"
    one, n = torch.tensor(1.0, device=dev()), torch.tensor(float(rc.SL1_N), device=dev())
    sc = torch.tensor(gscale, device=dev()) * (one / n)
    exact("grad", "sl1 exact", grad, (p.dense() - t.dense()).clamp(-1, 1) * sc)


@pytest.mark.parametrize("d", rc.sl1_boundary_values(), ids=lambda d: repr(d))
def test_smooth_l1_boundaries(ops, parity, d):
    """one difference in an all-equal pair: |d| = 1 from both sides, signed zeros, 1e30, a denormal.  Bars from the number format: the loss is two fp32 roundings
    (2^-22 relative) and the denormal difference may be flushed (2^-126 absolute)"""
    pred, target = rc.sl1_boundaries(d)
    p, t, loss, grad = run_sl1(ops, f"sl1 d = {d!r}", pred, target, 2.0, 0.0)
    ref = rc.sl1_ref(p.dense(), t.dense(), gscale=2.0)
    want = torch.tensor([ref.loss_sum], dtype=torch.float64, device=dev())
    judge(parity, "sl1 loss_sum", f"d = {d!r}", loss, want, 2.0 ** -22 * want.abs() + 2.0 ** -126)
    judge(parity, "sl1 grad", f"d = {d!r}", grad, ref.grad, 2.0 ** -22 * ref.grad.abs() + 2.0 ** -126)
    if abs(d) == 1.0:
        assert float(loss[0]) == 0.5


def test_smooth_l1_refuses_a_ragged_length(ops):
    p, t = torch.zeros(8, device=dev()), torch.ones(8, device=dev())
    loss, gs, grad = Vec(1, fill=SENTINEL), Vec(1, fill=1.0), Vec(8, fill=SENTINEL)
    refused(lambda: ops.smooth_l1_fwd(p[:6], t[:6], loss.t), loss.t)
    refused(lambda: ops.smooth_l1_bwd(p[:6], t[:6], gs.t, grad.t[:6]), grad.t)

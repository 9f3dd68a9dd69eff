"""GPU: the kernels of csrc/mim.hip -- the MIM decoder's train-mode BatchNorm, the align_corners=True bilinear resizes and their adjoints, the fused
upsample + SmoothL1 loss and the feature products -- on inputs built to make one wrong formula, one dropped row or one lost tap an error of many bars,
through every instantiation the host functions can launch, against the float64 references of tests/mim_cases.py (premises pinned on the CPU by
tests/test_mim_cases_cpu.py; docs/mim_edges.md has the tables).

Bars: the project's 1e-3 (fp32) / 2e-2 (bf16), an fp16 output 1e-3 + 2^-11 -- the narrowest dtype a case WRITES decides --, applied
  per row         y, dz, resize outputs (t x max |ref| over the row, resizes plus the fp32-coordinate slack of mim_cases.resize_ref)
  per column      s1, s2, sum, sumsq, g_beta, g_gamma against the column's sum of absolute terms; mean against max(|mean|, std); rstd relative
  per element     the adjoints, against |U|^T |g| |U|
never against one global maximum.  Where the input makes the answer exact (integer sums, products, single-row dy, `+=` of integer sums, a narrow-dtype
launch against the fp32 launch on the rounded operands, fused against unfused finalize) the check is bit equality.
A failure prints the case, the instantiation (mvlt_amd._lib.last_kernel()), row, column, the value got and the value wanted.

EVERY launch goes through the wrappers below: operands and results live in flat buffers filled with the sentinel 7.0, leading dimensions are larger than C
(multiples of 8 where the wide paths need that), one guard row sits behind every matrix and one guard element behind every vector; after the launch every
sentinel must be bit-identical (integer view).
"""
import math

import numpy as np
import pytest
import torch

from tests import mim_cases as mc

pytestmark = pytest.mark.gpu

BF, F32, F16 = mc.BF, mc.F32, mc.F16
DT_ID = {BF: "bf16", F32: "fp32", F16: "fp16"}
SENTINEL = 7.0
INT_VIEW = {BF: torch.int16, F16: torch.int16, F32: torch.int32}
EPS, MOM = mc.EPS, mc.MOMENTUM


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


def ran(base, targs=()):
    """the kernel launched last on this thread must be the instantiation base<targs>.  The C++ runtime's demangler gives up on names that hold the bf16 or
    fp16 element types (template arguments or parameters): those come back mangled, and the template arguments are looked up in the mangled form"""
    name = last_kernel()
    enc = lambda t: "DF16b" if t is BF else "DF16_" if t is F16 else "f" if t is F32 else f"Li{t}E"
    txt = lambda t: "float" if t is F32 else "_Float16" if t is F16 else "__bf16" if t is BF else str(t)
    if name.startswith("_Z"):
        want = f"{len(base)}{base}" + ("I" + "".join(enc(t) for t in targs) + "E" if targs else "E")
        assert want in name, f"meant to reach {base}{targs} ({want}), the library launched {name}"
    else:
        # (a demangler that reads the bf16 code "DF16b" as a fixed-point type swallows the character behind it: <bf16, float, ...> comes back as <bool _Accum, ...>)
        quirk, i = [], 0
        while i < len(targs):
            pair = targs[i] is BF and i + 1 < len(targs) and targs[i + 1] is F32
            quirk.append("bool _Accum" if pair else txt(targs[i]))
            i += 2 if pair else 1
        want = {base + ("<" + ", ".join(p) + ">" if targs else "") for p in ([txt(t) for t in targs], quirk)}
        assert name in want, f"meant to reach {sorted(want)}, the library launched {name}"


# ------------------------------------------------------------------------------------------------ buffers and guards
def sentinels_intact(flat, dead, dtype, what):
    got = flat.view(INT_VIEW[dtype])[dead]
    want = torch.tensor([SENTINEL], dtype=dtype).view(INT_VIEW[dtype]).to(flat.device)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {got.numel()} sentinels overwritten; first at flat element "
                              f"{int(dead.nonzero()[bad[0, 0], 0])} of {dead.numel()}; last kernel {last_kernel()}")


class Mat:
    """[rows, C] at the columns [off, off + C) of rows `ld` apart inside a flat device buffer of sentinels that starts `base` elements in, one guard row
    behind the last row.  `.p` is what a kernel is handed (the address of element (0, off))"""

    def __init__(self, rows, C, dtype, dense=None, fill=0.0, ld=None, off=0, base=0):
        self.rows, self.C, self.ld, self.off, self.base, self.dtype = rows, C, ld or C + 8, off, base, dtype
        assert off + C <= self.ld
        self.t = torch.full((base + (rows + 1) * self.ld,), SENTINEL, dtype=dtype, device=dev())
        self.m = self.t[base: base + rows * self.ld].view(rows, self.ld)
        self.m[:, off:off + C] = dense.to(device=dev(), dtype=dtype).reshape(rows, C) if dense is not None else fill
        self.p = self.t[base + off:]

    def dense(self):
        return self.m[:, self.off:self.off + self.C]

    def check(self, what):
        dead = torch.ones_like(self.t, dtype=torch.bool)
        dead[self.base: self.base + self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.C] = False
        sentinels_intact(self.t, dead, self.dtype, what)


class Vec:
    """n live elements and one guard element behind them"""

    def __init__(self, n, dense=None, fill=0.0, dtype=F32):
        self.n, self.dtype = n, dtype
        self.t = torch.full((n + 1,), SENTINEL, dtype=dtype, device=dev())
        self.t[:n] = dense.to(device=dev(), dtype=dtype).reshape(-1) if dense is not None else fill

    def dense(self):
        return self.t[: self.n]

    def check(self, what):
        sentinels_intact(self.t[self.n:], torch.ones(1, dtype=torch.bool, device=dev()), self.dtype, what)


def check_all(what, *bufs):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        if b is not None:
            b.check(f"{what}, buffer {i}")


# ------------------------------------------------------------------------------------------------ judging
FAILED = []      # the comparisons of the running test that missed: a test walks ALL its cases and reports every miss at its end


@pytest.fixture(autouse=True)
def every_case_is_reported():
    FAILED.clear()
    yield
    assert not FAILED, f"{len(FAILED)} comparisons missed:\n" + "\n".join(FAILED[:40])


def judge(parity, name, what, got, ref, bar):
    """|got - ref| <= bar element by element (bar broadcasts: per row, per column or per element); records the worst error / bar"""
    got, ref = got.double(), ref.double().to(got.device)
    bar = torch.as_tensor(bar, dtype=torch.float64, device=got.device)
    if got.dim() == 1:
        got, ref, bar = got[None], ref[None], (bar[None] if bar.dim() == 1 else bar)
    bar = bar.expand_as(got).reshape(-1, got.shape[-1])
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, got.shape[-1])
    if got.numel() == 0:
        return
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, math.inf))
    i = int(ratio.argmax())
    r, c = i // got.shape[1], i % got.shape[1]
    print(f"{name:34s} {what:46s} worst {float(ratio.max()):9.3e} bars")
    if not parity(f"{name}/{what}", ratio.max(), 1.0):
        FAILED.append(f"{what}: {name} row {r} column {c}: got {float(got[r, c])!r}, want {float(ref[r, c])!r}, bar {float(bar[r, c]):.3e} "
                      f"({float(ratio[r, c]):.3g} bars); last kernel {last_kernel()}")


def exact(name, what, got, want):
    want = want.to(device=got.device)
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, got.shape[-1])
    same = got.double() == want.double() if want.dtype != got.dtype else got == want
    if not bool(same.all()):
        bad = (~same).nonzero()
        r, c = int(bad[0, 0]), int(bad[0, 1])
        FAILED.append(f"{what}: {name} must be exact; {bad.shape[0]} elements differ, first at row {r} column {c}: got {float(got[r, c])!r}, "
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
        assert bool((t.float() == SENTINEL).all())


# ================================================================================================ BatchNorm statistics and finalize
def run_stats(ops, what, z, ld=None, base=0):
    M, C = z.shape
    zb = Mat(M, C, F32, z, ld=ld, base=base)
    s1, s2 = Vec(C), Vec(C)
    ops.col_stats(zb.p, zb.ld, M, C, s1.t, s2.t)
    ran(*mc.stats_kernel(C, zb.ld, 4 * base))
    check_all(what, zb, s1, s2)
    return zb, s1, s2


def run_finalize(ops, what, s1, s2, M, C, copies=1):
    """-> dense (mean, rstd, running_mean, running_var) and the starting running statistics"""
    rm0, rv0 = torch.linspace(-1.0, 1.0, C), torch.linspace(0.5, 2.0, C)
    mean, rstd, rm, rv = Vec(C), Vec(C), Vec(C, rm0), Vec(C, rv0)
    ops.bn_finalize(s1, s2, M, C, EPS, MOM, mean.t, rstd.t, rm.t, rv.t, copies=copies)
    ran("bn_finalize_kernel")
    check_all(what, mean, rstd, rm, rv)
    return (mean.dense(), rstd.dense(), rm.dense(), rv.dense()), (rm0.to(dev()), rv0.to(dev()))


def judge_stats(parity, what, out, start, ref, t=mc.TOL[F32], tag="bn_finalize"):
    mean, rstd, rm, rv = out
    std = ref.var.sqrt()
    rm_ref, rv_ref = mc.bn_running_ref(start[0], start[1], ref.mean, ref.var, ref.M)
    judge(parity, f"{tag} mean", what, mean, ref.mean, t * torch.maximum(ref.mean.abs(), std).clamp_min(1e-30))
    judge(parity, f"{tag} rstd", what, rstd, ref.rstd, t * ref.rstd)
    judge(parity, f"{tag} running_mean", what, rm, rm_ref, t * ((1 - MOM) * start[0].abs() + MOM * torch.maximum(ref.mean.abs(), std)).clamp_min(1e-30))
    judge(parity, f"{tag} running_var", what, rv, rv_ref, t * rv_ref)


def test_col_stats_and_finalize(ops, parity):
    """col_reduce4_kernel<0, 1024> at every width class, col_reduce_kernel<0> by C % 4 and by a misaligned base, each at M = 1, 3, rpp - 1, rows_per_wg -+ 1
    and 4096; bn_finalize_kernel on the sums: mean bit-equal to fl(s1 / M) on integer data, rstd within the one-pass bound, the running statistics against
    nn.BatchNorm2d's rule (unbiased variance, its M > 1 guard at M = 1) from non-trivial starting values"""
    shapes = [(C, C + 8, 0) for C in mc.STATS_WIDTHS] + list(mc.STATS_SCALAR)
    for C, ld, base in shapes:
        for M in mc.stats_row_counts(C if C % 4 == 0 else 64):
            for builder in ("integer", "constant", "offset", "scaled"):
                if builder != "integer" and M < 3:
                    continue        # one row has no variance: only integer data (m m and s2 exact) is inside the one-pass contract there
                z = {"integer": mc.bn_integer_columns, "constant": mc.bn_constant_columns, "offset": mc.bn_offset_columns,
                     "scaled": mc.bn_scaled_columns}[builder](M, C, seed=M)
                what = f"{builder} M {M} C {C} ld {ld} base {base}"
                zb, s1, s2 = run_stats(ops, what, z, ld, base)
                ref = mc.bn_stats_ref(zb.dense())
                if builder in ("integer", "offset"):
                    exact("col_stats sum", what, s1.dense(), ref.s1)
                    exact("col_stats sumsq", what, s2.dense(), ref.s2)
                else:
                    judge(parity, "col_stats sum", what, s1.dense(), ref.s1, mc.bar_cols(ref.abs1, mc.TOL[F32]))
                    judge(parity, "col_stats sumsq", what, s2.dense(), ref.s2, mc.bar_cols(ref.s2, mc.TOL[F32]))
                out, start = run_finalize(ops, what, s1.t, s2.t, M, C)
                judge_stats(parity, what, out, start, ref)
                if builder == "integer":
                    want = (s1.dense().cpu().numpy() / np.float32(M)).astype(np.float32)
                    exact("bn_finalize mean = fl(s1 / M)", what, out[0], torch.from_numpy(want))
                    # var = s2 / M - m m from exact sums: two roundings of s2 / M and m m (each half an ulp of its value), one of the difference; rsqrt 2 ulp
                    ex2 = ref.s2 / M + ref.mean ** 2
                    judge(parity, "bn_finalize rstd (integer)", what, out[1], ref.rstd, ref.rstd * (0.5 * 4 * 2.0 ** -24 * ex2 / (ref.var + EPS) + 4 * 2.0 ** -24))
                    ops.col_stats(zb.p, zb.ld, M, C, s1.t, s2.t)             # the sums ACCUMULATE: a second launch doubles them exactly
                    check_all(what, zb, s1, s2)
                    exact("col_stats sum, second launch", what, s1.dense(), 2 * ref.s1)
                    exact("col_stats sumsq, second launch", what, s2.dense(), 2 * ref.s2)
                if builder == "constant":
                    k = min(len(mc.CONSTANTS), C)
                    judge(parity, "bn_finalize rstd (constant)", what, out[1][:k], torch.full((k,), 1.0 / math.sqrt(mc.f32(EPS)), dtype=torch.float64),
                          mc.TOL[F32] / math.sqrt(mc.f32(EPS)))


def parts_of(zf, copies):
    """the conv epilogue's interleaved accumulators: row tile t adds into copy t % copies"""
    C = zf.shape[1]
    parts = torch.zeros(2, copies, C, device=dev())
    for k in range(copies):
        rows = zf[k::copies].double()
        parts[0, k], parts[1, k] = rows.sum(0).float(), (rows * rows).sum(0).float()
    return parts


@pytest.mark.parametrize("ydt", [F32, F16], ids=["y-fp32", "y-fp16"])
def test_finalize_inside_the_normalise_launch(ops, parity, ydt):
    """bn_fin_norm8_kernel<float | _Float16> with copies 1, 4, 16 against bn_finalize_kernel + bn_norm8_kernel bit for bit, and both against float64: the
    statistics, the running statistics (M = 1 included), y (constant columns: beta), with y16 a column range of a wider matrix and ld32 != ld16"""
    for C, M, copies, builder in ((8, 1, 1, "integer"), (8, 3, 4, "integer"), (64, 300, 16, "constant"), (192, 257, 4, "offset"), (256, 4096, 16, "integer"),
                                  (64, 4096, 1, "offset"), (128, 77, 4, "constant")):
        z = {"integer": mc.bn_integer_columns, "constant": mc.bn_constant_columns, "offset": mc.bn_offset_columns}[builder](M, C, seed=copies)
        what = f"{builder} M {M} C {C} copies {copies} y {DT_ID[ydt]}"
        g = torch.randn(C, generator=mc.gen(1)) * 0.5 + 1.0
        b = torch.randn(C, generator=mc.gen(2))
        gamma, beta = Vec(C, g), Vec(C, b)
        outs = []
        for fused in (False, True):
            zb = Mat(M, C, F16, z, ld=C + 8)
            parts = parts_of(zb.dense().float(), copies)
            rm0, rv0 = torch.linspace(-1.0, 1.0, C), torch.linspace(0.5, 2.0, C)
            mean, rstd, rm, rv = Vec(C), Vec(C), Vec(C, rm0), Vec(C, rv0)
            y32, y16 = Mat(M, C, ydt, ld=C + 16), Mat(M, C, BF, ld=2 * C + 8, off=C)
            if fused:
                ops.bn_finalize_norm(zb.p, zb.ld, parts[0], parts[1], copies, EPS, MOM, mean.t, rstd.t, rm.t, rv.t, gamma.t, beta.t, M, C,
                                     y32=y32.p, ld32=y32.ld, y16=y16.p, ld16=y16.ld)
                ran("bn_fin_norm8_kernel", (ydt,))
            else:
                ops.bn_finalize(parts[0], parts[1], M, C, EPS, MOM, mean.t, rstd.t, rm.t, rv.t, copies=copies)
                ran("bn_finalize_kernel")
                ops.bn_norm(zb.p, zb.ld, mean.t, rstd.t, gamma.t, beta.t, M, C, y32=y32.p, ld32=y32.ld, y16=y16.p, ld16=y16.ld)
                ran("bn_norm8_kernel", (ydt,))
            check_all(what, zb, mean, rstd, rm, rv, y32, y16, gamma, beta)
            outs.append((mean.dense(), rstd.dense(), rm.dense(), rv.dense(), y32.dense(), y16.dense()))
        for name, a, bb in zip(("mean", "rstd", "running_mean", "running_var", "y32", "y16"), *outs):
            exact(f"fused {name} == unfused", what, bb, a)
        ref = mc.bn_stats_ref(zb.dense())
        judge_stats(parity, what, outs[1][:4], (rm0.to(dev()), rv0.to(dev())), ref, tag="bn_fin_norm8")
        yref = mc.bn_norm_ref(zb.dense(), ref.mean, ref.rstd, gamma.dense(), beta.dense())
        judge(parity, f"bn_fin_norm8 y {DT_ID[ydt]}", what, outs[1][4], yref, mc.bar_rows(yref, mc.tol(ydt)))
        judge(parity, "bn_fin_norm8 y16", what, outs[1][5], yref, mc.bar_rows(yref, mc.TOL[BF]))
        if builder == "constant":
            judge(parity, "bn_fin_norm8 y (constant) = beta", what, outs[1][4][:, :4], beta.dense()[:4].double().expand(M, 4), mc.bar_rows(yref, mc.tol(ydt)))


# ================================================================================================ normalise
def shifted_columns(M, C, seed=0):
    """N(0,1) with a mean and a scale of its own per column: a kernel that takes a neighbour column's statistics is off by whole sigmas"""
    c = torch.arange(C)
    return torch.randn(M, C, generator=mc.gen(800 + seed)) * (1.0 + 0.5 * (c % 3)) + (c % 5 - 2.0)


NORM_CASES = (  # C, z dtype, y32 dtype, y16 dtype
    (64, F32, F32, F32), (12, F32, F32, BF), (12, F16, F32, BF), (4, F16, F32, BF), (64, F16, F32, BF), (64, F16, F16, BF), (8, F16, F16, BF))


def test_bn_norm_every_instantiation(ops, parity):
    """bn_norm_kernel<float>, <bf16>, <bf16, _Float16> (C % 8 != 0), bn_norm8_kernel<float>, <_Float16>: y32 only, y16 only, both; ld32 != ld16 and y16 a
    column range of a wider matrix; one row, and several workgroups"""
    for C, zdt, y32dt, y16dt in NORM_CASES:
        for M in (1, 37, 1031):
            z = shifted_columns(M + 2, C)[:M] if M > 1 else shifted_columns(1, C)
            stat = mc.bn_stats_ref(shifted_columns(64, C).to(zdt))
            for which in ("y32", "y16", "both"):
                what = f"C {C} M {M} z {DT_ID[zdt]} {which} ({DT_ID[y32dt]}, {DT_ID[y16dt]})"
                zb = Mat(M, C, zdt, z, ld=C + 8)
                mean, rstd = Vec(C, stat.mean), Vec(C, stat.rstd)
                gamma, beta = Vec(C, torch.linspace(0.5, 1.5, C)), Vec(C, torch.linspace(-1.0, 1.0, C))
                y32 = Mat(M, C, y32dt, ld=C + 16) if which != "y16" else None
                y16 = Mat(M, C, y16dt, ld=2 * C + 8, off=8) if which != "y32" else None
                ops.bn_norm(zb.p, zb.ld, mean.t, rstd.t, gamma.t, beta.t, M, C, y32=y32.p if y32 else None, ld32=y32.ld if y32 else 0,
                            y16=y16.p if y16 else None, ld16=y16.ld if y16 else 0)
                ran(*mc.norm_kernel(C, zb.ld, zdt, y32dt if y32 else None, y32.ld if y32 else 0, y16dt if y16 else None, y16.ld if y16 else 0))
                check_all(what, zb, mean, rstd, gamma, beta, y32, y16)
                yref = mc.bn_norm_ref(zb.dense(), mean.dense(), rstd.dense(), gamma.dense(), beta.dense())
                if y32:
                    judge(parity, f"bn_norm y32 {DT_ID[y32dt]}", what, y32.dense(), yref, mc.bar_rows(yref, mc.tol(y32dt)))
                if y16:
                    judge(parity, f"bn_norm y16 {DT_ID[y16dt]}", what, y16.dense(), yref, mc.bar_rows(yref, mc.tol(y16dt)))


# ================================================================================================ backward reduce
RED_CASES = ([(32, dy, z) for dy in (BF, F32) for z in (F16, F32)] + [(100, dy, z) for dy in (BF, F32) for z in (F16, F32)] +
             [(C, dy, F16) for C, _ in mc.RED8 for dy in (BF, F32)] + [(6, F32, F32)])


def test_bn_bwd_reduce_every_instantiation(ops, parity):
    """col_reduce_kernel<1>, col_reduce4_kernel<1, 512 | 1024, TDY, TZ> for the four (TDY, TZ), col_reduce8_kernel<512 | 768 | 1024, bf16 | float> at C = 64, 192,
    128, 256; dy a column range at a non-zero offset; two workgroups with one row in the second.  Single-row dy at the seams (s1 exact), then random dy over
    columns scaled 1e-3 .. 1e3 (per-column bars)"""
    for C, dydt, zdt in RED_CASES:
        lddy, off, ldz = (2 * C + 8, C, C + 8) if C % 4 == 0 else (2 * C + 1, C, C + 1)
        kern = mc.bwd_reduce_kernel(C, lddy, ldz, dydt, zdt, dy_off=off * (2 if dydt is BF else 4))
        if kern[0] == "col_reduce8_kernel":
            rpp, rows_per_wg, _ = mc.red8_rows(1, C, kern[2])
        elif kern[0] == "col_reduce4_kernel":
            rows_per_wg = mc.reduce_rows_per_wg(1, C, kern[2])
        else:
            rows_per_wg = 64
        M = rows_per_wg + 1
        z = mc.bn_scaled_columns(M, C, seed=C)
        zb = Mat(M, C, zdt, z, ld=ldz)
        stat = mc.bn_stats_ref(zb.dense())
        mean, rstd = Vec(C, stat.mean), Vec(C, stat.rstd)
        cases = [(f"single row {r}", mc.bn_single_row_dy(M, C, r, seed=r)) for r in mc.seam_rows(M, rows_per_wg)]
        cases.append(("random", torch.randn(M, C, generator=mc.gen(C))))
        for label, dy in cases:
            what = f"{label} M {M} C {C} dy {DT_ID[dydt]} z {DT_ID[zdt]}"
            dyb = Mat(M, C, dydt, dy, ld=lddy, off=off)
            s1, s2 = Vec(C), Vec(C)
            ops.bn_bwd_reduce(dyb.p, dyb.ld, zb.p, zb.ld, mean.t, rstd.t, M, C, s1.t, s2.t)
            ran(*kern[:2])
            check_all(what, dyb, zb, mean, rstd, s1, s2)
            ref = mc.bn_bwd_sums_ref(dyb.dense(), zb.dense(), mean.dense(), rstd.dense())
            if label != "random":
                exact("bn_bwd_reduce s1", what, s1.dense(), ref.s1)
            judge(parity, "bn_bwd_reduce s1", what, s1.dense(), ref.s1, mc.bar_cols(ref.abs1, mc.TOL[F32]))
            judge(parity, "bn_bwd_reduce s2", what, s2.dense(), ref.s2, mc.bar_cols(ref.abs2, mc.TOL[F32]))


# ================================================================================================ backward apply
APPLY_CASES = (  # C, dy dtype, z dtype, dz dtype
    (64, BF, F16, BF), (64, F32, F16, BF), (12, BF, F16, BF), (12, F32, F16, BF), (64, BF, F32, BF), (64, F32, F32, BF), (12, BF, F32, F32), (64, F32, F32, F32))


def test_bn_bwd_apply_every_instantiation(ops, parity):
    """all eight instantiations, several workgroups, g_beta / g_gamma starting from non-zero values: `+=` of the (integer-valued) sums exactly once -- one
    writer --, dz per row against float64; shifted columns, then constant columns (x_hat ~ 0, rstd = 1 / sqrt(eps): dz finite and within bar)"""
    seen = set()
    for C, dydt, zdt, dzdt in APPLY_CASES:
        for builder, M in (("shifted", 301), ("constant", 301), ("shifted", 1)):
            z = shifted_columns(M, C) if builder == "shifted" else mc.bn_constant_columns(M, C)
            what = f"{builder} M {M} C {C} dy {DT_ID[dydt]} z {DT_ID[zdt]} dz {DT_ID[dzdt]}"
            zb = Mat(M, C, zdt, z, ld=C + 8)
            dyb = Mat(M, C, dydt, torch.randn(M, C, generator=mc.gen(C + M)), ld=2 * C + 8, off=8)
            if M > 1:
                stat = mc.bn_stats_ref(zb.dense())
                mu, rs = stat.mean, stat.rstd
            else:
                mu, rs = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
            mean, rstd, gamma = Vec(C, mu), Vec(C, rs), Vec(C, torch.linspace(0.5, 1.5, C))
            s1v = torch.randint(-9, 10, (C,), generator=mc.gen(1)).float()
            s2v = torch.randint(-9, 10, (C,), generator=mc.gen(2)).float() + 20.0          # never equal to s1: a swap shows
            s1, s2 = Vec(C, s1v), Vec(C, s2v)
            gb0, gg0 = torch.arange(C).float() + 1.0, -torch.arange(C).float() - 3.0
            gb, gg = Vec(C, gb0), Vec(C, gg0)
            dz = Mat(M, C, dzdt, ld=C + 16)
            ops.bn_bwd_apply(dyb.p, dyb.ld, zb.p, zb.ld, mean.t, rstd.t, gamma.t, s1.t, s2.t, M, C, dz.p, dz.ld, g_beta=gb.t, g_gamma=gg.t)
            kern = mc.apply_kernel(C, dyb.ld, zb.ld, dz.ld, dydt, zdt, dzdt)
            ran(*kern[:2])
            seen.add(kern[:2])
            if M > 1:
                assert mc.grid_for(M * (C // kern[2])) > 1, "one writer needs more than one workgroup"
            check_all(what, dyb, zb, mean, rstd, gamma, s1, s2, gb, gg, dz)
            exact("bn_bwd_apply g_beta += s1 once", what, gb.dense(), gb0 + s1v)
            exact("bn_bwd_apply g_gamma += s2 once", what, gg.dense(), gg0 + s2v)
            ref = mc.bn_dz_ref(dyb.dense(), zb.dense(), mean.dense(), rstd.dense(), gamma.dense(), s1.dense(), s2.dense())
            judge(parity, f"bn_bwd_apply dz {DT_ID[dzdt]}", what, dz.dense(), ref, mc.bar_rows(ref, mc.tol(dzdt)))
            # without the parameter gradients: the same dz bit for bit, nothing else written
            dz2 = Mat(M, C, dzdt, ld=C + 16)
            ops.bn_bwd_apply(dyb.p, dyb.ld, zb.p, zb.ld, mean.t, rstd.t, gamma.t, s1.t, s2.t, M, C, dz2.p, dz2.ld)
            check_all(what, dz2, gb, gg)
            exact("bn_bwd_apply dz without g_beta", what, dz2.dense(), dz.dense())
    assert seen == set(mc.APPLY_ALL)


# ================================================================================================ products
def test_ew_mul_exact(ops):
    """ew_mul_kernel<float>, <bf16>, <bf16, _Float16>: two and three factors, accumulate on and off, out only / out16 only / both, strided factors
    (lda = 2 C, as the decoder's halves of a concat), out16 a column range -- all bit-equal to the integer reference"""
    C = 12
    for idt, odt in ((F32, F32), (F32, BF), (F16, BF)):
        for M in (1, 700):
            for nfac in (2, 3):
                for acc in (False, True):
                    for which in ("out", "out16", "both"):
                        if acc and which == "out16":
                            continue
                        what = f"M {M} in {DT_ID[idt]} out16 {DT_ID[odt]} factors {nfac} accumulate {acc} {which}"
                        fac = mc.product_integers(M, C, nfac + 1, seed=nfac)
                        a = Mat(M, C, idt, fac[0], ld=2 * C, off=C)
                        b = Mat(M, C, idt, fac[1], ld=C + 4)
                        c3 = Mat(M, C, idt, fac[2], ld=2 * C + 8, off=4) if nfac == 3 else None
                        out = Mat(M, C, F32, fac[nfac], ld=C + 8) if which != "out16" else None
                        o16 = Mat(M, C, odt, ld=3 * C, off=C) if which != "out" else None
                        ops.ew_mul(out.p if out else None, out.ld if out else 0, a.p, a.ld, b.p, b.ld, c3.p if c3 else None, c3.ld if c3 else 0, M=M, Cdim=C,
                                   accumulate=acc, out16=o16.p if o16 else None, ld16=o16.ld if o16 else 0)
                        ran("ew_mul_kernel", (BF if (o16 is None or odt is BF) else F32, idt))
                        check_all(what, a, b, c3, out, o16)
                        want = fac[0] * fac[1] * (fac[2] if nfac == 3 else 1.0) + (fac[nfac] if acc else 0.0)
                        if out:
                            exact("ew_mul out", what, out.dense(), want)
                        if o16:
                            exact("ew_mul out16", what, o16.dense(), want)


def test_ew_mul3_bwd_exact(ops):
    """ew_mul3_bwd_kernel<float, float>, <bf16, bf16>, <bf16, bf16, _Float16>: dy a column range at an offset; da, db, dc bit-equal to the integer products"""
    C, ld = 12, 20
    for dydt, idt in ((F32, F32), (BF, F32), (BF, F16)):
        for M in (1, 700):
            what = f"M {M} dy {DT_ID[dydt]} factors {DT_ID[idt]}"
            g, fa, fb, fc = mc.product_integers(M, C, 4, seed=M)
            dy = Mat(M, C, dydt, g, ld=3 * C, off=C)
            a, b, c = (Mat(M, C, idt, f, ld=ld) for f in (fa, fb, fc))
            da, db, dc = (Mat(M, C, dydt, ld=ld) for _ in range(3))
            ops.ew_mul3_bwd(dy.p, dy.ld, a.p, b.p, c.p, ld, da.p, db.p, dc.p, M, C)
            ran("ew_mul3_bwd_kernel", (dydt, dydt, idt))
            check_all(what, dy, a, b, c, da, db, dc)
            exact("ew_mul3_bwd da", what, da.dense(), g * fb * fc)
            exact("ew_mul3_bwd db", what, db.dense(), g * fa * fc)
            exact("ew_mul3_bwd dc", what, dc.dense(), g * fa * fb)


# ================================================================================================ resize forward and adjoint
def batch_of_inputs(H, W, C, seed=0):
    """one image per builder: a delta at every corner / border / interior point, the ramp, N(0,1)"""
    xs = [mc.resize_delta(1, H, W, C, iy, ix) for iy, ix in mc.delta_points(H, W)]
    xs += [mc.resize_ramp(1, H, W, C), mc.resize_random(1, H, W, C, seed)]
    return torch.cat(xs)


def batch_of_gradients(Ho, Wo, C, seed=0):
    gs = [mc.resize_delta_out(1, Ho, Wo, C, oy, ox) for oy, ox in mc.delta_points(Ho, Wo)]
    gs += [mc.resize_ramp(1, Ho, Wo, C, 1, 1, 1), mc.resize_random(1, Ho, Wo, C, seed)]
    return torch.cat(gs)


def run_resize_fwd(ops, parity, x, s, odt, nchw=False, ldx=None, ldo=None):
    B, H, W, C = x.shape
    Ho, Wo = H * s, W * s
    what = f"B {B} {H}x{W} C {C} s {s} {'nchw' if nchw else 'pixel-major'} {DT_ID[odt]}"
    xb = Mat(B * H * W, C, F32, x, ld=ldx)
    if nchw:
        ob = Vec(B * C * Ho * Wo)
        ops.upsample_fwd(xb.p, xb.ld, B, H, W, C, s, ob.t, 0, nchw=True)
        got = ob.dense().view(B, C, Ho, Wo).permute(0, 2, 3, 1)
    else:
        ob = Mat(B * Ho * Wo, C, odt, ld=ldo)
        ops.upsample_fwd(xb.p, xb.ld, B, H, W, C, s, ob.p, ob.ld)
        got = ob.dense().view(B, Ho, Wo, C)
    kern = mc.upsample_fwd_kernel(B, H, W, C, s, xb.ld, 0 if nchw else ob.ld, odt, nchw)
    ran(*kern)
    check_all(what, xb, ob)
    ref = mc.resize_ref(xb.dense().view(B, H, W, C), H, W, s)
    judge(parity, f"{kern[0]} {DT_ID[odt]}", what, got, ref.y, mc.bar_resize(ref, mc.tol(odt)))
    return kern


def run_resize_bwd(ops, parity, g, H, W, s, dydt, dxdt, nchw=False, accumulate=False, lddy=None, lddx=None):
    B, Ho, Wo, C = g.shape
    what = f"B {B} {H}x{W} C {C} s {s} {'nchw' if nchw else 'pixel-major'} dy {DT_ID[dydt]} dx {DT_ID[dxdt]} accumulate {accumulate}"
    base = torch.randint(-3, 4, (B * H * W, C), generator=mc.gen(H * 100 + W)).float()
    dxb = Mat(B * H * W, C, dxdt, base, ld=lddx)
    if nchw:
        dyb = Vec(B * C * Ho * Wo, g.permute(0, 3, 1, 2).contiguous())
        ops.upsample_bwd(dyb.t, 0, True, B, H, W, C, s, dxb.p, dxb.ld, accumulate=accumulate)
        gs = dyb.dense().view(B, C, Ho, Wo).permute(0, 2, 3, 1)
    else:
        dyb = Mat(B * Ho * Wo, C, dydt, g, ld=lddy)
        ops.upsample_bwd(dyb.p, dyb.ld, False, B, H, W, C, s, dxb.p, dxb.ld, accumulate=accumulate)
        gs = dyb.dense().view(B, Ho, Wo, C)
    kern = mc.upsample_bwd_kernel(B, H, W, C, s, 0 if nchw else dyb.ld, dxb.ld, dydt, dxdt, nchw)
    ran(*kern)
    check_all(what, dyb, dxb)
    ref = mc.resize_adj_ref(gs, H, W, s)
    b0 = base.view(B, H, W, C).to(dev()).double() if accumulate else 0.0
    t = mc.tol(dxdt)
    judge(parity, f"{kern[0]} dx {DT_ID[dxdt]}", what, dxb.dense().view(B, H, W, C), ref.dx + b0, t * (ref.mag + (b0.abs() if accumulate else 0.0)) + ref.slack)
    return kern, dxb, dyb


def test_resize_sweep_pixel_major(ops, parity):
    """every (H, W) in {1, 2, 3, 4, 5, 7, 8}^2 at scale 2: upsample_fwd_row_kernel<float | bf16> and upsample_bwd_row_s_kernel<float | bf16, 2> at C = 4 (the fixed
    5-tap window against the whole footprint, H or W = 1 with every window open-ended, H = 2), upsample_fwd_kernel<float | bf16> and upsample_bwd_kernel at
    C = 3; deltas, ramp and N(0,1) ride in the batch dimension of each launch; accumulate alternates"""
    seen = set()
    for H in mc.SWEEP:
        for W in mc.SWEEP:
            acc = (H + W) % 2 == 1
            for C, ld in ((4, 12), (3, 5)):
                x = batch_of_inputs(H, W, C, seed=H * 10 + W)
                g = batch_of_gradients(2 * H, 2 * W, C, seed=H * 10 + W)
                for odt in (F32, BF):
                    seen.add(run_resize_fwd(ops, parity, x, 2, odt, ldx=ld, ldo=ld))
                k32, dx32, _ = run_resize_bwd(ops, parity, g, H, W, 2, F32, F32, accumulate=acc, lddy=ld, lddx=ld)
                seen.add(k32)
                if C == 4:
                    k16, dx16, dy16 = run_resize_bwd(ops, parity, g, H, W, 2, BF, F32, accumulate=acc, lddy=ld, lddx=ld)
                    seen.add(k16)
                    # the bf16-dy launch == the fp32-dy launch on the rounded gradient, bit for bit
                    _, dxr, _ = run_resize_bwd(ops, parity, dy16.dense().float().view(g.shape).cpu(), H, W, 2, F32, F32, accumulate=acc, lddy=ld, lddx=ld)
                    exact("upsample_bwd_row_s bf16 dy == fp32 launch on the rounded dy", f"{H}x{W}", dx16.dense(), dxr.dense())
    assert seen == {("upsample_fwd_row_kernel", (F32,)), ("upsample_fwd_row_kernel", (BF,)), ("upsample_fwd_kernel", (F32,)), ("upsample_fwd_kernel", (BF,)),
                    ("upsample_bwd_row_s_kernel", (F32, 2)), ("upsample_bwd_row_s_kernel", (BF, 2)), ("upsample_bwd_kernel", ())}


def test_resize_other_scales(ops, parity):
    """scale 1 (the identity: ry = rx = 1), 3 and 8: upsample_bwd_row_kernel<float | bf16> and the forward / generic kernels at sizes with H or W = 1"""
    seen = set()
    for s in (1, 3, 8):
        for H, W in ((1, 1), (1, 4), (2, 3), (5, 4), (8, 8)):
            for C, ld in ((4, 12), (3, 5)):
                x = batch_of_inputs(H, W, C, seed=s)
                g = batch_of_gradients(s * H, s * W, C, seed=s)
                for odt in (F32, BF):
                    seen.add(run_resize_fwd(ops, parity, x, s, odt, ldx=ld, ldo=ld))
                for dydt in ((F32, BF) if C == 4 else (F32,)):
                    seen.add(run_resize_bwd(ops, parity, g, H, W, s, dydt, F32, accumulate=s == 3, lddy=ld, lddx=ld)[0])
            if s == 1:
                xb = Mat(H * W, 4, F32, mc.resize_random(1, H, W, 4), ld=12)
                ob = Mat(H * W, 4, F32, ld=12)
                ops.upsample_fwd(xb.p, 12, 1, H, W, 4, 1, ob.p, 12)
                check_all(f"identity {H}x{W}", xb, ob)
                exact("upsample_fwd scale 1 is the identity", f"{H}x{W}", ob.dense(), xb.dense())
    assert ("upsample_bwd_row_kernel", (F32,)) in seen and ("upsample_bwd_row_kernel", (BF,)) in seen


NCHW_CASES = (  # B, C, H, W, s
    (11, 3, 4, 32, 8),     # nchw4, the decoder's geometry (Wo = 256)
    (7, 3, 3, 2, 2),       # nchw4, 126 plane rows: the row >= nrows tail of the last workgroup
    (11, 3, 3, 5, 3),      # fallback (Wo = 15), 297 plane rows: the tail of the last workgroup
    (8, 3, 2, 72, 4),      # fallback by W > 64 and Wo = 288 > 256: a second trip of the ox loop
    (5, 3, 5, 1, 8),       # W = 1: rx = 0
    (5, 3, 1, 8, 8),       # H = 1: ry = 0
    (2, 2, 64, 64, 4),     # Wo = 256, W = 64: the widest nchw4 geometry (ramp and N(0,1) only)
)


def test_resize_nchw(ops, parity):
    """upsample_fwd_nchw4_kernel / upsample_fwd_nchw_kernel and upsample_bwd_nchw4_kernel / upsample_bwd_nchw_kernel <float | bf16>: B C H s no multiple of 8,
    Wo > NT, W > 64, W or H = 1; dx with lddx = 8 (pad columns untouched), accumulate on and off"""
    seen = set()
    for B, C, H, W, s in NCHW_CASES:
        assert (B * C * H * s % 8 != 0) == ((C, H, W, s) in ((3, 3, 2, 2), (3, 3, 5, 3)))
        take = lambda full: full[(torch.arange(B) + len(full) - B % len(full)) % len(full)]       # the last B builders (all of them, cyclically, where B is larger)
        x, g = take(batch_of_inputs(H, W, C, seed=W)), take(batch_of_gradients(H * s, W * s, C, seed=W))
        seen.add(run_resize_fwd(ops, parity, x, s, F32, nchw=True, ldx=8))
        for dxdt in (F32, BF):
            for acc in (False, True):
                seen.add(run_resize_bwd(ops, parity, g, H, W, s, F32, dxdt, nchw=True, accumulate=acc, lddx=8)[0])
    assert seen == {("upsample_fwd_nchw4_kernel", ()), ("upsample_fwd_nchw_kernel", ()), ("upsample_bwd_nchw4_kernel", (F32,)), ("upsample_bwd_nchw4_kernel", (BF,)),
                    ("upsample_bwd_nchw_kernel", (F32,)), ("upsample_bwd_nchw_kernel", (BF,))}


# ================================================================================================ fused upsample + SmoothL1
L1_CASES = (  # B, C, H, W, s, target
    (1, 3, 3, 2, 2, "boundary"),      # 18 plane rows: nrows % 8 != 0
    (2, 3, 5, 1, 8, "boundary"),      # W = 1
    (1, 2, 3, 64, 4, "boundary"),     # W = 64, Wo = 256
    (2, 3, 4, 32, 8, "random"),       # the decoder's geometry
    (11, 3, 64, 1, 8, "boundary"),    # 16896 plane rows > 2048 x 8: the grid-stride loop's second trip
    (1, 1, 1, 4, 1, "boundary"),      # scale 1, H = 1
)


def test_upsample_l1(ops, parity):
    """upsample_l1_fwd_kernel and upsample_l1_bwd_kernel<float | bf16>: nrows % 8 != 0, the second trip of the forward's grid-stride loop, W = 64 / Wo = 256, W = 1,
    targets on either side of |d| = 1 and at 1e4 (the clamp), loss_sum starting non-zero, gscale != 1, lddx = 8 with the pad columns untouched"""
    for B, C, H, W, s, kind in L1_CASES:
        what = f"B {B} C {C} {H}x{W} s {s} {kind}"
        Ho, Wo = H * s, W * s
        x = mc.resize_random(B, H, W, C, seed=H + W) * 1.5
        xb = Mat(B * H * W, C, F32, x, ld=8)
        xs = xb.dense().view(B, H, W, C).cpu()
        if kind == "boundary":
            target, _ = mc.l1_boundary_target(xs, H, W, s)
        else:
            target = torch.randn(B, C, Ho, Wo, generator=mc.gen(9))
        tb = Vec(B * C * Ho * Wo, target)
        loss0, gscale = 3.0, 0.75
        loss = Vec(1, fill=loss0)
        ops.upsample_l1_fwd(xb.p, xb.ld, B, H, W, C, s, tb.t, loss.t)
        ran("upsample_l1_fwd_kernel")
        check_all(what, xb, tb, loss)
        ref = mc.l1_ref(xb.dense().view(B, H, W, C), tb.dense().view(B, C, Ho, Wo), H, W, s, gscale)
        # the loss is a sum of non-negative terms; |d| itself carries the coordinate slack of the prediction (slope of SmoothL1 <= 1)
        slack = float(ref.pred.slack.sum())
        judge(parity, "upsample_l1_fwd loss_sum", what, loss.dense(), (ref.loss_sum + loss0).reshape(1), mc.TOL[F32] * (float(ref.abs_sum) + loss0) + slack)
        for dxdt in (F32, BF):
            dx = Mat(B * H * W, C, dxdt, ld=8)
            gs = Vec(1, fill=gscale)
            ops.upsample_l1_bwd(xb.p, xb.ld, B, H, W, C, s, tb.t, gs.t, dx.p, dx.ld)
            ran("upsample_l1_bwd_kernel", (dxdt,))
            check_all(what, xb, tb, gs, dx)
            # at the branch points themselves (|d| = 1 to a rounding) the clamp is continuous; where |d| < 1 the gradient moves with the prediction's own error
            inner = (ref.d.abs() < 1.0).double() * (mc.TOL[F32] * ref.pred.y.abs().amax(-1, keepdim=True) + ref.pred.slack + 2.0 ** -23 * tb.dense().view(B, C, Ho, Wo).permute(0, 2, 3, 1).abs().double())
            moved = mc.resize_adj_ref(inner * (mc.f32(gscale) / ref.d.numel()), H, W, s).dx
            judge(parity, f"upsample_l1_bwd dx {DT_ID[dxdt]}", what, dx.dense().view(B, H, W, C), ref.dx, mc.tol(dxdt) * ref.adj.mag + ref.adj.slack + moved)


# ================================================================================================ refusals, M = 0
def test_refusals(ops):
    """argument checks: MVLTError, no launch, nothing written"""
    S = lambda n, dt=F32: torch.full((n,), SENTINEL, dtype=dt, device=dev())
    M = 16
    z, s1, s2 = S(M * 264), S(264), S(264)
    refused(lambda: ops.col_stats(z, 264, M, 260, s1, s2), s1, s2)                                            # C > 256
    refused(lambda: ops.bn_bwd_reduce(z, 264, z, 264, s1, s2, M, 260, s1, s2), s1, s2)
    dyh, z6 = S(M * 6, BF), S(M * 6)
    refused(lambda: ops.bn_bwd_reduce(dyh, 6, z6, 6, s1, s2, M, 6, s1, s2), s1, s2)                            # bf16 dy without the vector path
    zh, y16 = S(M * 12, F16), S(M * 12, F16)
    refused(lambda: ops.bn_norm(zh, 12, s1, s1, s1, s1, M, 12, y32=y16, ld32=12), y16)                         # fp16 y off the 8-wide path (C % 8 != 0)
    zf = S(M * 16)
    refused(lambda: ops.bn_norm(zf, 16, s1, s1, s1, s1, M, 16, y32=y16, ld32=16), y16)                         # ... and with an fp32 z
    x, tgt, acc, dx = S(2 * 72 * 8), S(3 * 2 * 4 * 288), S(1), S(2 * 72 * 8)
    refused(lambda: ops.upsample_l1_fwd(x, 8, 1, 2, 72, 3, 4, tgt, acc), acc)                                  # W > 64
    refused(lambda: ops.upsample_l1_bwd(x, 8, 1, 2, 72, 3, 4, tgt, acc, dx, 8), dx)
    refused(lambda: ops.upsample_l1_fwd(x, 8, 1, 3, 5, 3, 3, tgt, acc), acc)                                   # Wo % 4 != 0
    refused(lambda: ops.upsample_l1_bwd(x, 8, 1, 3, 5, 3, 3, tgt, acc, dx, 8), dx)
    dxh = S(3 * 5 * 8, BF)
    refused(lambda: ops.upsample_bwd(tgt, 4, False, 1, 3, 5, 4, 2, dxh, 8), dxh)                               # bf16 dx off the NCHW path
    refused(lambda: ops.ew_mul(None, 0, x, 8, x, 8, M=4, Cdim=8, accumulate=True, out16=dxh, ld16=8), dxh)     # accumulate without the fp32 output


def test_zero_rows(ops):
    """M = 0: every entry point that takes it returns OK, launches nothing and writes nothing"""
    S = lambda n, dt=F32: torch.full((n,), SENTINEL, dtype=dt, device=dev())
    a, b, c, d = S(64), S(64), S(64), S(64)
    h, k = S(64, BF), S(64, F16)
    before = last_kernel()
    ops.col_stats(a, 8, 0, 8, b, c)
    ops.bn_norm(a, 8, b, b, b, b, 0, 8, y32=c, ld32=8, y16=h, ld16=8)
    ops.bn_norm(k, 8, b, b, b, b, 0, 8, y32=c, ld32=8, y16=h, ld16=8)
    ops.bn_bwd_reduce(a, 8, a, 8, b, b, 0, 8, c, d)
    ops.bn_bwd_apply(a, 8, a, 8, b, b, b, b, b, 0, 8, c, 8, g_beta=d, g_gamma=d)
    ops.ew_mul(c, 8, a, 8, b, 8, M=0, Cdim=8, out16=h, ld16=8)
    ops.ew_mul3_bwd(a, 8, a, a, a, 8, b, c, d, 0, 8)
    torch.cuda.synchronize()
    assert last_kernel() == before
    for t in (a, b, c, d, h, k):
        assert bool((t.float() == SENTINEL).all())

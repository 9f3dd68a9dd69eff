"""GPU: the LayerNorm arithmetic that is written out by hand inside OTHER kernels, against the float64 references of tests/rowwise_cases.py on rows that
are known exactly (tests/fusedln_cases.py; premises and the eight wrong formulas: tests/test_fusedln_cases_cpu.py; argument: docs/fused_layernorm_edges.md):
  site 1  csrc/gemm_common.h  nt_epilogue_lean<.., EPIX = 8>   post_y / post_mean / post_rstd = LN(C row), the row split over two waves (LDS exchange)
  site 2  csrc/mlp_common.h   mlp_epilogue<C, 0>, p.post_y      LN of the output row, xor-shuffles over C / 8 lanes
  site 3  csrc/mlp_common.h   mlp_epilogue<C, 1>, p.lnb_x       norm2 backward: dx += .. in place, dx2, dgamma / dbeta through per-workgroup partials
  site 4  csrc/mlp_common.h   mlp_load_rows<C, 0>, p.ln_x       norm2 folded into the operand load

Bars: only rowwise_cases.TOL (1e-3 fp32, 2e-2 bf16), per row or per column, never against a global maximum:
  y (bf16 at every site)   per element, TOL[bf16] x max|ref| over the row
  mean, rstd               TOL of the dtype the ROW is read in (fp32 residual / out / R: 1e-3; bf16 R: 2e-2): mean against max(|ref|, row std), rstd relative
  dx, dx2 (site 3)         per element, 2 TOL[bf16] x max over the row of |ref - old| (x the row's dx2 factor), plus half a bf16 ulp of the reference element
  dgamma, dbeta            TOL[bf16] x the column's sum of absolute terms
Where the input makes the answer exact the check is torch.equal: constant rows (y == beta, mean == c), the C / out part of every launch, rows of a dropped sample
and rows whose dy is zero at site 3 (dx == old, dx2 == bf16(old x factor)), `out` with and without a fused LayerNorm beside it.
Every operand and result lives in a flat buffer of sentinels (7.0) with a guard row behind every matrix and a guard element behind every vector, the per-workgroup
partials of site 3 included; results are pre-filled with NaN, so an element that is not written is an error too.  After each launch every sentinel is bit-identical.
A failure prints the case, the instantiation (mvlt_amd._lib.last_kernel()), row, column, the value got and the value wanted.

Instantiation -> the case that launches it and asserts its name:
  gemm_nt_dma_kernel<64 | 128, 0, 8, 64, ..>    test_gemm_layernorm_epilogue, every launch (N 64 / 128)
  mlp_fused_kernel<64 | 128, 0>                 test_mlp_post_layernorm and test_mlp_folded_layernorm at hid 64
  mlp_pipe_kernel<64 | 128, 0>                  the same two at hid 128 (and 192 for post_ln)
  mlp_fused_kernel<64 | 128, 1>                 test_mlp_layernorm_backward at hid 64
  mlp_pipe_kernel<128, 1>, mlp_pipe_kernel<64, 1> (the PFALL = false epilogue)     test_mlp_layernorm_backward at hid 128 and 192

Measured on an MI355X, worst error / bar per site and dtype (against the float64 reference; these are measurements and gate nothing):
  site 1   y 0.189 (fp32 and bf16 C); mean fp32 rows 4.0e-5 / bf16 rows 3.2e-7; rstd 1.3e-4 / 6.3e-6
  site 2   y 0.193; mean 4.6e-5; rstd 1.2e-4                site 4   y 0.182; mean 3.1e-5; rstd 1.4e-4
           (0.19 = the rounding of a bf16 output: 2^-9 of an element against 2e-2 of the row maximum)
  site 3   dx 0.96, dx2 0.998 (where `old` dominates, the bar is little more than the half ulp the bf16 store may use); dgamma 5.1e-3; dbeta 0 (exact sums)
(docs/fused_layernorm_edges.md has the same figures as a table)
"""
import ctypes as C_
import math

import pytest
import torch

from tests import fusedln_cases as fc
from tests import mlp_cases as mc
from tests import rowwise_cases as rc
from tests.test_exact_gpu import dev, last_kernel, ops, ran                       # noqa: F401  (ops is the module-scoped fixture)
from tests.test_rowwise_edges_gpu import Mat, Vec, check_all, exact, judge

pytestmark = pytest.mark.gpu

BF, F32 = fc.BF, fc.F32
DT_ID = {BF: "bf16", F32: "fp32"}
NAN = math.nan


def mat(t, dtype=None):
    """an operand matrix, contiguous (the MLP entry points take no leading dimension), behind it a guard row"""
    return Mat(t.shape[0], t.shape[1], dtype or t.dtype, t, pad=0)


def vec(t):
    return None if t is None else Vec(t.numel(), t.reshape(-1), dtype=t.dtype)


def res(rows, C, dtype, pad=0):
    """a result matrix: NaN where the kernel must write"""
    return Mat(rows, C, dtype, fill=NAN, pad=pad)


def t_(b):
    return None if b is None else b.t


def judge_fwd(parity, site, what, got, ref, row_dtype):
    for (q, r, bar), g in zip(fc.ln_fwd_checks(ref, row_dtype), got):
        judge(parity, f"{site} {q} {DT_ID[row_dtype]}", what, g, r, bar)


def constant_rows_exact(what, rows, y, mean, rstd, beta, value):
    """x - mean == 0 in fp32: y is beta, rounded once, and the mean is the row's value, bit for bit; eps is all of the denominator"""
    exact("y == beta", what, y[rows], beta.to(BF)[None, :])
    exact("mean == c", what, mean[rows], value[rows])
    assert bool(torch.isfinite(rstd[rows]).all())


# ================================================================================================ site 1: GEMM EPI 8
def run_gemm_post(c, gamma, beta):
    """one mvlt_gemm_nt launch with post_y, the args struct built here: C, R and post_y eight columns wider than N.  -> (C, y, mean, rstd) dense"""
    from mvlt_amd import _lib as L
    A, W = c.A.to(BF).to(dev()).contiguous(), c.W.to(BF).to(dev()).contiguous()
    Cb, Rb, yb = res(c.M, c.N, c.cdt, pad=8), Mat(c.M, c.N, c.cdt, c.R, pad=8), res(c.M, c.N, BF, pad=8)
    mean, rstd = Vec(c.M, fill=NAN), Vec(c.M, fill=NAN)
    bias, scale, g, b = vec(c.bias), vec(c.scale), vec(gamma), vec(beta)
    a = L.GemmNTArgs(A=L.ptr(A), B=L.ptr(W), C=L.ptr(Cb.t), M=c.M, N=c.N, K=c.K, lda=c.K, ldb=c.K, ldc=Cb.ld, dtype=0, out_dtype=L.DT[c.cdt],
                     a_map=L.rowmap(), c_map=L.rowmap(), bias=L.ptr(t_(bias)), act=0, row_scale=L.ptr(t_(scale)), rows_per_scale=c.rps, R=L.ptr(Rb.t),
                     post_y=L.ptr(yb.t), post_ld=yb.ld, post_gamma=L.ptr(g.t), post_beta=L.ptr(b.t), post_eps=fc.EPS, post_mean=L.ptr(mean.t),
                     post_rstd=L.ptr(rstd.t))
    L.check(L.lib.mvlt_gemm_nt(C_.byref(a), L.stream_ptr()), "mvlt_gemm_nt")
    ran(f"gemm_nt_dma_kernel<{c.N}, 0, 8, 64")
    check_all(c.name, C=Cb, R=Rb, post_y=yb, post_mean=mean, post_rstd=rstd, bias=bias, row_scale=scale, gamma=g, beta=b)
    return Cb.dense(), yb.dense(), mean.dense(), rstd.dense()


@pytest.mark.parametrize("M", fc.GEMM_M)
@pytest.mark.parametrize("cdt", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", fc.GEMM_N)
def test_gemm_layernorm_epilogue(parity, N, cdt, M):
    """builder rows behind a factor of 0 and behind A = 0, the integer GEMM under per-sample factors, the half-row peaks and (bf16 C) rows that bf16 cannot hold"""
    gamma, beta = rc.ln_params(N)
    for K in fc.GEMM_K:
        for kind in fc.gemm_kinds(cdt):
            c = fc.gemm_case(kind, M, N, K, cdt)
            Cg, y, mean, rstd = run_gemm_post(c, gamma, beta)
            v = c.v.to(dev())
            mc.compare(Cg, v, None, f"{c.name}: C")                            # the fp32 row itself, or the row rounded once
            ref = rc.ln_fwd_ref(v, gamma.to(dev()), beta.to(dev()), fc.EPS)
            judge_fwd(parity, "site1", c.name, (y, mean, rstd), ref, cdt)
            if kind.startswith("constant"):
                constant_rows_exact(c.name, slice(None), y, mean, rstd, beta.to(dev()), v[:, 0].float())


# ================================================================================================ site 2: the MLP's post_ln
def run_mlp_fwd(ops, c, fam, *, post=None, with_out=True, out_op=False, ln=None, x=None, w=None):
    """one mvlt_mlp_fwd launch of an mlp_cases-shaped case.  post / ln = (gamma, beta).  -> namespace of dense results"""
    w = w or c
    M, Cd, hid = c.M, c.C, c.hid
    xb = mat((x if x is not None else c.x).to(BF)) if ln is None else None
    w1, w2, b1, b2, resb, scale = mat(w.w1), mat(w.w2), vec(w.b1), vec(w.b2), mat(c.res), vec(c.scale)
    bufs = dict(x=xb, w1=w1, w2=w2, b1=b1, b2=b2, residual=resb, row_scale=scale)
    o = fc.NS()
    outb = res(M, Cd, F32) if with_out else None
    opb = res(M, Cd, BF) if out_op else None
    kw = dict(row_scale=t_(scale), rows_per_scale=c.rps, out_op=opb.m if opb else None)
    for name, gb in (("post_ln", post), ("ln", ln)):
        if gb is not None:
            g, b, yb, mean, rstd = vec(gb[0]), vec(gb[1]), res(M, Cd, BF), Vec(M, fill=NAN), Vec(M, fill=NAN)
            kw[name] = (g.t, b.t, fc.EPS, yb.m, mean.t, rstd.t)
            bufs.update({f"{name}_gamma": g, f"{name}_beta": b, f"{name}_y": yb, f"{name}_mean": mean, f"{name}_rstd": rstd})
    ops.mlp_fwd(xb.m if xb else None, w1.m, b1.t, w2.m, b2.t, resb.m, outb.m if outb else None, M, Cd, hid, **kw)
    ran(f"{fam}<{Cd}, 0>")
    check_all(f"C {Cd} hid {hid} M {M}", out=outb, out_op=opb, **bufs)
    o.out, o.out_op = (outb.dense() if outb else None), (opb.dense() if opb else None)
    for name in ("post_ln", "ln"):
        if name in kw:
            setattr(o, name, tuple(bufs[f"{name}_{q}"].dense() for q in ("y", "mean", "rstd")))
    return o


@pytest.mark.parametrize("M,rps,factors", mc.FWD_ROWS)
@pytest.mark.parametrize("hid,fam", fc.POST_HID)
@pytest.mark.parametrize("C", fc.MLP_C)
def test_mlp_post_layernorm(ops, parity, C, hid, fam, M, rps, factors):
    gamma, beta = rc.ln_params(C, seed=3)
    gd, bd = gamma.to(dev()), beta.to(dev())
    what = f"C {C} hid {hid} M {M}"
    for off in (False, True):
        for kind in (fc.ROW_KINDS if factors and 0.0 in factors else fc.ROW_KINDS[:1]):
            c = fc.post_case(C, hid, M, rps, factors, off, kind)
            name = f"{what} {'off units' if off else 'all on'}, dropped rows {kind}"
            o = run_mlp_fwd(ops, c, fam, post=(gamma, beta))
            mc.compare(o.out, c.ref.out.to(dev()), c.bound.out.to(dev()) if off else None, name + ": out")
            # all on: the row is known exactly; with off units the kernel's own stored row, which the line above has pinned to the reference
            v = o.out.double() if off else c.ref.out.to(dev())
            judge_fwd(parity, "site2", name, o.post_ln, rc.ln_fwd_ref(v, gd, bd, fc.EPS), F32)
            dead = fc.dropped_rows(c).to(dev())
            if bool(dead.any()):
                exact("out == residual", name, o.out[dead], c.res.to(dev())[dead])
                if kind == "constant":
                    constant_rows_exact(name, dead, *o.post_ln, bd, o.out[:, 0])
        plain = run_mlp_fwd(ops, c, fam)
        exact("out beside post_ln == out alone", what, o.out, plain.out)
        alone = run_mlp_fwd(ops, c, fam, post=(gamma, beta), with_out=False, out_op=True)
        exact("out_op == out rounded once", what, alone.out_op, o.out.to(BF))
        for q, a_, b_ in zip(("y", "mean", "rstd"), alone.post_ln, o.post_ln):
            exact(f"post_{q} without out == with out", what, a_, b_)
    # builder rows in EVERY row: W2 = 0, b2 = 0
    for kind in fc.ROW_KINDS:
        c = fc.post_case_zero_w2(C, hid, M, rps, factors, kind)
        name = f"{what} W2 = 0, rows {kind}"
        o = run_mlp_fwd(ops, c, fam, post=(gamma, beta))
        exact("out == residual", name, o.out, c.res.to(dev()))
        judge_fwd(parity, "site2", name, o.post_ln, rc.ln_fwd_ref(c.res.to(dev()), gd, bd, fc.EPS), F32)
        if kind == "constant":
            constant_rows_exact(name, slice(None), *o.post_ln, bd, o.out[:, 0])
    # sites 4 and 2 in one launch: ordinary weights, the stored out is the row (pinned by the second launch of the plain kernel on the stored ln_y)
    w = fc.fold_weights(C, hid, seed=M)
    g4, b4 = rc.ln_params(C, seed=4)
    c = fc.NS(C=C, hid=hid, M=M, rps=rps, scale=None if factors is None else torch.tensor(factors), res=fc.builder_rows("scaled", M, C, seed=M + 3))
    name = what + " ln + post_ln"
    o = run_mlp_fwd(ops, c, fam, post=(gamma, beta), ln=(g4, b4), w=w)
    judge_fwd(parity, "site4", name, o.ln, rc.ln_fwd_ref(c.res.to(dev()), g4.to(dev()), b4.to(dev()), fc.EPS), F32)
    judge_fwd(parity, "site2", name, o.post_ln, rc.ln_fwd_ref(o.out.double(), gd, bd, fc.EPS), F32)
    exact("out == the plain kernel on the stored ln_y", name, o.out, run_mlp_fwd(ops, c, fam, x=o.ln[0], w=w).out)


# ================================================================================================ site 4: the MLP's ln fold
@pytest.mark.parametrize("M", fc.FOLD_M)
@pytest.mark.parametrize("hid,fam", fc.FOLD_HID)
@pytest.mark.parametrize("C", fc.MLP_C)
def test_mlp_folded_layernorm(ops, parity, C, hid, fam, M):
    gamma, beta = rc.ln_params(C, seed=4)
    gd, bd = gamma.to(dev()), beta.to(dev())
    w = fc.fold_weights(C, hid)
    for kind in fc.ROW_KINDS:
        c = fc.NS(C=C, hid=hid, M=M, rps=0, scale=None, res=fc.builder_rows(kind, M, C, seed=M))
        name = f"C {C} hid {hid} M {M} rows {kind}"
        o = run_mlp_fwd(ops, c, fam, ln=(gamma, beta), w=w)
        ref = rc.ln_fwd_ref(c.res.to(dev()), gd, bd, fc.EPS)
        judge_fwd(parity, "site4", name, o.ln, ref, F32)
        if kind == "constant":
            constant_rows_exact(name, slice(None), *o.ln, bd, c.res.to(dev())[:, 0])
        # the same instantiation on the same operand bits
        exact("out == the plain kernel on the stored ln_y", name, o.out, run_mlp_fwd(ops, c, fam, x=o.ln[0], w=w).out)


# ================================================================================================ site 3: the MLP's ln_bwd
DG0, DB0 = 2.0, -1.0          # what dgamma / dbeta hold before the launch: they accumulate


def run_mlp_ln_bwd(ops, k, fam, old, dx2_scale, alias):
    """mvlt_mlp_bwd_dx with lnb_x, the args struct built here (the partials get their guard, and the kernel's name can be asked for before
    mvlt_add_column_sums replaces it).  alias: lnb_dx IS dy, as the trunk calls it.  -> namespace(dx, dx2, dgamma, dbeta) dense"""
    from mvlt_amd import _lib as L
    c, M, Cd, hid = k.c, k.M, k.C, k.c.hid
    xb, dyb = mat(c.x), mat(c.dy)
    w1, w1t, w2t, b1, scale = mat(c.w1), mat(c.w1.t().contiguous()), mat(c.w2.t().contiguous()), vec(c.b1), vec(c.scale)
    lx, mean, rstd, gam = mat(k.x), vec(k.mean), vec(k.rstd), vec(k.gamma)
    dxb = dyb if alias else mat(old)
    dx2b, sc = (res(M, Cd, BF), vec(dx2_scale)) if dx2_scale is not None else (None, None)
    nwg = (M + 127) // 128
    part = Vec(nwg * 2 * Cd, fill=NAN)
    dg, db = Vec(Cd, fill=DG0), Vec(Cd, fill=DB0)
    a = L.MlpArgs(x=L.ptr(xb.t), dy=L.ptr(dyb.t), w1=L.ptr(w1.t), wb=L.ptr(w1t.t), wc=L.ptr(w2t.t), b1=L.ptr(b1.t), row_scale=L.ptr(t_(scale)),
                  rows_per_scale=c.rps, M=M, C=Cd, hid=hid, lnb_x=L.ptr(lx.t), lnb_mean=L.ptr(mean.t), lnb_rstd=L.ptr(rstd.t), lnb_gamma=L.ptr(gam.t),
                  lnb_dx=L.ptr(dxb.t), lnb_dx2=L.ptr(t_(dx2b)), lnb_dx2_scale=L.ptr(t_(sc)), lnb_dx2_rows_per_scale=fc.DX2_RPS if sc else 0,
                  lnb_partials=L.ptr(part.t))
    L.check(L.lib.mvlt_mlp_bwd_dx(C_.byref(a), L.stream_ptr()), "mvlt_mlp_bwd_dx")
    ran(f"{fam}<{Cd}, 1>")
    ops.add_column_sums(part.t[: nwg * 2 * Cd].view(nwg, 2 * Cd), dg.t[:Cd], db.t[:Cd])
    check_all(k.name, x=xb, dy=dyb, w1=w1, w1t=w1t, w2t=w2t, b1=b1, row_scale=scale, lnb_x=lx, lnb_mean=mean, lnb_rstd=rstd, lnb_gamma=gam,
              lnb_dx=dxb, lnb_dx2=dx2b, lnb_dx2_scale=sc, lnb_partials=part, dgamma=dg, dbeta=db)
    assert bool(torch.isfinite(part.dense()).all()), f"{k.name}: a workgroup left its partials unwritten"
    return fc.NS(dx=dxb.dense(), dx2=dx2b.dense() if dx2b else None, dgamma=dg.dense(), dbeta=db.dense())


# x rows, lnb_dx aliasing dy, dx2 (None: absent; else the rotation of its factor table), single live row
LNB_CONFIGS = (("scaled", True, 0, False), ("offset", False, None, False), ("scaled", False, 1, False), ("offset", True, 2, False), ("scaled", True, 0, True))


@pytest.mark.parametrize("M,rps,factors", fc.LNB_ROWS)
@pytest.mark.parametrize("hid,fam", ((64, "mlp_fused_kernel"), (128, "mlp_pipe_kernel"), (192, "mlp_pipe_kernel")))
@pytest.mark.parametrize("C", fc.MLP_C)
def test_mlp_layernorm_backward(ops, parity, C, hid, fam, M, rps, factors):
    t = rc.TOL[BF]
    for xkind, alias, dx2_seed, single in LNB_CONFIGS:
        k = fc.lnb_case(C, hid, M, rps, factors, xkind, live_row=fc.LNB_LIVE_ROW[M] if single else None)
        name = f"{k.name}, lnb_dx {'aliasing dy' if alias else 'separate'}, dx2 {'absent' if dx2_seed is None else 'rotation %d' % dx2_seed}"
        old = k.c.dy if alias else fc.lnb_old(M, C, seed=M)
        sc = None if dx2_seed is None else fc.dx2_factors(M, dx2_seed)
        got = run_mlp_ln_bwd(ops, k, fam, old, sc, alias)
        kd = fc.NS(**{**vars(k), "x": k.x.to(dev())})
        r = fc.lnb_ref(kd, old.to(dev()), sc)
        judge(parity, "site3 dx", name, got.dx, r.dx, r.bar_dx)
        u = r.untouched
        exact("dx == old", name + ": rows of a dropped sample / of a zero dy", got.dx[u], old.to(dev())[u])
        if sc is not None:
            judge(parity, "site3 dx2", name, got.dx2, r.dx2, r.bar_dx2)
            exact("dx2 == bf16(old x factor)", name, got.dx2[u], (old.to(dev()).float() * r.sc.float())[u].to(BF))
        judge(parity, "site3 dgamma", name, got.dgamma, r.dgamma + DG0, rc.bar_col(r.abs_gamma, t))
        judge(parity, "site3 dbeta", name, got.dbeta, r.dbeta + DB0, rc.bar_col(r.abs_beta, t))

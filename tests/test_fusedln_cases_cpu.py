"""CPU: the premises of tests/test_fusedln_edges_gpu.py (inputs, references and bars: tests/fusedln_cases.py), with no GPU and no library.
  * the float64 reference, rounded to the dtype the kernel stores, passes every bar of every case on its own;
  * a factor of 0 or a zero operand gives v == R in fp32 arithmetic; the integer cases stay below 2^24 (exact in any order of summation);
  * dyn = dx_mlp * factor of the all-on mlp_cases data is exact in fp32;
  * each of the eight mistakes the GPU file is there to catch, written out in fp32, FAILS the comparison on the case built for it, at a row the
    message names: (a) one-pass variance, (b) eps dropped, (c) a neighbouring row's statistics, (d) the partner wave's half-row sum lost, (e) LN of the
    bf16-rounded row, (f) the last workgroup's dgamma / dbeta partial lost, (g) dx2 under the neighbouring sample's factor, (h) `old` not added to dx."""
import pytest
import torch

from tests import fusedln_cases as fc
from tests import mlp_cases as mc
from tests import rowwise_cases as rc

BF, F32 = fc.BF, fc.F32


def fwd_worst(got, ref, row_dtype):
    """{quantity: worst(...)} of a forward site's three outputs"""
    return {q: fc.worst(getattr(got, q), r, bar) for q, r, bar in fc.ln_fwd_checks(ref, row_dtype)}


def rounded(ref):
    return fc.NS(y=ref.y.float().to(BF), mean=ref.mean.float(), rstd=ref.rstd.float())


def must_fail(w, what, rows=None):
    assert w.ratio > 2.0, f"{what}: the wrong formula stays within {w.ratio:.2f} bars (worst at row {w.row} column {w.col})"
    if rows is not None:
        assert w.row in rows, f"{what}: fails at row {w.row}, not in the rows built for it"
    return f"{what}: row {w.row} column {w.col}: got {w.got!r}, want {w.want!r} ({w.ratio:.1f} bars)"


# ================================================================================================ the reference alone
@pytest.mark.parametrize("cdt", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", fc.GEMM_N)
def test_site1_reference_alone_passes_and_v_is_exact(N, cdt):
    g, b = rc.ln_params(N)
    for M in fc.GEMM_M:
        for K in fc.GEMM_K:
            for kind in fc.gemm_kinds(cdt):
                c = fc.gemm_case(kind, M, N, K, cdt)
                assert mc.bf16_exact(c.A) and mc.bf16_exact(c.W), c.name
                assert float((c.A.abs() @ c.W.abs().t()).max()) * 2 + 9 * 2 + 5 < fc.LIM, c.name
                v32 = fc.epilogue_fp32(c)
                assert torch.equal(v32.double(), c.v), f"{c.name}: (acc + bias) * factor + R is not the row the reference normalises"
                if kind not in ("ints", "unrounded"):
                    assert torch.equal(v32, c.R.float()), f"{c.name}: v != R"
                ref = rc.ln_fwd_ref(c.v, g, b, fc.EPS)
                for q, w in fwd_worst(rounded(ref), ref, cdt).items():
                    assert w.ratio < 0.25, (c.name, q, w.ratio)
                if kind.startswith("constant"):
                    assert torch.equal(ref.y, b.double().expand_as(ref.y)) and torch.equal(ref.mean, c.v[:, 0])


def test_site1_sample_edges_fall_inside_a_half():
    for M in fc.GEMM_M[1:]:
        rps = fc.gemm_rps(M)
        assert rps > 0 and any(e % 32 for e in range(rps, M, rps)), M


def test_site1_unrounded_rows_do_not_fit_bf16():
    for N in fc.GEMM_N:
        c = fc.gemm_case("unrounded", 130, N, 72, BF)
        lost = c.v.float().to(BF).double() != c.v
        assert 0.2 < float(lost.double().mean()) < 0.8 and bool(lost.any(-1).all()), "every row holds values bf16 cannot"
        assert 0.3 < float(c.v.var(-1, unbiased=False).min()) and float(c.v.var(-1, unbiased=False).max()) < 4.0


def mlp_rows():
    return [(C, hid, M, rps, fac) for C in fc.MLP_C for hid, _ in fc.POST_HID for M, rps, fac in mc.FWD_ROWS]


def test_site2_reference_alone_passes_and_dropped_rows_are_the_residual():
    for C, hid, M, rps, fac in mlp_rows():
        g, b = rc.ln_params(C, seed=3)
        for kind in fc.ROW_KINDS:
            cases = [fc.post_case(C, hid, M, rps, fac, False, kind), fc.post_case_zero_w2(C, hid, M, rps, fac, kind)]
            for i, c in enumerate(cases):
                out = fc.integral(c.ref.out, 0.5) if kind == "constant" or (i == 0 and not bool(fc.dropped_rows(c).any())) else c.ref.out
                assert torch.equal(out.float().double(), out), "out is an fp32 number"
                dead = fc.dropped_rows(c) if i == 0 else torch.ones(M, dtype=torch.bool)
                # fp32, step by step: (acc + b2) * factor + residual
                acc = (c.ref.G @ c.w2.double().t()).float()
                v32 = (acc + c.b2) * c.srow.float() + c.res
                assert torch.equal(v32.double(), out) and torch.equal(v32[dead], c.res[dead])
                ref = rc.ln_fwd_ref(out, g, b, fc.EPS)
                for q, w in fwd_worst(rounded(ref), ref, F32).items():
                    assert w.ratio < 0.25, (C, hid, M, kind, i, q, w.ratio)
    assert bool(fc.dropped_rows(mc.fwd_case(64, 64, 200, 50, (2.0, 0.0, 0.5, 1.0), False))[50:100].all())


def lnb_all():
    return [(C, hid, M, rps, fac) for C in fc.MLP_C for hid, _ in fc.POST_HID for M, rps, fac in fc.LNB_ROWS]


def test_site3_dyn_is_exact_and_the_reference_alone_passes():
    for C, hid, M, rps, fac in lnb_all():
        for xkind, live in (("scaled", None), ("offset", None), ("scaled", fc.LNB_LIVE_ROW[M])):
            k = fc.lnb_case(C, hid, M, rps, fac, xkind, live_row=live)
            assert torch.equal(k.dyn.float().double(), k.dyn) and float(k.dyn.abs().max()) <= 512 and float(k.c.ref.dG.abs().max()) <= 256, k.name
            assert float(k.c.ref.on.min()) == 1.0, "all-on data"
            sc = fc.dx2_factors(M)
            for old in (k.c.dy, fc.lnb_old(M, C)):
                r = fc.lnb_ref(k, old, sc)
                assert fc.worst(r.dx.float().to(BF), r.dx, r.bar_dx).ratio <= 1.0 and fc.worst(r.dx2.float().to(BF), r.dx2, r.bar_dx2).ratio <= 1.0, k.name
                assert fc.worst(r.dgamma.float(), r.dgamma, rc.bar_col(r.abs_gamma, rc.TOL[BF])).ratio < 0.01
                # untouched rows: the reference IS old, and old * factor is exact in fp32 (8 bits x 3 bits)
                u = r.untouched
                assert torch.equal(r.dx[u], old.double()[u]) and torch.equal((old.float() * r.sc.float())[u].double(), r.dx2[u])
            if live is not None:
                assert int((~r.untouched).sum()) <= 1 and (M == 1 or M - live <= 128), "one live row, in the last workgroup"
                assert live // 50 >= len(fac or ()) or (fac or (1.0,))[live // max(rps, 1)] != 0, "the live row's sample is not dropped"
                assert float(r.abs_beta.max()) > 0
            elif fac and 0.0 in fac:
                assert bool(r.untouched.any()), "a dropped sample leaves untouched rows"
    assert fc.DX2_RPS not in {rps for _, rps, _ in fc.LNB_ROWS}


def test_site4_reference_alone_passes():
    for C in fc.MLP_C:
        g, b = rc.ln_params(C, seed=4)
        for M in fc.FOLD_M:
            for kind in fc.ROW_KINDS:
                ref = rc.ln_fwd_ref(fc.builder_rows(kind, M, C, seed=M), g, b, fc.EPS)
                for q, w in fwd_worst(rounded(ref), ref, F32).items():
                    assert w.ratio < 0.25, (C, M, kind, q, w.ratio)


# ================================================================================================ the eight mistakes
@pytest.mark.parametrize("C", (64, 128))
def test_a_one_pass_variance_fails_on_offset_rows(C):
    """through R of site 1 (fp32 C) and through the residual of sites 2 and 4: the rows are fp32, rstd is judged at 1e-3.  The bf16 y alone would NOT
    separate it at these widths (2e-2 of the row maximum against a ~2 % error of every element): the statistics do."""
    x = rc.ln_offset_rows(130, C, 1000 * C)
    g, b = rc.ln_params(C)
    ref = rc.ln_fwd_ref(x, g, b, fc.EPS)
    right, wrong = fwd_worst(fc.wrong_fwd(x, g, b), ref, F32), fwd_worst(fc.wrong_fwd(x, g, b, one_pass=True), ref, F32)
    assert all(w.ratio < 0.5 for w in right.values()), {q: w.ratio for q, w in right.items()}
    print(must_fail(wrong["rstd"], f"one-pass variance, C {C}, rstd"))
    assert int(wrong["rstd"].rows.sum()) > 130 // 2, "most rows fail, not one lucky one"


@pytest.mark.parametrize("C", (64, 128))
def test_b_dropped_eps_fails_on_the_small_scaled_rows(C):
    x = rc.ln_scaled_rows(130, C, 7)
    g, b = rc.ln_params(C)
    ref = rc.ln_fwd_ref(x, g, b, fc.EPS)
    small = {r for r in range(130) if r % 6 in (0, 1)}                      # factors 1e-4 and 1e-3
    assert all(w.ratio < 0.5 for w in fwd_worst(fc.wrong_fwd(x, g, b), ref, F32).values())
    wrong = fwd_worst(fc.wrong_fwd(x, g, b, no_eps=True), ref, F32)
    print(must_fail(wrong["y"], f"eps dropped, C {C}, y", small), must_fail(wrong["rstd"], "rstd", small))
    # and constant rows: inf x 0
    xc = rc.ln_constant_rows(7, C)
    assert fwd_worst(fc.wrong_fwd(xc, g, b, no_eps=True), rc.ln_fwd_ref(xc, g, b, fc.EPS), F32)["y"].ratio == float("inf")


@pytest.mark.parametrize("kind", ("offset", "scaled"))
@pytest.mark.parametrize("C", (64, 128))
def test_c_a_neighbouring_rows_statistics_fail(C, kind):
    x = fc.builder_rows(kind, 33, C, 5)
    g, b = rc.ln_params(C)
    ref = rc.ln_fwd_ref(x, g, b, fc.EPS)
    wrong = fwd_worst(fc.wrong_fwd(x, g, b, neighbour=True), ref, F32)
    print(must_fail(wrong["y"], f"neighbour's statistics, {kind}, C {C}, y"))
    if kind == "scaled":
        print(must_fail(wrong["rstd"], "rstd"))


def test_d_a_lost_half_row_sum_fails_at_128():
    c = fc.gemm_case("half", 33, 128, 72, F32)
    g, b = rc.ln_params(128)
    ref = rc.ln_fwd_ref(c.v, g, b, fc.EPS)
    assert all(w.ratio < 0.5 for w in fwd_worst(fc.wrong_fwd(c.v, g, b), ref, F32).values())
    wrong = fwd_worst(fc.wrong_fwd(c.v, g, b, drop_half=True), ref, F32)
    print(must_fail(wrong["mean"], "partner wave's sum lost, mean"), must_fail(wrong["y"], "y"))
    assert bool(wrong["mean"].rows.all()) and bool(wrong["y"].rows.all()), "every row shows it, whichever half holds its peak"


@pytest.mark.parametrize("N", fc.GEMM_N)
def test_e_layernorm_of_the_rounded_row_fails(N):
    c = fc.gemm_case("unrounded", 130, N, 200, BF)
    g, b = rc.ln_params(N)
    ref = rc.ln_fwd_ref(c.v, g, b, fc.EPS)
    assert all(w.ratio < 0.5 for w in fwd_worst(fc.wrong_fwd(c.v, g, b), ref, BF).values())
    wrong = fwd_worst(fc.wrong_fwd(c.v, g, b, round_bf16=True), ref, BF)
    print(must_fail(wrong["y"], f"LN of the rounded C, N {N}, y"))
    assert int(wrong["y"].rows.sum()) > 100


def bwd_worst(w, r):
    t = rc.TOL[BF]
    return dict(dx=fc.worst(w.dx, r.dx, r.bar_dx), dx2=fc.worst(w.dx2, r.dx2, r.bar_dx2),
                dgamma=fc.worst(w.dgamma, r.dgamma, rc.bar_col(r.abs_gamma, t)), dbeta=fc.worst(w.dbeta, r.dbeta, rc.bar_col(r.abs_beta, t)))


def right_passes(w):
    """the right formula in fp32: the bf16 stores may use up the half ulp their bar grants (a dx that `old` dominates), the column sums stay far below theirs"""
    return w["dx"].ratio <= 1.0 and w["dx2"].ratio <= 1.0 and w["dgamma"].ratio < 0.01 and w["dbeta"].ratio < 0.01


@pytest.mark.parametrize("C", fc.MLP_C)
def test_f_g_h_backward_mistakes_fail(C):
    M, rps, fac = fc.LNB_ROWS[-1]
    sc = fc.dx2_factors(M)
    live = fc.lnb_case(C, 128, M, rps, fac, "scaled", live_row=fc.LNB_LIVE_ROW[M])
    old = fc.lnb_old(M, C)
    r = fc.lnb_ref(live, old, sc)
    assert right_passes(bwd_worst(fc.wrong_bwd(live, old, sc), r))
    # (f) with the single live row in the last workgroup the lost partial is ALL of the column sums
    w = bwd_worst(fc.wrong_bwd(live, old, sc, drop_last_wg=True), r)
    print(must_fail(w["dgamma"], f"last workgroup's partial lost, C {C}, dgamma"), must_fail(w["dbeta"], "dbeta"))
    for xkind in ("scaled", "offset"):
        k = fc.lnb_case(C, 128, M, rps, fac, xkind)
        for o in (old, k.c.dy):
            r = fc.lnb_ref(k, o, sc)
            assert right_passes(bwd_worst(fc.wrong_bwd(k, o, sc), r)), xkind
            # (g) the factor of sample s + 1: rows of a sample whose neighbour has another factor
            w = bwd_worst(fc.wrong_bwd(k, o, sc, neighbour_dx2=True), r)
            print(must_fail(w["dx2"], f"dx2 under the neighbour's factor, {xkind}, C {C}"))
            assert w["dx"].ratio <= 1.0
            # (h) old dropped
            w = bwd_worst(fc.wrong_bwd(k, o, sc, no_old=True), r)
            print(must_fail(w["dx"], f"old not added, {xkind}, C {C}"))
            assert float(o.float().abs()[w["dx"].row].max()) > 0

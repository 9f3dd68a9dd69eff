"""Test infrastructure: inputs, float64 references and bars of the tests of the LayerNorm arithmetic that is written out inside OTHER kernels
(tests/test_fusedln_edges_gpu.py; the premises are pinned on the CPU by tests/test_fusedln_cases_cpu.py; the argument is in
docs/fused_layernorm_edges.md).  The four sites:
  1  csrc/gemm_common.h  nt_epilogue_lean<.., EPIX = 8>   post_y / post_mean / post_rstd = LN(C row), the row split over two waves
  2  csrc/mlp_common.h   mlp_epilogue<C, 0>, p.post_y      LN of the output row (the next block's norm1)
  3  csrc/mlp_common.h   mlp_epilogue<C, 1>, p.lnb_x       norm2 backward: dx += .. in place, dx2, dgamma / dbeta through per-workgroup partials
  4  csrc/mlp_common.h   mlp_load_rows<C, 0>, p.ln_x       norm2 folded into the operand load

Plain torch on the CPU, no GPU and no library.  Builders, references, bars and TOL are those of tests/rowwise_cases.py, the saturated integer MLP data
that of tests/mlp_cases.py.  What is new here is how a row a fused site normalises becomes KNOWN EXACTLY:
  * a factor of 0 (row_scale == 0) or a zero operand (A = 0, W2 = 0): v = (acc + bias) * 0 + R = R bit for bit, so any builder row can be put in
    front of sites 1 and 2 through R / residual;
  * integer data: v is an integer or a half below 2^24, whatever the order of summation;
  * (site 2, cases with off units) the kernel's own stored fp32 output row, which the same test pins to the MLP reference.
"""
import types

import torch

from tests import mlp_cases as mc
from tests import rowwise_cases as rc

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NS = types.SimpleNamespace
EPS = 1e-6
LIM = float(2 ** 24)
ROW_KINDS = ("offset", "constant", "scaled")
DROP_FACTORS = (0.0, 0.5, 1.0, 2.0)

# ---- site 1
GEMM_N = (64, 128)
GEMM_K = (72, 200)                             # ragged k-tiles (tests/test_exact_gpu.py)
GEMM_M = (1, 31, 33, 130, 257)                 # one row; one short of / one past a 32-row half; a second workgroup with two rows; a third with one
# ---- sites 2, 3, 4
MLP_C = (64, 128)
POST_HID = ((64, "mlp_fused_kernel"), (128, "mlp_pipe_kernel"), (192, "mlp_pipe_kernel"))
LNB_ROWS = mc.FWD_ROWS + ((260, 50, (1.0, 0.5, 2.0, 0.0, 1.0, 2.0)),)      # 260: three workgroups of partials, the last one of 4 rows
LNB_LIVE_ROW = {1: 0, 33: 32, 129: 128, 200: 130, 260: 258}               # the single live row: in the last workgroup, in the last wave that has rows
DX2_SCALES = (0.0, 1.0 / 0.8, 2.0)
DX2_RPS = 37                                   # != rows_per_scale (33, 50): the two factor tables are indexed apart
FOLD_HID = ((64, "mlp_fused_kernel"), (128, "mlp_pipe_kernel"))
FOLD_M = (1, 33, 129)
# the family literals above against the dispatch itself (csrc/mlp_plan.h), where the library is loadable: no launch of these sites asks for a pre-activation
for _C in MLP_C:
    for _hid, _fam in POST_HID + FOLD_HID:
        _fwd, _dx = mc.planned("fwd", _C, _hid, 129), mc.planned("bwd_dx", _C, _hid, 129)
        assert _fwd is None or (_fwd.name, _dx.name) == (f"{_fam}<{_C}, 0>", f"{_fam}<{_C}, 1>"), (_C, _hid, _fam)


def ints(shape, lo, hi, seed):
    """uniform integers in [lo, hi] (float64) from a seeded CPU generator"""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.randint(lo, hi + 1, shape, generator=rc.gen(seed)).double()


def picks(n, values, seed):
    return torch.tensor(values, dtype=F32)[torch.randint(0, len(values), (n,), generator=rc.gen(seed))]


def integral(ref64, unit=1.0):
    """the reference must be exact in fp32 in any order of summation: whole multiples of `unit` (a power of two) below 2^24 units"""
    q = ref64 / unit
    assert torch.equal(q, q.round()) and float(q.abs().max()) < LIM, "the reference is not an integer below 2^24: the case itself is wrong"
    return ref64


def builder_rows(kind, rows, C, seed=0):
    """fp32 [rows, C] of one of the rowwise_cases classes: what each exposes is said there and in docs/fused_layernorm_edges.md"""
    if kind == "offset":
        return rc.ln_offset_rows(rows, C, seed)
    if kind == "constant":
        return rc.ln_constant_rows(rows, C)
    assert kind == "scaled", kind
    return rc.ln_scaled_rows(rows, C, seed)


HALF_BASE, HALF_PEAK = 1.0, 9.0


def half_row_cols(N):
    return (0, N // 2 - 1, N // 2, N - 1)


def half_rows(rows, N):
    """every value 1 but ONE 9 per row, at column 0, N/2 - 1, N/2 or N - 1 (row r: entry r % 4): the whole deviation of a row lives in one wave's half,
    at the half's first or last column.  A partial sum of the partner wave that is lost, or taken from the wrong LDS slot, moves the mean by half the
    row -- and the row's only non-trivial y by many bars.  All sums are small integers: exact in fp32."""
    x = torch.full((rows, N), HALF_BASE)
    cols = torch.tensor(half_row_cols(N))[torch.arange(rows) % 4]
    x[torch.arange(rows), cols] = HALF_PEAK
    return x


# ================================================================================================ judging (device-agnostic)
def worst(got, ref, bar):
    """-> namespace(ratio, row, col, got, want, bar) of the element with the largest |got - ref| / bar; a non-finite `got` counts as infinitely wrong.
    bar broadcasts (one per row, per column or per element); 1-D operands are one column."""
    got = got.double()
    if got.dim() == 1:
        got, ref = got[:, None], ref[:, None]
        bar = bar[:, None] if torch.is_tensor(bar) and bar.dim() == 1 else bar
    bar = torch.as_tensor(bar, dtype=F64, device=got.device).expand_as(got)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    r, c = i // got.shape[1], i % got.shape[1]
    return NS(ratio=float(ratio[r, c]), row=r, col=c, got=float(got[r, c]), want=float(ref[r, c]), bar=float(bar[r, c]), rows=(ratio > 1).any(-1))


def stat_tol(row_dtype):
    """the bar of mean / rstd: they are fp32 numbers computed from the fp32 register row v, which the case knows exactly -- so the dtype the ROW was read
    in decides (fp32 residual / R: 1e-3; bf16 R: 2e-2), as tests/test_rowwise_edges_gpu.py judges them by the dtype of x"""
    return rc.tol(row_dtype)


def ln_fwd_checks(ref, row_dtype):
    """(quantity, float64 reference, bar) of a forward site: y is bf16 at every site -> TOL[bf16] of the row maximum"""
    ts = stat_tol(row_dtype)
    return (("y", ref.y, rc.bar_y(ref.y, rc.TOL[BF])), ("mean", ref.mean, rc.bar_mean(ref, ts)), ("rstd", ref.rstd, ts * ref.rstd))


# ================================================================================================ site 1: the GEMM's LayerNorm epilogue
def gemm_rps(M):
    """rows_per_scale = M // 2 - 3: the sample edges fall inside a 32-row half"""
    return max(1, M // 2 - 3)


def _zero_factor(M):
    rps = gemm_rps(M)
    return torch.zeros((M + rps - 1) // rps, dtype=F32), rps


def gemm_case(kind, M, N, K, cdt, seed=0):
    """one launch of site 1.  -> namespace(A, W [float64 integers, bf16-exact], bias, scale [fp32 or None], rps, R [cdt], v [float64: the fp32 row the
    epilogue normalises, exact], name).  kind:
      "<rows>/rs0"   builder rows in R, integer A, W and bias under a factor of 0            "<rows>/a0"   builder rows in R, A = 0, no bias, no factor
      "ints"         integer GEMM, integer R, per-sample factors from {0, 0.5, 1, 2}          "half"        half_rows in R, A = 0
      "unrounded"    (bf16 C) offset rows in R plus a small integer GEMM part and a bias of 1..3: v = 251 .. 261, half of it odd above 256, which bf16
                     cannot hold; the variance stays about 1, so LN of the ROUNDED C is many bars from LN of v"""
    s = 1000 * N + 10 * K + M + seed
    c = NS(name=f"{kind} M {M} N {N} K {K} {'bf16' if cdt == BF else 'fp32'}", kind=kind, M=M, N=N, K=K, cdt=cdt, bias=None, scale=None, rps=0)
    c.A, c.W = ints((M, K), -3, 3, s + 1), ints((N, K), -3, 3, s + 2)
    rows, _, via = kind.partition("/")
    if kind == "ints":
        c.bias, c.rps = ints(N, -9, 9, s + 3).float(), gemm_rps(M)
        c.scale = picks((M + c.rps - 1) // c.rps, DROP_FACTORS, s + 4)
        c.R = ints((M, N), -5, 5, s + 5).to(cdt)
        srow = c.scale.double().repeat_interleave(c.rps)[:M, None]
        c.v = integral((c.A @ c.W.t() + c.bias.double()) * srow + c.R.double(), 0.5)
    elif kind == "unrounded":
        assert cdt == BF
        c.A = torch.zeros(M, K, dtype=F64)
        c.A[torch.arange(M), torch.arange(M) % K] = ints(M, 0, 1, s + 6) * 2 - 1                  # one +-1 per row
        c.W = ints((N, K), -2, 2, s + 2)
        c.bias = ints(N, 1, 3, s + 3).float()
        c.R = rc.ln_offset_rows(M, N, s).to(cdt)
        c.v = integral(c.A @ c.W.t() + c.bias.double() + c.R.double())
    else:
        c.R = (half_rows(M, N) if rows == "half" else builder_rows(rows, M, N, s)).to(cdt)
        if rows == "half" or via == "a0":
            c.A = torch.zeros(M, K, dtype=F64)
        else:
            assert via == "rs0", kind
            c.bias = ints(N, -9, 9, s + 3).float()
            c.scale, c.rps = _zero_factor(M)
        c.v = c.R.double()
    return c


def gemm_kinds(cdt):
    k = [f"{rows}/{via}" for rows in ROW_KINDS for via in ("rs0", "a0")] + ["ints", "half"]
    return k + ["unrounded"] if cdt == BF else k


def epilogue_fp32(c):
    """v as the epilogue forms it, in fp32 arithmetic step by step: (acc + bias) * factor + R"""
    acc = (c.A @ c.W.t()).float()                                          # integers: exact
    bias = c.bias if c.bias is not None else torch.zeros(c.N)
    srow = c.scale.repeat_interleave(c.rps)[:c.M, None] if c.scale is not None else torch.ones(c.M, 1)
    return (acc + bias) * srow + c.R.float()


# ================================================================================================ site 2: the MLP's post_ln
def variant(c, **kw):
    """a copy of an mlp_cases case with some operands replaced and the reference recomputed (the off-unit bounds do not depend on the residual)"""
    d = NS(**vars(c))
    for k, v in kw.items():
        setattr(d, k, v)
    d.ref = mc.reference(d)
    return d


def dropped_rows(c):
    """bool [M]: the rows of the samples whose DropPath factor is 0"""
    return (c.srow[:, 0] == 0) if c.scale is not None else torch.zeros(c.M, dtype=torch.bool)


def post_case(C, hid, M, rps, factors, off, kind):
    """the mlp_cases forward case with builder rows of `kind` in the residual of every DROPPED sample: there out = (..) * 0 + residual = residual"""
    c = mc.fwd_case(C, hid, M, rps, factors, off)
    dead = dropped_rows(c)
    if not bool(dead.any()):
        return c
    res = c.res.clone()
    res[dead] = builder_rows(kind, int(dead.sum()), C, seed=M)
    return variant(c, res=res)


def post_case_zero_w2(C, hid, M, rps, factors, kind):
    """W2 = 0 and b2 = 0: out = residual in EVERY row, whatever the factor: builder rows in front of site 2 at every row geometry"""
    c = mc.fwd_case(C, hid, M, rps, factors, False)
    d = variant(c, w2=torch.zeros_like(c.w2), b2=torch.zeros_like(c.b2), res=builder_rows(kind, M, C, seed=M + 1))
    d.bound = NS(**{k: None for k in vars(c.bound)})
    return d


# ================================================================================================ site 3: the MLP's ln_bwd
def lnb_case(C, hid, M, rps, factors, xkind, live_row=None):
    """all-on mlp_cases data -> dyn = dx_mlp * factor exactly (integers and halves); lnb_x from a rowwise builder; mean / rstd in float64 from lnb_x,
    rounded to fp32 -- the reference uses the ROUNDED values, the op's contract.  live_row: dy is zero in every other row."""
    c = mc.fwd_case(C, hid, M, rps, factors, False)
    if live_row is not None:
        dy = torch.zeros_like(c.dy)
        dy[live_row] = c.dy[live_row]
        c = variant(c, dy=dy)
    x = builder_rows(xkind, M, C, seed=M + 2)
    gamma, _ = rc.ln_params(C, seed=C)
    st = rc.ln_fwd_ref(x, gamma, torch.zeros(C), EPS)
    return NS(c=c, C=C, M=M, x=x, gamma=gamma, mean=st.mean.float(), rstd=st.rstd.float(), dyn=integral(c.ref.dx, 0.5), live_row=live_row,
              name=f"C {C} hid {hid} M {M} x {xkind}" + (f" live row {live_row}" if live_row is not None else ""))


def dx2_factors(M, seed=0):
    n = (M + DX2_RPS - 1) // DX2_RPS
    return torch.tensor([DX2_SCALES[(b + seed) % 3] for b in range(n)], dtype=F32)


def lnb_old(M, C, seed=0):
    """what a separate lnb_dx buffer holds before the launch: 3 N(0,1) in bf16, no zeros"""
    o = (3 * torch.randn(M, C, generator=rc.gen(seed + 500))).to(BF)
    return torch.where(o == 0, torch.ones_like(o), o)


def lnb_ref(k, old, dx2_scale=None):
    """-> namespace(part [LN backward alone], dx = part + old, dx2 = dx * factor of the row, dgamma, dbeta, abs_gamma, abs_beta, untouched [rows whose
    dyn is all zero: dx == old bit for bit], bar_dx, bar_dx2)"""
    dev = k.x.device
    r = rc.ln_bwd_ref(k.dyn.to(dev), k.x, k.gamma.to(dev), k.mean.to(dev), k.rstd.to(dev))
    out = NS(part=r.dx, dx=r.dx + old.double(), dgamma=r.dgamma, dbeta=r.dbeta, abs_gamma=r.abs_gamma, abs_beta=r.abs_beta,
             untouched=(k.dyn.to(dev) == 0).all(-1))
    t = rc.TOL[BF]
    out.bar_dx = rc.bar_dx(out.part, t) + rc.bf16_half_ulp(out.dx)
    if dx2_scale is not None:
        out.sc = dx2_scale.to(dev).double()[torch.arange(k.M, device=dev) // DX2_RPS][:, None]
        out.dx2 = out.dx * out.sc
        out.bar_dx2 = rc.bar_dx(out.part * out.sc, t) + rc.bf16_half_ulp(out.dx2)
    return out


# ================================================================================================ site 4: the MLP's ln fold
def fold_weights(C, hid, seed=0):
    """ordinary small weights: site 4's out is compared bit for bit with a second launch, not with a closed form"""
    g = rc.gen(seed + 900)
    r = lambda *s: torch.randn(*s, generator=g)
    return NS(w1=(r(hid, C) * C ** -0.5).to(BF), w2=(r(C, hid) * hid ** -0.5).to(BF), b1=0.1 * r(hid), b2=0.1 * r(C))


# ================================================================================================ what a WRONG kernel would return
# Each of these computes, in the arithmetic of the kernel (fp32), what one specific mistake gives.  tests/test_fusedln_cases_cpu.py runs them through the
# comparison of the GPU file on the case built for the mistake and requires the failure, at the row it names.
def wrong_fwd(v, gamma, beta, eps=EPS, *, one_pass=False, no_eps=False, neighbour=False, drop_half=False, round_bf16=False):
    """LN forward of the fp32 rows v with one mistake -> namespace(y [bf16], mean, rstd)"""
    v = v.float()
    src = v.to(BF).float() if round_bf16 else v
    n = src.shape[-1]
    inv = torch.tensor(1.0 / n, dtype=F32)
    s = src[:, : n // 2].sum(-1) if drop_half else src.sum(-1)
    mean = s * inv
    if one_pass:
        var = (src * src).sum(-1) * inv - mean * mean
    else:
        d = src - mean[:, None]
        var = (d * d).sum(-1) * inv
    rstd = var.rsqrt() if no_eps else (var + torch.tensor(eps, dtype=F32)).rsqrt()
    if neighbour:
        mean, rstd = mean.roll(-1), rstd.roll(-1)
    y = (src - mean[:, None]) * rstd[:, None] * gamma + beta
    return NS(y=y.to(BF), mean=mean, rstd=rstd)


def wrong_bwd(k, old, dx2_scale, *, drop_last_wg=False, neighbour_dx2=False, no_old=False):
    """site 3 in fp32 with one mistake -> namespace(dx, dx2 [bf16], dgamma, dbeta [fp32, the sums alone])"""
    dyn, x, g = k.dyn.float(), k.x, k.gamma
    xh = (x - k.mean[:, None]) * k.rstd[:, None]
    gg = dyn * g
    s1, s2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    dxv = k.rstd[:, None] * (gg - s1 - xh * s2) + (0.0 if no_old else old.float())
    sample = torch.arange(k.M) // DX2_RPS
    if neighbour_dx2:
        sample = (sample + 1) % dx2_scale.numel()
    rows = slice(0, (k.M - 1) // 128 * 128) if drop_last_wg else slice(0, k.M)
    return NS(dx=dxv.to(BF), dx2=(dxv * dx2_scale[sample][:, None]).to(BF), dgamma=(dyn * xh)[rows].sum(0), dbeta=dyn[rows].sum(0))

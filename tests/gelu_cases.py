"""Test infrastructure: the active-range sweep of every GELU / GELU' form (tests/test_gelu_range_gpu.py; the premises are pinned on the CPU by
tests/test_gelu_cases_cpu.py; the argument is written down in docs/gelu_range.md).  Plain torch on the CPU, no GPU and no library.

Every pre-activation is h[m][j] = a_m * w_j with a_m = +-2^e, e in [-28, 3], and w_j = 1 + (j mod 128) / 128: both bf16-exact, and so is the product.  64 rows x
128 columns are every bf16 value of 32 binades and both signs; three more rows add -0, the smallest bf16 normal and a bf16 denormal.  The builders below give each
kernel operands that make one output element ONE activation (a one-hot second matrix: no sum sits between the activation and the assertion).

The forms of csrc/common.h and csrc/mlp_wgrad.hip are RESTATED here in float32 -- same constants, same clamps, the table read from csrc/gelu_lut.inc itself --
only to size the bars: per form and row (= sign and binade), E_phi = max |Phi~ - Phi| and E_dg = max |GELU'~ - GELU'| over the 128 mantissas, against float64.
The comparison itself is against the float64 exact-erf GELU and its autograd derivative, never against the restatement."""
import functools
import os
import re
import types

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NS = types.SimpleNamespace

EXPS = tuple(range(-28, 4))
NMAIN = 2 * len(EXPS)                                        # 64 rows: sign x exponent
EXTRA = (-0.0, 2.0 ** -126, -(2.0 ** -130))                  # -0, the smallest bf16 normal, a bf16 denormal (its products with w_j are not bf16-exact: below every bar)
DENORMAL_ROWS = (NMAIN + 2,)
NROWS = NMAIN + len(EXTRA)                                   # 67
SLOP = 1.25                                                  # FMA contraction and the 1-ulp hardware exp2 / rcp against torch's (supposed; measured margins in the doc)
ABS = 4e-7                                                   # fp32 rounding of the result itself, relative to max(1, |r|)


def row_values():
    """a_m, float64 [67]: +2^e for e = -28 .. 3, then -2^e, then the extra rows"""
    a = [2.0 ** e for e in EXPS] + [-(2.0 ** e) for e in EXPS] + list(EXTRA)
    return torch.tensor(a, dtype=F64)


def col_values(n):
    """w_j = 1 + (j mod 128) / 128, float64 [n]"""
    return 1.0 + (torch.arange(n) % 128).double() / 128


def sweep(n=128, rows=None):
    """h[m][j] = a_m w_j, float64 [rows, n]"""
    a = row_values() if rows is None else row_values()[list(rows)]
    return a[:, None] * col_values(n)[None, :]


def bf16_exact(t):
    return torch.equal(t.float().to(BF).double(), t.double())


def exact(h):
    """float64 exact-erf GELU and its autograd derivative"""
    x = h.double().clone().requires_grad_(True)
    g = torch.nn.functional.gelu(x)
    g.sum().backward()
    return g.detach(), x.grad


# ---------------------------------------------------------------------------------------------------------------- the forms, restated in float32
# Each returns (g~, dg~) as float32 for float32 h: GELU and GELU' as the source computes them.  `v` names a deliberately WRONG variant (the perturbations of the CPU test); None is the form as it stands.
LOG2E = 1.4426950408889634
GP0, GP1, GP2 = 1.594965410743013, 0.07397063459225359, -0.0006933278070537189
PHI_C = (2.816099979e-08, -1.891889492e-06, 5.419039730e-05, -8.789809206e-04, 9.112951399e-03, -6.538835501e-02, 3.985269119e-01)
DG_C = (-1.641974535e-08, 1.213803683e-06, -3.845951304e-05, 6.876447493e-04, -7.687437410e-03, 5.591481231e-02, -2.620298260e-01, 7.967216338e-01)
PHI_CLAMP, DG_CLAMP, SIG_CLAMP = 3.985, 4.0, 7.0
AS_P, AS_A = 0.3275911, (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)
INV_SQRT2, INV_SQRT2PI = 0.70710678118654752440, 0.39894228040143267794


def f32(v):
    return torch.tensor(v, dtype=F32)


def fma(a, b, c):
    """a b + c rounded once, as v_fma_f32 / v_pk_fma_f32 do (the source writes __builtin_fmaf, or a * b + c under -ffp-contract=fast): the product of two float32
    is exact in float64"""
    return (a.double() * b.double() + (c.double() if torch.is_tensor(c) else c)).float()


def horner(coef, s):
    r = torch.full_like(s, coef[0])
    for c in coef[1:]:
        r = fma(r, s, f32(c))
    return r


def poly_phi(h, v=None):
    """gelu_poly1: Phi(xc) = 1/2 + xc P(xc^2), xc clamped at 3.985; g = h Phi"""
    clamp = DG_CLAMP if v == "clamp4" else PHI_CLAMP
    coef = list(PHI_C)
    if v == "coef_sign":
        coef[2] = -coef[2]
    xc = h.clamp(-clamp, clamp)
    return fma(xc, horner(coef, xc * xc), 0.5)


def form_poly(h, v=None):
    """gelu_poly1 / gelu_poly_grad1 (gelu_fast2 / gelu_fast_grad2 / gelu_fast1 / gelu_fast_grad1 at MVLT_GELU_POLY = 3)"""
    coef = list(DG_C)
    if v == "coef_sign":
        coef[3] = -coef[3]
    xc = h.clamp(-DG_CLAMP, DG_CLAMP)
    return h * poly_phi(h, v), fma(xc, horner(coef, xc * xc), 0.5)


def form_pair(h, v=None):
    """the packed polynomial pair of gelu_fast_both2 (MVLT_GELU_POLY bit 2; compiled out at the default 3): Phi polynomial + one exponential"""
    xc = h.clamp(-PHI_CLAMP, PHI_CLAMP)
    ph = poly_phi(h, v)
    e = torch.exp2(xc * xc * f32(-0.5 * LOG2E))
    return h * ph, fma(xc * f32(INV_SQRT2PI), e, ph)


def form_sigmoid(h, v=None):
    """gelu_fast_parts2 + the tail of gelu_fast_both2 at MVLT_GELU_POLY = 3: Phi ~ sigmoid(u(x)), the derivative is the approximant's own"""
    xc = h.clamp(-SIG_CLAMP, SIG_CLAMP)
    s2 = xc * xc
    t = xc * ((s2 * f32(-LOG2E * GP2) + f32(-LOG2E * GP1)) * s2 + f32(-LOG2E * GP0))
    e = torch.exp2(t)
    sg = 1.0 / (e + 1.0)
    up = (s2 * f32(5.0 * GP2) + f32(3.0 * GP1)) * s2 + f32(GP0)
    if v == "coef_sign":
        up = (s2 * f32(5.0 * GP2) - f32(3.0 * GP1)) * s2 + f32(GP0)
    return h * sg, (h * up) * (sg * sg * e) + sg


def _erf_parts(az):
    t = 1.0 / (1.0 + f32(AS_P) * az)
    poly = horner(AS_A, t) * t
    return poly


def form_erf(h, v=None):
    """gelu_erf / gelu_erf_grad (scalar: the ragged columns of the generic GEMM epilogue, gelu_bwd_kernel)"""
    z = h * f32(INV_SQRT2)
    az = z.abs()
    y = torch.copysign(1.0 - _erf_parts(az) * torch.exp(-az * az), z)
    return 0.5 * h * (1.0 + y), 0.5 * (1.0 + y) + h * f32(INV_SQRT2PI) * torch.exp(-0.5 * h * h)


def form_erf2(h, v=None):
    """gelu_erf2 / gelu_erf_grad2 (packed: the full 8-column chunks of the generic GEMM epilogue)"""
    az = h.abs() * f32(INV_SQRT2)
    gauss = torch.exp2(az * az * f32(-LOG2E))
    y = 1.0 - _erf_parts(az) * gauss
    hx = h * 0.5
    hs = torch.copysign(torch.full_like(h, 0.5), h)
    return hx + hx.abs() * y, (hs * y + 0.5) + h * (gauss * f32(INV_SQRT2PI))


@functools.lru_cache(maxsize=None)
def lut():
    """csrc/gelu_lut.inc as the kernel includes it: (BASE, TOP, float32 [N, 2])"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "mvlt_amd", "csrc", "gelu_lut.inc")).read()
    base, top, n = (int(re.search(r"#define MVLT_GELU_LUT_%s (\d+)" % k, text).group(1)) for k in ("BASE", "TOP", "N"))
    rows = re.findall(r"\{([-+0-9.e]+)f, ([-+0-9.e]+)f\}", text)
    assert len(rows) == n == top - base + 1
    return base, top, torch.tensor([[float(a), float(b)] for a, b in rows], dtype=F64).float()


def form_lut(h, v=None):
    """gelu_lut_both2 (mlp_wgrad2_kernel): the input rounded to bf16, its magnitude's 15 bits clamped to [BASE, TOP] = [2^-9, 8], the sign by one FMA"""
    base, top, tab = lut()
    u = (h.to(BF).view(torch.int16).to(torch.int32) & 0x7fff)
    idx = u.clamp(base, top) - base
    if v == "index":
        idx = (idx + 1).clamp(max=top - base)
    t = tab[idx.long()]
    sign = torch.where(torch.signbit(h), -1.0, 1.0).float()
    if v == "sign":
        sign = torch.ones_like(sign)
    return h * (sign * t[..., 0] + 0.5), sign * t[..., 1] + 0.5


FORMS = dict(poly=form_poly, pair=form_pair, sigmoid=form_sigmoid, erf=form_erf, erf2=form_erf2, lut=form_lut)


def emulate(form, h64, v=None, lanes=False):
    """(g~, dg~) of a form over a float64 h, as float64; lanes: the two packed lanes exchanged (each result taken from its neighbour's input)"""
    h = h64.float()
    if lanes:
        h = h.reshape(h.shape[0], -1, 2).flip(-1).reshape(h.shape)
    g, dg = FORMS[form](h, v)
    return g.double(), dg.double()


@functools.lru_cache(maxsize=None)
def errors(form):
    """E_phi, E_dg per row (float64 [67]) of a form: the maximum over the 128 mantissas of |Phi~ - Phi| and |GELU'~ - GELU'|.  Phi~ = g~ / h is taken in float64 from
    the float32 g~ (where h is 0 or underflows the quotient: from the form's GELU' at that point, whose limit at 0 it is)."""
    h = sweep(128)
    g, dg = emulate(form, h)
    r, dr = exact(h)
    big = h.abs() >= 2.0 ** -100
    e_phi = torch.where(big, ((g - r) / torch.where(big, h, torch.ones_like(h))).abs(), (dg - dr).abs())
    return NS(phi=e_phi.max(1).values, dg=(dg - dr).abs().max(1).values, abs_g=(g - r).abs().max(1).values)


def half_ulp_bf16(v):
    """half a bf16 ulp (8 significant bits) of |v|: 2^(floor(log2 |v|) - 8), 0 at 0"""
    return torch.ldexp(torch.ones_like(v), torch.frexp(v)[1] - 9) * (v != 0)


def bar(form, what, h, r, rows, *, rounded):
    """the bound of one activation per element: h, r float64 [R, n] (input and float64 reference), rows the sweep row of each row of h (None: the worst row for all).
    SLOP x E_row x (|h| for GELU, 1 for GELU') + half a bf16 ulp where the kernel rounds + ABS x max(1, |r|).  The half ulp is that of |r| + the rest of the bar, not
    of r alone: the kernel rounds ITS value, which may lie across a power of two from r (up to twice the half ulp of r just under a power of two, and in the tiny
    binades where ABS is all of the bar; docs/gelu_range.md names this as the one departure from the formula the tests were specified with)."""
    e = errors(form)
    E = e.phi if what == "g" else e.dg
    E = E.max() if rows is None else E[list(rows)][:, None]  # rows None: an input that is no sweep value (the integer pre-activations of the 8-phase position case) takes the form's worst row
    b = SLOP * E * (h.abs() if what == "g" else torch.ones_like(h)) + ABS * r.abs().clamp(min=1.0)
    if rounded:
        b = b + half_ulp_bf16(r.abs() + b)
    return b


class OverBar(AssertionError):
    """a failed comparison; .first holds the first few (row, col, h, got, want)"""

    def __init__(self, message, first):
        super().__init__(message)
        self.first = first


def compare(got, want, bound, h, what):
    """|got - want| <= bound elementwise; a failure names (row, col, h, got, want).  Returns the worst error / bound."""
    assert got.shape == want.shape == bound.shape == h.shape, (what, got.shape, want.shape, bound.shape, h.shape)
    g = got.double().cpu()
    err = (g - want).abs()
    bad = ~(err <= bound)                                    # (a NaN is bad)
    if bool(bad.any()):
        g2, w2, h2, b2 = (t.reshape(t.shape[0], -1) for t in (g, want, h, bad))
        idx = b2.nonzero()
        first = [(int(r), int(k), float(h2[r, k]), float(g2[r, k]), float(w2[r, k])) for r, k in idx[:6].tolist()]
        raise OverBar(f"{what}: {int(b2.sum())} of {b2.numel()} elements over their bar; first (row, col, h, got, want): {first}", first)
    return float((err / bound).max())


# ---------------------------------------------------------------------------------------------------------------- one-hot operands
def mlp_fwd_case(C, hid, s):
    """forward: x[m][0] = a_m, W1[j][0] = w_j, W2[c][j] = 1 iff j == c + C s -- out[m][c] = bf16(gelu~(h[m][c + C s])) for the columns c with c + C s < hid"""
    x = torch.zeros(NROWS, C, dtype=F64)
    x[:, 0] = row_values()
    w1 = torch.zeros(hid, C, dtype=F64)
    w1[:, 0] = col_values(hid)
    w2 = torch.zeros(C, hid, dtype=F64)
    cols = [c for c in range(C) if c + C * s < hid]
    for c in cols:
        w2[c, c + C * s] = 1.0
    return NS(x=x, w1=w1, w2=w2, cols=cols, units=[c + C * s for c in cols], h=sweep(hid))


def fwd_slices(C, hid):
    return (hid + C - 1) // C


def mlp_dx_case(C, hid, grp):
    """input gradient: h as in the forward; dy[m][0] = 1 and W2[0][j] = 1 make dG = 1 everywhere; W1[j][1 + k] = 1 for the k-th unit j_k of group `grp` (C - 1
    units), x zero in those columns -- dx[m][1 + k] = bf16(gelu'~(h[m][j_k])), dx[m][0] = sum_j bf16(gelu'~(h[m][j])) w_j"""
    units = list(range(grp * (C - 1), min(hid, (grp + 1) * (C - 1))))
    x = torch.zeros(NROWS, C, dtype=F64)
    x[:, 0] = row_values()
    w1 = torch.zeros(hid, C, dtype=F64)
    w1[:, 0] = col_values(hid)
    for k, j in enumerate(units):
        w1[j, 1 + k] = 1.0
    w2 = torch.zeros(C, hid, dtype=F64)
    w2[0, :] = 1.0
    dy = torch.zeros(NROWS, C, dtype=F64)
    dy[:, 0] = 1.0
    return NS(x=x, w1=w1, w2=w2, dy=dy, units=units, h=sweep(hid))


def dx_groups(C, hid):
    return (hid + C - 2) // (C - 1)


def dw_rows(M):
    """the sweep row behind each of M token rows of a weight-gradient launch: the 64 main rows, the extra ones, then the main rows again"""
    return [m if m < NROWS else (m - NROWS) % NMAIN for m in range(M)]


def mlp_dw2_case(C, hid, M):
    """G through dW2: dy[m][c] = 1 iff c == m, W2 = 0 (dG = 0: dW1 = db1 = 0) -- dW2[c][j] = bf16(gelu~(h[c][j])), db2 = 1"""
    assert M <= C
    rows = dw_rows(M)
    x = torch.zeros(M, C, dtype=F64)
    x[:, 0] = row_values()[rows]
    w1 = torch.zeros(hid, C, dtype=F64)
    w1[:, 0] = col_values(hid)
    dy = torch.eye(M, C, dtype=F64)
    return NS(x=x, w1=w1, w2=torch.zeros(C, hid, dtype=F64), dy=dy, rows=rows, h=sweep(hid, rows))


def mlp_dw1_case(C, hid, part):
    """dH through dW1: rows `part` (C - 1 sweep rows at most); x[m][0] = a_m, x[m][1 + m] = 1, W1[j][c >= 1] = 0, dy[m][0] = 1, W2[0][j] = 1 (dG = 1) --
    dW1[j][1 + m] = bf16(gelu'~(h[m][j])), dW1[j][0] = sum_m dH a_m, db1[j] = sum_m dH, dW2[0][j] = sum_m G, db2[0] = M"""
    rows = list(range(part * (C - 1), min(NROWS, (part + 1) * (C - 1))))
    M = len(rows)
    x = torch.zeros(M, C, dtype=F64)
    x[:, 0] = row_values()[rows]
    for m in range(M):
        x[m, 1 + m] = 1.0
    w1 = torch.zeros(hid, C, dtype=F64)
    w1[:, 0] = col_values(hid)
    w2 = torch.zeros(C, hid, dtype=F64)
    w2[0, :] = 1.0
    dy = torch.zeros(M, C, dtype=F64)
    dy[:, 0] = 1.0
    return NS(x=x, w1=w1, w2=w2, dy=dy, rows=rows, h=sweep(hid, rows))


def dw1_parts(C):
    return (NROWS + C - 2) // (C - 1)


def gemm_case(N, K=8, j0=0):
    """act 1: A[m][0] = a_m, B[n][0] = w_(j0 + n) -- C = gelu~(h), H = h.  act 2: A2[m][1] = 1, B2[n][1] = 1, column 0 zero (the product is exactly 1), H = h -- C = gelu'~(h)"""
    A = torch.zeros(NROWS, K, dtype=F64)
    A[:, 0] = row_values()
    B = torch.zeros(N, K, dtype=F64)
    B[:, 0] = col_values(j0 + N)[j0:]
    A2, B2 = torch.zeros(NROWS, K, dtype=F64), torch.zeros(N, K, dtype=F64)
    A2[:, 1] = 1.0
    B2[:, 1] = 1.0
    return NS(A=A, B=B, A2=A2, B2=B2, h=sweep(j0 + N)[:, j0:])


def h_of(c):
    """the pre-activations a case's operands give, in float64 (b1 = 0)"""
    return c.x @ c.w1.t()


# ---------------------------------------------------------------------------------------------------------------- the 8-phase NT GEMM epilogues (tests/test_gelu_p8_gpu.py)
# gemm_nt_p8_kernel<3 | 4, 4 | 3, 2, 2, false> compiles nt_epilogue_lean<128, EPI, TM = 8 | 6, NWN = 4, FULL = true>: 2 x 4 waves, a wave tile of (16 TM) x 64, walked in
# TM / 2 = 4 | 3 halves of 32 rows; a lane owns the 8 columns `n0 + 64 wn + 8 (lane % 8)` and the rows `... + 32 half + 8 it + lane / 8`.  The launches are as large as
# the plan's smallest 8-phase shapes, so nothing of M x N elements lives on the host: every expectation is a small TABLE (the 67 x 128 sweep, or the integers) and an
# index u[m][n] into it, built where the output lives.  The functions below take a device for that reason and run on the CPU just the same.
P8_N = 2048
P8_M = {256: 6400, 192: 4608}                                # tile height -> rows: 200 tiles of 256 x 256, 192 tiles of 192 x 256 (the smallest counts the plan takes)
P8_KERNEL = {256: "gemm_nt_p8_kernel<%d, 4, 2, 2, false>", 192: "gemm_nt_p8_kernel<%d, 3, 2, 2, false>"}
P8_BATCH = {256: (5, 1280), 192: (6, 768)}                   # batches x rows per batch of the layout case
NFLAT = NROWS * 128
INT_LIM = 256
BIAS2 = {5: 0.5, 70: -1.5, 131: 2.0, 200: -3.0, 1031: 0.75, 2047: 1.0}      # act 2: one column in every wave column, the first and the last lane chunk; no entry cancels a power of two


@functools.lru_cache(maxsize=None)
def sweep_table(form="poly"):
    """the sweep laid flat (u = 128 row + column): inputs, float64 references and bars.  bar_dg is the GELU' bar BEFORE the product with the accumulator and its rounding."""
    h, rows = sweep(128), list(range(NROWS))
    g, dg = exact(h)
    loose = torch.zeros(NROWS, 128, dtype=torch.bool)
    loose[list(DENORMAL_ROWS)] = True
    return NS(h=h.flatten(), g=g.flatten(), dg=dg.flatten(), bar_g=bar(form, "g", h, g, rows, rounded=True).flatten(),
              bar_dg=bar(form, "dg", h, dg, rows, rounded=False).flatten(), loose=loose.flatten())


@functools.lru_cache(maxsize=None)
def int_table(form="poly"):
    """the integers -256 .. 256 (u = h + 256), each a bf16 value: the worst sweep row's E for all of them"""
    h = torch.arange(-INT_LIM, INT_LIM + 1).double()[None, :]
    g, dg = exact(h)
    return NS(h=h.flatten(), g=g.flatten(), dg=dg.flatten(), bar_g=bar(form, "g", h, g, None, rounded=True).flatten(),
              bar_dg=bar(form, "dg", h, dg, None, rounded=False).flatten(), loose=torch.zeros(2 * INT_LIM + 1, dtype=torch.bool))


def grid(M, N, dev="cpu"):
    return torch.arange(M, device=dev)[:, None], torch.arange(N, device=dev)[None, :]


def u_tiled(m, n):
    """the sweep tiled over the output: 67 is coprime to every tile dimension"""
    return (m % NROWS) * 128 + n % 128


def u_hash(m, n):
    """a sweep value per (m, n) with no period in either index (the product terms break every row / column period)"""
    return (m * 7919 + n * 104729 + (m // 7) * (n // 5) + (m * n) % 8191) % NFLAT


def u_bias(n, rep):
    """the main sweep value of column n in launch `rep` of four: (37 n + 11) mod 2048 runs through a quarter of the 64 x 128 values laid flat, 64 columns on are 10 rows
    (binades) on, 128 columns 20"""
    return ((37 * n + 11) % 2048) * 4 + rep


def pm1(shape, seed, density=0.22):
    """entries in {-1, 0, 1}, half the density each sign, from a seeded generator"""
    r = torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)
    return (r < density / 2).double() - (r >= 1 - density / 2).double()


POSITION_SEED = 20


def p8_sweep_case(BM, M=None, K=128):
    """cases 1 and 2.  act 1: A[m][0] = a_(m mod 67), B[n][0] = w_(n mod 128): h = the tiled sweep.  act 2: A2[m][1] = 2^(m mod 3), B2[n][1] = 2^-(n mod 5): the
    accumulator is a power of two that names its row AND its column; H = the tiled sweep from the host; bias2 = BIAS2 (or none)."""
    M, N = M or P8_M[BM], P8_N
    A, B, A2, B2 = (torch.zeros(r, K, dtype=F64) for r in (M, N, M, N))
    A[:, 0] = row_values()[torch.arange(M) % NROWS]
    B[:, 0] = col_values(N)
    A2[:, 1] = 2.0 ** (torch.arange(M) % 3).double()
    B2[:, 1] = 2.0 ** -(torch.arange(N) % 5).double()
    bias2 = torch.zeros(N, dtype=F64)
    for n, v in BIAS2.items():
        bias2[n] = v
    return NS(BM=BM, M=M, N=N, K=K, A=A, B=B, bias=None, A2=A2, B2=B2, bias2=bias2, t1=sweep_table(), t2=sweep_table(), u1=lambda dev="cpu": u_tiled(*grid(M, N, dev)),
              u2=lambda dev="cpu": u_tiled(*grid(M, N, dev)))


def p8_bias_case(BM, rep, M=None, K=128):
    """case 3, act 1 only: A = 0 and bias[n] = the main sweep value u_bias(n, rep), the same in every row"""
    M, N = M or P8_M[BM], P8_N
    n = torch.arange(N)
    return NS(BM=BM, M=M, N=N, K=K, A=torch.zeros(M, K, dtype=F64), B=col_values(N)[:, None].repeat(1, K), bias=sweep_table().h[u_bias(n, rep)], t1=sweep_table(),
              u1=lambda dev="cpu": u_bias(grid(M, N, dev)[1], rep) + 0 * grid(M, N, dev)[0])


def p8_position_case(BM, M=None, K=192):
    """case 4: A, B in {-1, 0, 1} through three k-tiles.  act 1: h = A B^T, an integer and a bf16 value.  act 2: the same product as the accumulator, H = a sweep value
    per (m, n) by u_hash"""
    M, N = M or P8_M[BM], P8_N
    A, B = pm1((P8_M[BM], K), POSITION_SEED)[:M], pm1((N, K), POSITION_SEED + 1)

    def u1(dev="cpu"):
        return (A.to(dev) @ B.to(dev).t()).round().long() + INT_LIM
    return NS(BM=BM, M=M, N=N, K=K, A=A, B=B, bias=None, A2=A, B2=B, bias2=None, t1=int_table(), t2=sweep_table(), u1=u1, u2=lambda dev="cpu": u_hash(*grid(M, N, dev)))


def to_bf16(t):
    return t.float().to(BF).double()


def compare_at(got, want, bound, h, what):
    """`compare` where the output lives: everything on got's device, only a failure's first elements travel.  Returns the worst error / bound (0 / 0 counts as 0)."""
    assert got.shape == want.shape == bound.shape == h.shape, (what, got.shape, want.shape, bound.shape, h.shape)
    g = got.double()
    err = (g - want).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = bad.nonzero()[:6].cpu()
        first = [(int(r), int(k), float(h[r, k]), float(g[r, k]), float(want[r, k])) for r, k in idx.tolist()]
        raise OverBar(f"{what}: {int(bad.sum())} of {bad.numel()} elements over their bar; first (row, col, h, got, want): {first}", first)
    return float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max())


def p8_check_h(c, H, what):
    """act 1: the stored pre-activation equals the table's value bit for bit (check_h's rule for the denormal row: below ABS instead)"""
    t, u = c.t1, c.u1(H.device)
    want, loose = t.h.to(H.device)[u], t.loose.to(H.device)[u]
    got = H.double()
    assert bool(((got == want) | loose).all()), f"{what}: the stored pre-activation is not h"      # (as in check_h, the -0 row may come back +0: 0 + -0 in the accumulator)
    assert not bool(loose.any()) or float(got[loose].abs().max()) <= ABS, what


def p8_check_act1(c, C, what):
    """C against the float64 exact-erf GELU of the table's value under its bar"""
    t, u = c.t1, c.u1(C.device)
    return compare_at(C, t.g.to(C.device)[u], t.bar_g.to(C.device)[u], t.h.to(C.device)[u], what)


def p8_check_act2(c, C, what, bias=None):
    """C against (acc + bias) GELU'(h) in float64: |acc + bias| times the GELU' bar of h, plus half a bf16 ulp of the result (taken, as in `bar`, at |result| + the rest)"""
    dev = C.device
    t, u = c.t2, c.u2(dev)
    acc = c.A2.to(dev) @ c.B2.to(dev).t()
    if bias is not None:
        acc = acc + bias.to(dev)[None, :]
    want = acc * t.dg.to(dev)[u]
    b = acc.abs() * t.bar_dg.to(dev)[u]
    return compare_at(C, want, b + half_ulp_bf16(want.abs() + b), t.h.to(dev)[u], what)


# ---- what a wrong epilogue would store: the form as it stands on operands that took a wrong turn (tests/test_gelu_cases_cpu.py applies each move to every case)
P8_MOVES = ("slot1", "slot2", "chunk64", "chunk128", "bias_wave", "rows16", "bias_order")


def p8_rows(M, BM, move):
    """the row a row's operand comes from"""
    m = torch.arange(M)
    if move == "rows16":                                     # rows r and r + 16 of a staged 32-row half exchanged
        return m ^ 16
    if move in ("slot1", "slot2"):                           # the prefetch slots: half h processed with the H requested for half h + 1 | h + 2 (among the wave's TM / 2)
        W = BM // 2
        r = m % BM
        rr = r % W
        return m - r + (r // W) * W + ((rr // 32 + int(move[-1])) % (W // 32)) * 32 + rr % 32
    return m


def p8_cols(N, move):
    """the column a column's operand comes from"""
    n = torch.arange(N)
    c = n % 256
    if move in ("chunk64", "chunk128"):                      # one lane chunk (columns 88 .. 95 of every tile: wave column 1, lane chunk 3) addressed 64 | 128 columns on
        return torch.where((c >= 88) & (c < 96), n - c + (c + int(move[5:])) % 256, n)
    if move == "bias_wave":                                  # the bias chunk of the next wave column
        return n - c + (c + 64) % 256
    return n


def p8_model(c, act, move=None, bias=None, form="poly"):
    """(C, H) as the epilogue stores them (the restated form, products and sums rounded as fp32 does, then bf16), with one `move` applied.  bias_order: GELU taken of the
    value BEFORE the bias, which is added behind it (act 2: the bias added behind the product)."""
    acc = (c.A @ c.B.t()) if act == 1 else (c.A2 @ c.B2.t())
    b = torch.zeros(c.N, dtype=F64) if bias is None else bias
    if move == "rows16":
        acc = acc[p8_rows(c.M, c.BM, move)]
    if move == "bias_wave":
        b = b[p8_cols(c.N, move)]
    if act == 1:
        pre = (acc + b).float().double()
        H = to_bf16(pre)
        C = emulate(form, acc)[0] + b if move == "bias_order" else emulate(form, pre)[0]
    else:
        H = to_bf16(c.t2.h[c.u2()])
        if move in ("slot1", "slot2"):
            H = H[p8_rows(c.M, c.BM, move)]
        dg = emulate(form, H)[1]
        C = acc * dg + b if move == "bias_order" else (acc + b) * dg
    C = to_bf16(C)
    if move in ("chunk64", "chunk128"):
        C, H = C[:, p8_cols(c.N, move)], H[:, p8_cols(c.N, move)]
    return C, H

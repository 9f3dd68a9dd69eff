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
    """the bound of one activation per element: h, r float64 [R, n] (input and float64 reference), rows the sweep row of each row of h.
    SLOP x E_row x (|h| for GELU, 1 for GELU') + half a bf16 ulp where the kernel rounds + ABS x max(1, |r|).  The half ulp is that of |r| + the rest of the bar, not
    of r alone: the kernel rounds ITS value, which may lie across a power of two from r (up to twice the half ulp of r just under a power of two, and in the tiny
    binades where ABS is all of the bar; docs/gelu_range.md names this as the one departure from the formula the tests were specified with)."""
    e = errors(form)
    E = (e.phi if what == "g" else e.dg)[list(rows)][:, None]
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

"""Test infrastructure: inputs, the float64 reference and the bars of the label-smoothed / class-weighted cross entropy (csrc/loss.hip, include/mvlt_hip_loss.h,
docs/loss_options.md).  tests/test_loss_gpu.py measures the kernels against `smooth_ref`; tests/test_loss_cases_cpu.py pins the premises on the CPU: the
reference IS F.cross_entropy(weight=, ignore_index=, label_smoothing=) in float64, and each of the WRONG formulas below moves it by more than a bar on at least
one case, so a kernel that computes one of them cannot pass.

The generators and the bars are those of tests/rowwise_cases.py (imported, not edited); the tolerances are the project's, rowwise_cases.TOL.

    W = sum_c w_c, p = softmax(x_r), keep_r = [y_r != ignore], den = sum_r keep_r w[y_r]          (no weights: w = 1, W = V, den = the row count)
    loss         = sum_r keep_r [ (1 - e) w[y_r] (lse_r - x[r, y_r]) + (e / V) (W lse_r - sum_c w_c x[r, c]) ] / den
    dlogits[r,k] = keep_r [ (1 - e) w[y_r] (p_k - [k == y_r]) + (e / V) (W p_k - w_k) ] gscale / den         (1 / den = 0 when den == 0)
"""
import torch

from tests import rowwise_cases as rc

BF, F32, NS = rc.BF, rc.F32, rc.NS
IGNORE = -1
PAD_FILL = 1e30                      # what the padding columns [V, ld) hold: a kernel that reads one of them is off by 1e30
SHIFT = 3e4                          # the cancellation rows: W lse and sum_c w_c x_c are ~V 3e4 each, their difference ~V log V

# what a kernel could compute instead (the `wrong` argument of smooth_ref); the CPU file shows that every one of them is exposed
WRONG = ("e_over_ld",                # e / ld instead of e / V
         "sum_over_ld",              # the column sum runs over the padding as well
         "smooth_ignored",           # the smoothing term and its gradient also on ignored rows
         "den_rows",                 # den = the number of kept rows although weights are set
         "label_no_1me",             # the label column's gradient without its (1 - e)
         "W_is_V",                   # W = V although weights are set
         "den_clamped")              # den clamped with max(., 1)

# (V, ld, rows): ld = V and padded; 5 rows at the vocabulary width, 37 at the head widths, 1030 for the finish kernel's stride loop (1024 threads)
SHAPES = ((2, 2, 37), (48, 48, 37), (122, 122, 37), (122, 128, 37), (30522, 30522, 5), (30522, 30528, 5), (48, 48, 1030))
# (tag, e, weights)
OPTIONS = (("e0.1", 0.1, None), ("e0.3", 0.3, None), ("w", 0.0, "rand"), ("e0.1+w", 0.1, "rand"))


def _case(V, ld, rows, tag, e, weights, data="normal", ignored="fifth", backward=True):
    return NS(name=f"V{V}-ld{ld}-r{rows}-{data}-{tag}" + ("" if ignored == "fifth" else f"-{ignored}"), V=V, ld=ld, rows=rows, e=e, weights=weights, data=data,
              ignored=ignored, backward=backward)


CASES = [_case(V, ld, rows, *opt) for V, ld, rows in SHAPES for opt in OPTIONS]
# every row ignored: the loss is NaN and the gradient all zero
CASES += [_case(122, 128, 37, "e0.1+w", 0.1, "rand", ignored="all"), _case(48, 48, 37, "e0.1", 0.1, None, ignored="all")]
# weights that sum below 1 over the batch: den < 1 is legitimate, a clamp max(den, 1) is wrong by 1 / den
CASES += [_case(48, 48, 37, "e0.1+tiny", 0.1, "tiny"), _case(122, 128, 37, "tiny", 0.0, "tiny")]
# a late maximum (the last column) and all-equal rows, as for the plain kernels
CASES += [_case(122, 128, 37, "e0.1+w", 0.1, "rand", data="peaked"), _case(30522, 30528, 5, "e0.1", 0.1, None, data="peaked"),
          _case(2, 2, 37, "e0.3", 0.3, None, data="flat"), _case(122, 122, 37, "e0.1+w", 0.1, "rand", data="flat")]
# cancellation: logits near 3e4.  The FORWARD is judged (lse, the row's smoothing term, the loss).  The backward reads lse as an fp32 number, whose half ulp at
# 3e4 is 1e-3 -- every probability it forms carries that relative error, as in the plain ce_bwd_kernel; it is not judged on these rows.
SHIFTED = [_case(V, ld, rows, tag, 0.1, w, data="shifted", backward=False)
           for V, ld, rows in SHAPES[:6] for tag, w in (("e0.1", None), ("e0.1+w", "rand"))]
CASES += SHIFTED
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def weights_of(case):
    if case.weights is None:
        return None
    w = 0.5 + 1.5 * torch.rand(case.V, generator=rc.gen(4242 + case.V))           # uniform on [0.5, 2): mean 1.25, so W != V and den != the row count
    return w * 1e-3 if case.weights == "tiny" else w


def build(case):
    """-> namespace(x [rows, ld] fp32 with PAD_FILL in the padding columns, labels int64 [rows], weight fp32 [V] or None); CPU tensors"""
    V, rows = case.V, case.rows
    seed = 7 + V + rows
    if case.data == "normal":
        x, lab = rc.ce_shifted_rows(rows, V, 0.0, seed=seed)
    elif case.data == "shifted":
        x, lab = rc.ce_shifted_rows(rows, V, SHIFT, seed=seed)
    elif case.data == "peaked":
        x, lab = rc.ce_peaked_rows(rows, V, V - 1, seed=seed)
    else:
        x, lab = rc.ce_flat_rows(rows, V, seed=seed)
    lab = lab.clone()
    if case.ignored == "all":
        lab[:] = IGNORE
    else:
        lab[torch.arange(rows) % 5 == 2] = IGNORE                                 # a fifth of the rows
    full = torch.full((rows, case.ld), PAD_FILL, dtype=F32)
    full[:, :V] = x
    return NS(x=full, labels=lab, weight=weights_of(case))


def smooth_ref(x_full, labels, V, weight=None, ignore=IGNORE, e=0.0, gscale=1.0, wrong=None):
    """THE REFERENCE, float64, on whatever device the operands live on.  x_full [rows, ld] with its padding columns (only `wrong` formulas look at them).
    -> namespace(lse [rows], smooth [rows] = W lse - sum_c w_c x_c, num, den, W, loss (NaN when den == 0), dlogits [rows, V])"""
    assert wrong is None or wrong in WRONG
    ld = x_full.shape[1]
    x = x_full[:, :V].double()
    w = torch.ones(V, dtype=torch.float64, device=x.device) if weight is None else weight.double()
    W = float(V) if wrong == "W_is_V" else w.sum()
    lse = torch.logsumexp(x, -1)
    keep = (labels != ignore).double()
    y = torch.where(labels != ignore, labels, torch.zeros_like(labels))
    wy = w[y]
    nll = lse - x.gather(1, y[:, None])[:, 0]
    sum_wx = (w * x).sum(-1)
    if wrong == "sum_over_ld":
        sum_wx = sum_wx + x_full[:, V:].double().sum(-1)
    smooth = W * lse - sum_wx
    ev = e / (ld if wrong == "e_over_ld" else V)
    keep_s = torch.ones_like(keep) if wrong == "smooth_ignored" else keep
    num = (keep * (1 - e) * wy * nll).sum() + (keep_s * ev * smooth).sum()
    den = keep.sum() if wrong == "den_rows" else (keep * wy).sum()
    if wrong == "den_clamped":
        den = den.clamp_min(1.0)
    inv = 1.0 / den if float(den) > 0 else torch.zeros_like(den)
    p = (x - lse[:, None]).exp()
    onehot = torch.zeros_like(p).scatter_(1, y[:, None], 1.0)
    c_label = 1.0 if wrong == "label_no_1me" else 1 - e
    d = (keep * wy)[:, None] * ((1 - e) * p - c_label * onehot) + keep_s[:, None] * ev * (W * p - w)
    return NS(lse=lse, smooth=smooth, num=num, den=den, W=torch.as_tensor(W, dtype=torch.float64), loss=num / den, dlogits=d * (rc.f32(gscale) * inv))


def case_ref(case, inputs, gscale=1.0, wrong=None):
    return smooth_ref(inputs.x, inputs.labels, case.V, weight=inputs.weight, e=case.e, gscale=gscale, wrong=wrong)


# ---- bars: rowwise_cases' own, no new constants
def bar_row(ref_rows, t):
    """lse and the row's smoothing term: per row, TOL x max(|ref|, 1) -- rowwise_cases.bar_lse"""
    return rc.bar_lse(ref_rows, t)


def bar_loss(ref_loss, t):
    """the mean loss: TOL x max(|ref|, 1), as tests/test_rowwise_edges_gpu.py judges the plain one"""
    return t * max(1.0, abs(float(ref_loss)))


def bar_dlogits(ref, t, gscale, out_dtype):
    """rowwise_cases.bar_dlogits with den in the place of the count: TOL x gscale / max(den, 1) per element (+ half a bf16 ulp for a bf16 output).  Where
    den < 1 this is tighter than TOL x gscale / den."""
    return rc.bar_dlogits(ref.dlogits, t, gscale, float(ref.den), out_dtype)


def exposed(case, inputs, wrong, t=rc.TOL[F32], gscale=1.0):
    """does `wrong` move the float64 reference of this case past a bar (the loss, a row's smoothing term or an element of dlogits)?"""
    good, bad = case_ref(case, inputs, gscale), case_ref(case, inputs, gscale, wrong)
    if float(good.den) > 0:
        dl = bool(((bad.loss - good.loss).abs() > bar_loss(good.loss, t)) | ~torch.isfinite(bad.loss))
    else:
        dl = bool(torch.isfinite(bad.loss))
    ds = case.e > 0 and bool(((bad.smooth - good.smooth).abs() > bar_row(good.smooth, t)).any())
    dg = bool(((bad.dlogits - good.dlogits).abs() > bar_dlogits(good, t, gscale, F32)).any() or not bool(torch.isfinite(bad.dlogits).all()))
    return dl or ds or dg

"""Test infrastructure: inputs, float64 references and bars of the row-wise kernel tests (tests/test_rowwise_edges_gpu.py; the premises of
the inputs are pinned on the CPU by tests/test_rowwise_cases_cpu.py).  The kernels: csrc/norm.hip (LayerNorm forward / backward) and, in
csrc/elementwise.hip, bert_embed_*, ce_fwd / ce_loss_finish / ce_bwd and the two SmoothL1 kernels.

Plain torch, on whatever device the operands live on.  Every reference is float64 and is computed from the operands AS THE KERNEL READS THEM:
a bf16 operand is rounded first and widened afterwards, the row statistics a backward is handed are the fp32 values it is handed, eps is the
fp32 value of the C ABI.  N(0,1) data under one global maximum hides whole classes of wrong kernels; each builder below says which one it
is there to expose.
"""
import math
import types

import torch

BF, F32 = torch.bfloat16, torch.float32
TOL = {F32: 1e-3, BF: 2e-2}                    # the project's parity bars (tests/test_kernels_gpu.py, tests/test_attention_edges_gpu.py)
HID = 768                                      # bert-base hidden size: the only width of the embedding kernels
NS = types.SimpleNamespace

# ---- shapes shared by the GPU file and the CPU premises
LN_FIXED = (64, 128, 320, 512, 768)            # ln_fwd_fixed_kernel
LN_GENERIC = (8, 72, 192, 256, 1000, 1024)     # ln_fwd_kernel: G = 8 (seven idle lanes), 8 (ragged second chunk), 16, 32, 64 (ragged), 64 (full)
LN_BWD_WIDTHS = LN_FIXED + (8, 72, 256, 1024)
LN_FACTORS = (1e-4, 1e-3, 1e-2, 1.0, 1e2, 1e4)
LN_CONSTANTS = (1.0, 3.0, -4.0)
CE_SHAPES = ((2, 8), (122, 128), (123, 125), (8195, 8196), (30522, 30528))        # (V, ld); (123, 125): the fp32 scalar fallback
CE_PEAKS = (0, 3, 4, 1023 * 4, 8191, 8192, "V4-1", "V4", "V-1")
BERT_SHAPES = ((1, 5), (20, 17), (20, 40), (200, 33), (512, 2))                  # (T, batch)
SL1_N = 7 * 2 ** 20 + 148
SL1_DIFFS = (0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 3.0, -3.0)


def tol(*dtypes):
    """a case is judged against the bar of the narrowest dtype it reads or writes"""
    return TOL[BF] if BF in dtypes else TOL[F32]


def f32(v):
    """a Python float as the C ABI passes it (float)"""
    return float(torch.tensor(v, dtype=F32))


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def pick_group(C):
    """lanes per row of ln_fwd_kernel / ln_bwd_kernel (csrc/norm.hip pick_group)"""
    chunks, g = C // 8, 8
    while g < 64 and g * 2 <= chunks:
        g *= 2
    while g * 2 < chunks and g < 64:
        g *= 2
    return g


def ln_bwd_threshold(C):
    """rows one launch of ln_bwd_kernel covers without its grid-stride loop: 256 workgroups x (1024 / G) row groups"""
    return 256 * (1024 // pick_group(C))


def phys_rows(rows, rmap=None):
    """physical row of every logical row under a mode-0 row map (rows_per_batch, batch_stride, offset); None: the identity"""
    r = torch.arange(rows)
    if rmap is None:
        return r
    rpb, stride, off = rmap
    return (r // rpb) * stride + off + r % rpb


# ================================================================================================ float64 references
def ln_fwd_ref(x, gamma, beta, eps, add=None, add_rows=0, chain=None):
    """-> namespace(y, mean, rstd, std[, y2, mean2, rstd2, std2]); add: fp32 [add_rows, C] added to row r % add_rows after the affine;
    chain = (gamma2, beta2, eps2): the second LayerNorm of the UNROUNDED first output, as the kernel chains it from its registers"""
    x = x.double()
    mean = x.mean(-1)
    d = x - mean[:, None]
    var = (d * d).mean(-1)
    rstd = (var + f32(eps)).rsqrt()
    y = d * rstd[:, None] * gamma.double() + beta.double()
    if add is not None:
        y = y + add.double()[torch.arange(x.shape[0], device=x.device) % add_rows]
    out = NS(y=y, mean=mean, rstd=rstd, std=var.sqrt())
    if chain is not None:
        second = ln_fwd_ref(y, chain[0], chain[1], chain[2])
        out.y2, out.mean2, out.rstd2, out.std2 = second.y, second.mean, second.rstd, second.std
    return out


def ln_bwd_ref(dy, x, gamma, mean, rstd):
    """-> namespace(dx, dgamma, dbeta, abs_gamma, abs_beta); abs_* = per column sum over the rows of |dy x_hat| and |dy|: what the column
    gradients are sums OF, so that their bars know about cancellation"""
    dy, x, g = dy.double(), x.double(), gamma.double()
    xh = (x - mean.double()[:, None]) * rstd.double()[:, None]
    gg = dy * g
    s1, s2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    dx = rstd.double()[:, None] * (gg - s1 - xh * s2)
    t = dy * xh
    return NS(dx=dx, dgamma=t.sum(0), dbeta=dy.sum(0), abs_gamma=t.abs().sum(0), abs_beta=dy.abs().sum(0))


def bert_embed_x(ids, word, pos, type0, T):
    ids = ids.reshape(-1)
    t = torch.arange(ids.numel(), device=ids.device) % T
    return word.double()[ids] + type0.double() + pos.double()[t], t


def bert_fwd_ref(ids, word, pos, type0, gamma, beta, eps, T, keep=None, drop_p=0.0):
    """y = dropout(LN(word[ids] + type0 + pos[t])) -> namespace(y, mean, rstd, std); keep: uint8 [rows, 768] or None"""
    x, _ = bert_embed_x(ids, word, pos, type0, T)
    out = ln_fwd_ref(x, gamma, beta, eps)
    if keep is not None:
        out.y = out.y * keep.double() * (1.0 / (1.0 - f32(drop_p)))
    return out


def bert_bwd_ref(dy, ids, word, pos, type0, gamma, mean, rstd, T, keep=None, drop_p=0.0):
    """-> namespace(dword [V,768] (row 0 = PAD stays zero), dpos [512,768], dtype0, dgamma, dbeta, abs_gamma, abs_beta, abs_type0)"""
    x, t = bert_embed_x(ids, word, pos, type0, T)
    d = dy.double()
    if keep is not None:
        d = d * keep.double() * (1.0 / (1.0 - f32(drop_p)))
    r = ln_bwd_ref(d, x, gamma, mean, rstd)
    flat = ids.reshape(-1)
    dword = torch.zeros(word.shape, dtype=torch.float64, device=d.device).index_add_(0, flat, r.dx * (flat != 0)[:, None])
    dpos = torch.zeros(pos.shape, dtype=torch.float64, device=d.device).index_add_(0, t, r.dx)
    return NS(dword=dword, dpos=dpos, dtype0=r.dx.sum(0), abs_type0=r.dx.abs().sum(0), dgamma=r.dgamma, dbeta=r.dbeta,
              abs_gamma=r.abs_gamma, abs_beta=r.abs_beta)


def ce_ref(logits, labels, ignore=-1, gscale=1.0, count=None):
    """-> namespace(lse [rows], loss_sum, count, dlogits [rows, V]); count: the divisor of the gradient when it comes from another call"""
    x = logits.double()
    lse = torch.logsumexp(x, -1)
    valid = labels != ignore
    picked = x.gather(1, labels.clamp_min(0)[:, None])[:, 0]
    loss_sum = torch.where(valid, lse - picked, torch.zeros_like(lse)).sum()
    n = int(valid.sum())
    div = max(float(n if count is None else count), 1.0)
    p = (x - lse[:, None]).exp()
    onehot = torch.zeros_like(p).scatter_(1, labels.clamp_min(0)[:, None], 1.0)
    dl = torch.where(valid[:, None], (p - onehot) * (f32(gscale) / div), torch.zeros_like(p))
    return NS(lse=lse, loss_sum=float(loss_sum), count=n, dlogits=dl)


def sl1_ref(pred, target, gscale=1.0):
    d = pred.double() - target.double()
    a = d.abs()
    return NS(loss_sum=float(torch.where(a < 1, 0.5 * d * d, a - 0.5).sum()), grad=d.clamp(-1, 1) * (f32(gscale) / d.numel()))


# ================================================================================================ bars (float64 tensors, one per row / column / element)
def bar_y(ref, t):
    """LayerNorm y: per element, TOL x max|ref| over the row"""
    return t * ref.abs().amax(-1, keepdim=True)


def bar_mean(ref, t):
    return t * torch.maximum(ref.mean.abs(), ref.std)


def bar_dx(ref_dx, t):
    """LayerNorm dx (and the rows of the embedding tables' gradients): per element, 2 TOL x max|ref| over the row"""
    return 2 * t * ref_dx.abs().amax(-1, keepdim=True)


def bar_col(abs_terms, t):
    """dgamma, dbeta: TOL x the column's sum of absolute terms"""
    return t * abs_terms


def bar_lse(ref_lse, t):
    return t * ref_lse.abs().clamp_min(1.0)


def bf16_half_ulp(v):
    """half a bf16 ulp of every element of v (8 significant bits): 2^(floor(log2|v|) - 8); the smallest normal's for zero"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 8)


def bar_dlogits(ref, t, gscale, count, out_dtype):
    b = torch.full_like(ref, t * f32(gscale) / max(float(count), 1.0))
    return b + bf16_half_ulp(ref) if out_dtype == BF else b


# ================================================================================================ LayerNorm inputs
# ln_offset_rows: every value is exact in bf16 (253, 254, 255: eight significant bits -- the largest offset / step ratio bf16 holds) and every fp32
# partial sum of a row is exact (integers below 2^24).  One value in sixteen leaves the offset, so the variance is ~1/24 against a squared mean of 64516.
OFFSET_C0, OFFSET_S, OFFSET_SPARSITY = 254.0, 1.0, 16
LN_OFFSET_WIDTHS = tuple(C for C in sorted(set(LN_FIXED + LN_GENERIC)) if C != 8)


def ln_offset_rows(rows, C, seed=0):
    """x = 254 + k, k in {-1, 0, 1}, mostly 0.  Exposes a ONE-PASS variance E[x^2] - mean^2: in fp32 the two terms agree to ~2^-24 x 254^2 = 4e-3, the
    size of the variance itself, so y is off by many bars, while the two-pass kernel stays below 2e-5 of the row maximum.  N(0.5, 2) data has nothing to
    cancel.  (300 +- 2 and 1200 +- 8 are the same floating-point problem, scaled by a power of two where the ratio is equal; on dense k they stay within
    ONE bar at C = 64, 128, 256 and 512, whose fp32 mean is exact.)  Not for C = 8: x^2 has 16 bits, a row's sums 19 and mean^2 22 -- a one-pass
    variance is exact on any bf16-exact data of one binade, there is nothing to expose (tests/test_rowwise_cases_cpu.py pins that as well)."""
    g = gen(seed)
    k = torch.randint(-1, 2, (rows, C), generator=g).float() * (torch.randint(0, OFFSET_SPARSITY, (rows, C), generator=g) == 0)
    k[:, 0], k[:, 1] = -1.0, 1.0                           # no row is constant
    return OFFSET_C0 + OFFSET_S * k


def ln_constants(C):
    """row values whose fp32 mean (sum x fl(1 / C)) is exactly the value again; 3 is not at C = 1000"""
    return (1.0, 5.0, -4.0) if C == 1000 else LN_CONSTANTS


def ln_constant_rows(rows, C):
    """row r holds the one value ln_constants(C)[r % 3].  The fp32 mean is then exactly that value, every x - mean exactly 0, so y == beta bit for bit,
    mean == c and rstd == 1 / sqrt(eps): the only input on which eps is ALL of the denominator -- a kernel that drops eps returns inf / NaN, one that
    swaps eps and eps2 in the chained norm is off by sqrt(eps / eps2) in rstd2."""
    c = torch.tensor(ln_constants(C))[torch.arange(rows) % 3]
    return c[:, None].expand(rows, C).contiguous()


def ln_scaled_rows(rows, C, seed=0):
    """row r of N(0,1) times LN_FACTORS[r % 6] (1e-4 .. 1e4).  At 1e-3 and eps = 1e-6 the variance IS about eps, at 1e-4 eps is 100 x the variance: a
    kernel that ignores eps is wrong by 40 % / 10 x there.  Per-row dx spans eight decades, so a row with large x whose dx is entirely wrong no
    longer hides under the global maximum that the rows of small x set -- the bars are per row."""
    f = torch.tensor(LN_FACTORS)[torch.arange(rows) % 6]
    return torch.randn(rows, C, generator=gen(seed)) * f[:, None]


def ln_single_row_dy(rows, C, row, seed=0):
    """dy non-zero in ONE row: dgamma / dbeta are that row's dy x_hat / dy and nothing else (a column sum that takes x_hat, mean or rstd from a
    neighbouring row, or drops / doubles the rows of a grid-stride pass, is wrong by 100 %), every other row's dx is exactly 0 and, with
    `accumulate`, keeps its bits."""
    dy = torch.zeros(rows, C)
    dy[row] = torch.randn(C, generator=gen(seed))
    return dy


def ln_params(C, seed=0):
    g = gen(seed + 1000)
    return 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


# ================================================================================================ cross-entropy inputs
def ce_peak_column(peak, V):
    """a CE_PEAKS entry as a column of a V-wide row, None where the row is too narrow for it"""
    V4 = V & ~3
    col = {"V4-1": V4 - 1, "V4": V4, "V-1": V - 1}.get(peak, peak)
    return col if 0 <= col < V else None


def ce_labels(rows, V, avoid=None, seed=0, finite=None):
    """labels drawn from the columns (of `finite` [rows, V] bool when given); `avoid` [rows]: a column the row's label must not be"""
    g = gen(seed + 77)
    if finite is not None:
        w = finite.float()
        return torch.multinomial(w, 1, generator=g)[:, 0]
    lab = torch.randint(0, V, (rows,), generator=g)
    if avoid is not None and V > 1:
        lab = torch.where(lab == avoid, (lab + 1) % V, lab)
    return lab


def ce_peaked_rows(rows, V, col, seed=0):
    """N(0,1) clamped to +-3 with ONE column at 33: 30 above everything else, so lse = 33 + O(V e^-30).  The column is placed where a maximum
    can arrive late: behind the first vector, in a later trip, in the last vector column, in the scalar tail.  Exposes a log-sum-exp whose
    running sum is not rescaled when a later chunk raises the maximum (lse off by log of the earlier partial sum), and one that drops the
    scalar tail columns or the last vector (lse off by ~30).  The label sits on the peak in the even rows (loss ~ 0) and elsewhere in the odd ones (loss ~ 33).
    -> (logits fp32 [rows, V], labels)"""
    x = torch.randn(rows, V, generator=gen(seed)).clamp_(-3, 3)
    x[:, col] = 33.0
    peak = torch.full((rows,), col)
    lab = torch.where(torch.arange(rows) % 2 == 0, peak, ce_labels(rows, V, avoid=peak, seed=seed))
    return x, lab


def ce_shifted_rows(rows, V, shift, seed=0):
    """3 N(0,1) + shift, shift = +-100 (exact in bf16).  exp(100) overflows fp32 and exp(-100) underflows it: a log-sum-exp WITHOUT the maximum
    subtracted returns +inf / -inf where the right one returns shift + lse(3 N(0,1))."""
    x = 3 * torch.randn(rows, V, generator=gen(seed)) + shift
    return x, ce_labels(rows, V, seed=seed)


def ce_flat_rows(rows, V, value=-2.5, seed=0):
    """all logits equal: lse = value + log V and every probability 1 / V in closed form -- a column counted twice or not at all moves lse by
    log((V +- 1) / V), which at V = 2 is 40 % of the loss"""
    return torch.full((rows, V), value), ce_labels(rows, V, seed=seed)


def ce_masked_rows(rows, V, mode, seed=0):
    """3 N(0,1) with -inf columns (masked classes, as F.cross_entropy accepts them): "first4" columns 0..3, "first8192" columns 0..8191 -- every value
    a thread sees in its first vector / first unrolled trip is -inf --, "random30" a random 30 % per row (never all).  Exposes exp(x - max) evaluated
    while the running maximum is still -inf (NaN in lse).  The label is on a finite column.  -> (logits, labels)"""
    g = gen(seed)
    x = 3 * torch.randn(rows, V, generator=g)
    masked = torch.zeros(rows, V, dtype=torch.bool)
    if mode == "first4":
        masked[:, :4] = True
    elif mode == "first8192":
        masked[:, :8192] = True
    else:
        masked = torch.rand(rows, V, generator=g) < 0.3
        masked[torch.arange(rows), torch.randint(0, V, (rows,), generator=g)] = False
    assert bool((~masked).any(-1).all()), "every row needs a finite column"
    x[masked] = -math.inf
    return x, ce_labels(rows, V, seed=seed, finite=~masked)


# ================================================================================================ SmoothL1 inputs
def sl1_exact(seed=0, n=SL1_N):
    """pred - target in {0, +-0.5, +-1, +-1.5, +-3}, about 1/16 of them non-zero, n = 7 x 2^20 + 148 (past the 4x-unrolled main loop's threshold
    of 3 x 2048 x 1024, with a ragged last pass).  Every loss term is a multiple of 0.125, the total stays below 2^21, so every partial sum is exact in
    fp32 in ANY order of addition: loss_sum must be bit-equal.  Exposes elements skipped or counted twice between the unrolled and the tail loop, and a
    branch taken wrongly at |d| = 0.5, 1, 1.5.  -> (pred, target) fp32 [n]"""
    g = gen(seed)
    target = torch.randint(-8, 9, (n,), generator=g).float()
    pick = torch.randint(0, 16 * len(SL1_DIFFS), (n,), generator=g)
    d = torch.where(pick < len(SL1_DIFFS), torch.tensor(SL1_DIFFS)[pick % len(SL1_DIFFS)], torch.zeros(n))
    return target + d, target


def sl1_boundary_values():
    one = torch.tensor(1.0)
    below, above = float(torch.nextafter(one, torch.tensor(0.0))), float(torch.nextafter(one, torch.tensor(2.0)))
    return [0.0, -0.0, 1.0, -1.0, below, -below, above, -above, 1e30, -1e30, 1e-40, -1e-40]


def sl1_boundaries(d, n=1024, at=517):
    """one difference d in an otherwise all-equal pair: loss_sum is that element's loss, the gradient is non-zero in one place.  d walks the
    branch point |d| = 1 from both sides, the signed zeros, a huge value and an fp32 denormal.  -> (pred, target) fp32 [n]"""
    target = torch.linspace(-2, 2, n)
    pred = target.clone()
    target[at] = 0.0
    pred[at] = d
    return pred, target


# ================================================================================================ BERT-embedding inputs
def bert_tables(V, seed=0):
    g = gen(seed)
    r = lambda *s: 0.1 * torch.randn(*s, generator=g)
    gamma, beta = ln_params(HID, seed)
    return NS(word=r(V, HID), pos=r(512, HID), type0=r(HID), gamma=gamma, beta=beta, V=V)


def bert_ids(T, batch, V, layout, seed=0):
    """"mixed": random ids with V - 1 present and a PAD tail per sample; "same": every token the one id 5; "pad": every token PAD (id 0)"""
    if layout == "same":
        return torch.full((batch, T), 5)
    if layout == "pad":
        return torch.zeros(batch, T, dtype=torch.long)
    ids = torch.randint(1, V, (batch, T), generator=gen(seed))
    ids[:, T - T // 4:] = 0
    ids[0, 0] = V - 1
    return ids

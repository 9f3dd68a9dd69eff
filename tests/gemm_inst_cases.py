"""Test infrastructure: one exact integer-data case for every compiled GEMM instantiation that no bench shape and no other test reaches
(tests/test_gemm_inst_gpu.py launches them; tests/test_gemm_inst_cpu.py pins their plans and premises without a GPU), and the helpers of the exact GEMM
tests (tests/test_exact_gpu.py imports them back from here).  docs/gemm_instantiations.md has the table.

A case is (id, group, kernel, make): `kernel` is the instantiation the case claims, as mvlt_gemm_plan_name prints it; make(perturb=None) builds the operands
on dev() and returns the call and what to compare:

  t.op, t.args, t.kw   the ops.gemm_nt / ops.gemm_tn call (ops.gemm_nt_plan / gemm_tn_plan take the same arguments: plan(t))
  t.outs               [(what, got: () -> tensor, float64 reference, bound or None, gelu)]: gelu False = exact(), bit for bit; gelu True = mlp_cases.compare()
                       with the derived off-side bound (None: equal)
  t.guards             [(what, () -> bool tensor)]: guard rows, guard columns and rows the maps do not reach keep their fill

All operands are small integers, every reference an integer (or a multiple of 0.5 under a row factor) below 2^24: fp32 accumulation is exact in any order.
make(perturb=...) builds the reference the way a wrong kernel would compute it ("halo": one gathered row read from the zero page, "w_out": the scatter map's
w_out off by one, "factor": a sample's row factor taken from its neighbour, "r_twice": the residual added twice): the CPU test shows that the comparison fails.
"""
import contextlib
import types

import torch

from tests import mlp_cases as mc

BF, F32, F16, F64 = torch.bfloat16, torch.float32, torch.float16, torch.float64
LIM = float(2 ** 24)
NS = types.SimpleNamespace

_DEVICE = []                  # on_device() pushes here; empty: the GPU


def dev():
    if _DEVICE:
        return _DEVICE[-1]
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@contextlib.contextmanager
def on_device(device):
    """build the operands of the cases on `device` (the CPU test: torch.device("cpu")) instead of the GPU"""
    _DEVICE.append(torch.device(device))
    try:
        yield
    finally:
        _DEVICE.pop()


def last_kernel():
    from mvlt_amd._lib import last_kernel as lk
    return lk()


def ran(family):
    """the kernel launched last on this thread must be of `family`: a prefix of the demangled instantiation name.  (Instantiations over the bf16 element type come
    back mangled where the C++ runtime's demangler does not know that type: the kernel's name and the type code are looked up in the mangled form then.)"""
    name = last_kernel()
    if name.startswith("_Z"):
        base = family.split("<")[0]
        assert f"{len(base)}{base}I" in name and "DF16b" in name and "<float" not in family, f"meant to reach {family}, the library launched {name}"
        return
    assert name.startswith(family), f"meant to reach {family}, the library launched {name}"


def ints(shape, lo, hi, dtype, seed):
    """uniform integers in [lo, hi] from a seeded CPU generator, cast to `dtype`, on the device"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(dev())


def picks(shape, values, seed):
    """fp32 entries drawn uniformly from `values` (the DropPath factors {0, 0.5, 1, 2})"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.tensor(values, dtype=F32)[torch.randint(0, len(values), shape, generator=g)].to(dev())


def sparse_pm1(M, N, P, dtype, seed):
    """[M, N] with +-1 exactly where n % P == m % P: every column holds at most ceil(M / P) nonzero rows and (for N >= P) every row at least one"""
    sign = ints((M, N), 0, 1, F32, seed) * 2 - 1
    m = torch.arange(M, device=dev())[:, None] % P
    n = torch.arange(N, device=dev())[None, :] % P
    return (sign * (m == n)).to(dtype)


def integral(ref64, unit=1.0):
    """the reference must be exact in fp32: whole multiples of `unit` (a power of two) below 2^24 units"""
    q = ref64 / unit
    assert torch.equal(q, q.round()) and float(q.abs().max()) < LIM, "the reference is not an integer below 2^24: the case itself is wrong"
    return ref64


def exact(out, ref64, what=""):
    """fp32 out: equal to the float64 reference; bf16 / fp16 out: the reference rounded once to nearest-even"""
    assert out.shape == ref64.shape, (out.shape, ref64.shape)
    if out.dtype == F32:
        got, want = out.double(), ref64
    else:
        got, want = out, ref64.float().to(out.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want).reshape(got.shape[0], -1) if got.dim() > 1 else (got != want).reshape(-1, 1)
    g2, w2 = got.reshape(bad.shape), want.reshape(bad.shape)
    idx = bad.nonzero()
    first = [(int(r), int(c), float(g2[r, c]), float(w2[r, c])) for r, c in idx[:8].tolist()]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong; first (row, col, got, want): {first}; rows {int(idx[:, 0].min())}..{int(idx[:, 0].max())}, "
                         f"cols {int(idx[:, 1].min())}..{int(idx[:, 1].max())}; last kernel {last_kernel()}")


def pad_cols(t, ld, fill=0):
    out = torch.full((t.shape[0], ld), fill, device=t.device, dtype=t.dtype)
    out[:, : t.shape[1]] = t
    return out


def phys_rows(n_batch, rows, stride, off):
    return (torch.arange(n_batch, device=dev())[:, None] * stride + off + torch.arange(rows, device=dev())[None, :]).reshape(-1)


def gather_patch(X, Bsz, r, h_out, w_out, tokens_in):
    """mode-1 operand as a matrix: row (b, oi, oj), column (di*r + dj)*C + c = X[b*tokens_in + (oi*r+di)*w_in + oj*r+dj, c]"""
    Cs, w_in = X.shape[-1], r * w_out
    img = X.reshape(Bsz, tokens_in, Cs)[:, : h_out * r * w_in].reshape(Bsz, h_out, r, w_out, r, Cs)
    return img.permute(0, 1, 3, 2, 4, 5).reshape(Bsz * h_out * w_out, r * r * Cs)


def gather_3x3(X, Bsz, h, w, tokens_in):
    """mode-2 operand as a matrix: row (b, y, x), column (dy*3 + dx)*C + c = X[b, (y+dy-1)*w + x+dx-1, c], zero outside the grid"""
    Cs = X.shape[-1]
    img = X.reshape(Bsz, tokens_in, Cs)[:, : h * w].reshape(Bsz, h, w, Cs)
    pad = torch.zeros(Bsz, h + 2, w + 2, Cs, device=X.device, dtype=X.dtype)
    pad[:, 1:-1, 1:-1] = img
    taps = [pad[:, dy: dy + h, dx: dx + w] for dy in range(3) for dx in range(3)]
    return torch.stack(taps, 3).reshape(Bsz * h * w, 9 * Cs)


# ---------------------------------------------------------------------------------------------------------------- plans without a device
class Placeholder:
    """stands for a device tensor in ops.gemm_nt_plan / gemm_tn_plan: dtype and shape of the real one and an address of its own (the plan never follows a pointer)"""
    is_cuda = True

    def __init__(self, t, addr):
        self.dtype, self.shape, self._strides, self._addr, self._n, self._es = t.dtype, tuple(t.shape), tuple(t.stride()), addr, t.numel(), t.element_size()

    def data_ptr(self):
        return self._addr

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n

    def element_size(self):
        return self._es


def plan(t):
    """what the case's call would launch: ops.gemm_nt_plan / gemm_tn_plan on placeholder pointers (one address per tensor object, so R aliasing C stays an alias)"""
    from mvlt_amd import ops
    seen = {}

    def ph(v):
        if not isinstance(v, torch.Tensor):
            return v
        if id(v) not in seen:
            seen[id(v)] = Placeholder(v, 0x10000000 * (len(seen) + 1))
        return seen[id(v)]
    fn = ops.gemm_nt_plan if t.op == "nt" else ops.gemm_tn_plan
    return fn(*[ph(v) for v in t.args], **{k: ph(v) for k, v in t.kw.items()})


def launch(ops, t):
    (ops.gemm_nt if t.op == "nt" else ops.gemm_tn)(*t.args, **t.kw)


def check(t):
    """every output against its reference, then the guards"""
    for what, got, ref, bound, gelu in t.outs:
        if gelu:
            mc.compare(got(), ref, bound, what)
        else:
            exact(got(), ref, what)
    for what, ok in t.guards:
        assert bool(ok().all()), f"{what}: written outside the output"


def rounded(ref, like):
    """the float64 reference as a kernel that is right would store it: rounded once to the output's type"""
    return ref.float().to(like.dtype)


def guarded(rows, cols, dtype, fill=7.0):
    """[rows + 1, cols + 8]: one guard row and eight guard columns behind the rows x cols output"""
    return torch.full((rows + 1, cols + 8), fill, device=dev(), dtype=dtype)


def std_guards(buf, rows, cols, fill=7.0):
    return [("guard row", lambda: buf[rows] == fill), ("guard columns", lambda: buf[:, cols:] == fill)]


# ---------------------------------------------------------------------------------------------------------------- the gathered operands
# (the HAND structs of tests/test_gemm_plan_cpu.py: K = 64 behind the 2x2 patch gather, K = 576 behind the 3x3 gather; the grids are made non-square and
#  M ragged: 175 = 128 + 47 rows behind the patch gather, 180 = 128 + 52 behind the 3x3 gather)
PATCH = NS(r=2, h_out=5, w_out=7, c=16, T=3, B=5)
CONV = NS(h=5, w=12, c=64, T=5, B=3)
TEXT = 99                     # what the text tokens behind the image tokens hold: never read


def _operand(rows, c, lo, hi, seed, sparse):
    return sparse_pm1(rows, c, 16, BF, seed) if sparse else ints((rows, c), lo, hi, BF, seed)


def conv_operand(h, w, c, B, T, *, lo=-3, hi=3, seed=0, sparse=False, nz=None, zero_y=1):
    """a_map / b_map mode 2 over B images of h x w pixels with T text tokens behind each.  .zero: the rows of image 1's pixel row `zero_y` and the columns of their
    dy = 0 taps, i.e. what that row reads from the pixel row above it"""
    from mvlt_amd._lib import conv3map
    tokens = h * w + T
    X = _operand(B * tokens, c, lo, hi, seed, sparse).reshape(B, tokens, c)
    if nz is not None:
        X[:, :, nz:] = 0
    X[:, h * w:] = TEXT
    X = X.reshape(B * tokens, c)
    return NS(X=X, G=gather_3x3(X, B, h, w, tokens).double(), amap=conv3map(h, w, tokens, c), M=B * h * w, K=9 * c, lda=c, rpi=h * w, B=B,
              zero=(slice(h * w + zero_y * w, h * w + (zero_y + 1) * w), slice(0, 3 * c)))


def patch_operand(*, lo=-3, hi=3, seed=0, sparse=False):
    """a_map / b_map mode 1, PATCH's grid.  .zero: image 1's output row 1 and the columns of its di = 0 input row"""
    from mvlt_amd._lib import patchmap
    p = PATCH
    hw_in = p.r * p.h_out * p.r * p.w_out
    tokens, rpi = hw_in + p.T, p.h_out * p.w_out
    X = _operand(p.B * tokens, p.c, lo, hi, seed, sparse).reshape(p.B, tokens, p.c)
    X[:, hw_in:] = TEXT
    X = X.reshape(p.B * tokens, p.c)
    return NS(X=X, G=gather_patch(X, p.B, p.r, p.h_out, p.w_out, tokens).double(), amap=patchmap(p.r, p.r * p.w_out, tokens, rpi, p.w_out, p.c),
              M=p.B * rpi, K=p.r * p.r * p.c, lda=p.c, rpi=rpi, B=p.B, zero=(slice(rpi + p.w_out, rpi + 2 * p.w_out), slice(0, p.r * p.c)))


def gathered(am, perturb=None, **kw):
    """the A operand of an NT case by AMODE: 0 plain rows (257 x 72), 1 PATCH, 2 CONV; .G the matrix the GEMM multiplies"""
    if am == 0:
        X = _operand(257, 72, kw.get("lo", -3), kw.get("hi", 3), kw.get("seed", 0), kw.get("sparse", False))
        g = NS(X=X, G=X.double(), amap=None, M=257, K=72, lda=72, rpi=257, B=1, zero=(slice(128, 136), slice(0, 72)))
    else:
        g = patch_operand(**kw) if am == 1 else conv_operand(CONV.h, CONV.w, CONV.c, CONV.B, CONV.T, **kw)
    if perturb == "halo":
        g.G[g.zero] = 0
    return g


def width(bn):
    """N of the 64- and the 128-wide column tile: both with a ragged last tile (40 of 64; 128 + 72)"""
    return 40 if bn == 64 else 200


def nt_name(bn, am, epi):
    return f"gemm_nt_dma_kernel<{bn}, {am}, {epi}, 64, 128>"


def nt_call(g, W, out, N, **kw):
    if g.amap is not None:
        kw["a_map"] = g.amap
    return dict(op="nt", args=(g.X, W, out, g.M, N, g.K, g.lda, g.K, out.shape[-1]), kw=kw)


# ---------------------------------------------------------------------------------------------------------------- EPI 0: the generic epilogue behind a gather
FACTORS = {1: (2.0, 0.5, 0.0, 1.0, 2.0), 2: (0.5, 0.0, 2.0)}          # one per image (35 / 60 rows: neither divides 128)


def make_epi0(bn, am, perturb=None):
    g, N = gathered(am, seed=600 + bn + am), width(bn)
    W, bias = ints((N, g.K), -3, 3, BF, 601), ints(N, -9, 9, F32, 602)
    scale = torch.tensor(FACTORS[am], dtype=F32, device=dev())
    used = scale.roll(1) if perturb == "factor" else scale                # every sample takes its neighbour's factor
    srow = used.double().repeat_interleave(g.rpi)[:g.M, None]
    ref = integral((g.G @ W.double().t() + bias.double()) * srow, 0.5)
    out = guarded(g.M, N, BF if bn == 64 else F32)
    return NS(**nt_call(g, W, out, N, bias=bias, row_scale=scale, rows_per_scale=g.rpi), outs=[("row_scale alone", lambda: out[:g.M, :N], ref, None, False)],
              guards=std_guards(out, g.M, N), srow=srow, rps=g.rpi)


# ---------------------------------------------------------------------------------------------------------------- EPI 2: a residual behind a patch gather
def make_epi2(bn, alias, perturb=None):
    g, N = gathered(1, seed=610 + bn), width(bn)
    W, bias = ints((N, g.K), -3, 3, BF, 611), ints(N, -9, 9, F32, 612)
    pre = integral(g.G @ W.double().t() + bias.double())
    twice = 2.0 if perturb == "r_twice" else 1.0
    if alias:                                                               # bf16 C holding R, with a factor per image
        scale = torch.tensor(FACTORS[1], dtype=F32, device=dev())
        base = ints((g.M, N), -5, 5, BF, 613)
        out = guarded(g.M, N, BF)
        out[:g.M, :N] = base
        ref = integral(pre * scale.double().repeat_interleave(g.rpi)[:g.M, None] + twice * base.double(), 0.5)
        call = nt_call(g, W, out, N, bias=bias, row_scale=scale, rows_per_scale=g.rpi, R=out)
    else:                                                                   # fp32 R in a buffer of its own (in C's layout), fp32 C
        R = guarded(g.M, N, F32, fill=5.0)
        R[:g.M, :N] = ints((g.M, N), -5, 5, F32, 614)
        out = guarded(g.M, N, F32)
        ref = integral(pre + twice * R[:g.M, :N].double())
        call = nt_call(g, W, out, N, bias=bias, R=R)
    return NS(**call, outs=[("C", lambda: out[:g.M, :N], ref, None, False)], guards=std_guards(out, g.M, N))


# ---------------------------------------------------------------------------------------------------------------- EPI 5: column statistics behind a patch gather
def make_epi5(bn, odt, perturb=None):
    """operands in {-1, 0, 1}: |C| <= K = 64, the squares summed over 175 rows stay below 2^24 (NT_STATS of tests/test_exact_gpu.py)"""
    g, N = gathered(1, perturb, lo=-1, hi=1, seed=620 + bn), width(bn)
    W = ints((N, g.K), -1, 1, BF, 621)
    ref = integral(g.G @ W.double().t())
    assert float(ref.abs().max()) <= 64
    out = guarded(g.M, N, odt)
    st = torch.zeros(2, 5, N, device=dev())                                 # four interleaved accumulators and a guard row behind them
    st[:, 4] = 7.0
    return NS(**nt_call(g, W, out, N, col_sum=st[0], col_sumsq=st[1], col_copies=4),
              outs=[("C", lambda: out[:g.M, :N], ref, None, False), ("col_sum", lambda: st[0, :4].sum(0), integral(ref.sum(0)), None, False),
                    ("col_sumsq", lambda: st[1, :4].sum(0), integral((ref * ref).sum(0)), None, False)],
              guards=std_guards(out, g.M, N) + [("statistics guard row", lambda: st[:, 4] == 7.0)])


# ---------------------------------------------------------------------------------------------------------------- EPI 6 / 7: scatter behind a gather
SCATTER_GRID = {1: (7, 5), 2: (6, 10)}        # h_out x w_out of the r = 2 scatter map: as many rows per image as the gather has (35 / 60), another grid


def make_scatter(bn, am, epi, perturb=None):
    """dX[tokens] = G W^T through a patch map that is not the gather's; EPI 7 adds to what the buffer held (R aliasing C).  The text rows behind every image and the
    guard row keep their fill.  N = r r c_seg: 64, or 192 with c_seg = 48 (the 128-column tile boundary falls inside a segment)"""
    from mvlt_amd._lib import patchmap
    g = gathered(am, seed=630 + bn + am)
    ho, wo = SCATTER_GRID[am]
    cs, r = (16 if bn == 64 else 48), 2
    N, w_in, hw_in = r * r * cs, r * wo, r * ho * r * wo
    tokens = hw_in + 4
    rows = g.B * tokens
    odt = BF if bn == 64 else F32
    W = ints((N, g.K), -3, 3, BF, 631)
    prod = integral(g.G @ W.double().t())                                     # [M, (di, dj, c)]
    dX = guarded(rows, cs, odt)
    if epi == 7:
        dX[:rows, :cs] = ints((rows, cs), -5, 5, odt, 632)
    want = dX[:rows, :cs].double().clone()
    m = torch.arange(g.M, device=dev())
    b, rem = m // g.rpi, m % g.rpi
    wo_used = wo + 1 if perturb == "w_out" else wo
    oi, oj = rem // wo_used, rem % wo_used
    for seg in range(r * r):
        phys = b * tokens + (oi * r + seg // r) * w_in + oj * r + seg % r
        part = prod[:, seg * cs: (seg + 1) * cs]
        want[phys] = part + want[phys] if epi == 7 else part
    integral(want)
    kw = dict(c_map=patchmap(r, w_in, tokens, ho * wo, wo, cs))
    if epi == 7:
        kw["R"] = dX
    if g.amap is not None:
        kw["a_map"] = g.amap
    return NS(op="nt", args=(g.X, W, dX, g.M, N, g.K, g.lda, g.K, cs + 8), kw=kw, outs=[("dX", lambda: dX[:rows, :cs], want, None, False)],
              guards=[("guard row", lambda: dX[rows] == 7.0), ("guard columns", lambda: dX[:, cs:] == 7.0)], text_rows=tokens - hw_in)


# ---------------------------------------------------------------------------------------------------------------- EPI 3 / 4: GELU / GELU' on saturated data
def make_act(bn, am, epi, perturb=None):
    """mlp_cases.gemm_case on the GATHERED operand: A sparse +-1 before the gather, W in [-2, 2], bias = +-(SAT + max |G W^T|).  act 1 stores H = h exactly and
    G within bound_G (0 on the on side); act 2 reads H = h and gives v GELU'(h) = dH within bound_dH"""
    g, N = gathered(am, perturb, seed=640 + bn + am, sparse=True), width(bn)
    Wc = torch.randint(-2, 3, (N, g.K), generator=mc.gen(641 + bn + am)).double()
    c = mc.saturated(g.G.cpu(), Wc)
    to = lambda t: t.to(dev())
    W = to(Wc.to(BF))
    out = guarded(g.M, N, BF)
    view = lambda buf: (lambda: buf[:g.M, :N])
    if epi == 3:
        H = guarded(g.M, N, BF)
        call = nt_call(g, W, out, N, bias=to(c.bias), act=1, H=H)
        outs = [("H", view(H), to(c.h), None, True), ("gelu", view(out), to(c.G), to(c.bound_G), True)]
        guards = std_guards(out, g.M, N) + std_guards(H, g.M, N)
    else:
        H = guarded(g.M, N, BF)
        H[:g.M, :N] = to(c.h.to(BF))
        call = nt_call(g, W, out, N, act=2, H=H)
        outs = [("v * gelu'(H)", view(out), to(c.dH), to(c.bound_dH), True)]
        guards = std_guards(out, g.M, N) + std_guards(H, g.M, N)
    return NS(**call, outs=outs, guards=guards, sat=c)


# ---------------------------------------------------------------------------------------------------------------- the conv3x3 halo kernels
HALO_NT = [(24, 16, 192, 1, BF), (6, 64, 104, 1, F32), (6, 64, 120, 5, F32)]          # h, w, N, EPI, C's type: three 128-pixel tiles per image, three images = 9 row tiles


def make_halo(h, w, N, epi, odt, perturb=None):
    """every image has a top, an interior and a bottom tile; the nine row tiles are launched as 16 workgroups per column tile (whole groups of 8), seven of them idle.
    perturb "halo": the first pixel row of image 1's interior tile reads zeros for the row above it"""
    lim = 1 if epi == 5 else 3
    g = conv_operand(h, w, 64, 3, 5, lo=-lim, hi=lim, seed=650 + w + epi, nz=7 if epi == 5 else None, zero_y=128 // w)
    if perturb == "halo":
        g.G[g.zero] = 0
    W = ints((N, g.K), -lim, lim, BF, 651)
    ref = integral(g.G @ W.double().t())
    out = guarded(g.M, N, odt)
    outs = [("conv3x3", lambda: out[:g.M, :N], ref, None, False)]
    guards, kw = std_guards(out, g.M, N), {}
    if epi == 5:
        assert float(ref.abs().max()) <= 64                                  # 9 taps x 7 channels
        st = torch.zeros(2, 5, N, device=dev())
        st[:, 4] = 7.0
        kw = dict(col_sum=st[0], col_sumsq=st[1], col_copies=4)
        outs += [("col_sum", lambda: st[0, :4].sum(0), integral(ref.sum(0)), None, False), ("col_sumsq", lambda: st[1, :4].sum(0), integral((ref * ref).sum(0)), None, False)]
        guards.append(("statistics guard row", lambda: st[:, 4] == 7.0))
    return NS(**nt_call(g, W, out, N, **kw), outs=outs, guards=guards, tiles_per_img=h * w // 128)


# ---------------------------------------------------------------------------------------------------------------- TN LDS-DMA tiles behind mapped rows
def make_tn(bmt, bn, bmode, perturb=None):
    """C += A^T B into a C that holds 3.0, colsum_a, two m-splits, M no multiple of the 64-row k-tile.  BMODE 0: a token sub-range of both operands (the other rows
    hold 99); BMODE 1: PATCH's gather on B.  N1 > 128 >= 64 >= N2 is the 128 x 64 tile; N1 <= 64 < N2 the 64 x 128 tile, which ops.gemm_tn leaves as it is only
    when a partial-tile scratch is given (two splits are too few for a fold: the atomics stay)"""
    from mvlt_amd._lib import rowmap
    N1 = 200 if bmt == 128 else 40
    kw = dict(splits=2)
    if bmode == 0:
        N2 = 40 if bn == 64 else 200
        Bsz, rows, stride, off = 3, 100, 123, 4
        M = Bsz * rows
        A, Bm = ints((Bsz * stride, N1), -3, 3, BF, 660 + bmt), ints((Bsz * (stride + 5), N2), -3, 3, BF, 661)
        sa, sb = phys_rows(Bsz, rows, stride, off), phys_rows(Bsz, rows, stride + 5, off + 2)
        for buf, sel in ((A, sa), (Bm, sb)):
            keep = torch.ones(buf.shape[0], dtype=torch.bool, device=dev())
            keep[sel] = False
            buf[keep] = TEXT
        Am, G = A[sa].double(), Bm[sb].double()
        zero = (slice(rows, rows + 7), slice(0, N2))
        kw.update(a_map=rowmap(rows, stride, off), b_map=rowmap(rows, stride + 5, off + 2))
        ldb = N2
    else:
        g = patch_operand(seed=662)
        M, N2, Bm, G, ldb, zero = g.M, g.K, g.X, g.G, g.lda, g.zero
        A = ints((M, N1), -3, 3, BF, 663)
        Am = A.double()
        kw.update(b_map=g.amap)
    if perturb == "halo":
        G = G.clone()
        G[zero] = 0
    assert M % 64 != 0
    ref = integral(Am.t() @ G) + 3.0
    Cw = guarded(N1, N2, F32, fill=3.0)
    cs = torch.full((N1 + 1,), 3.0, device=dev())
    kw["colsum"] = cs
    if bmt == 64:
        kw["partials"] = torch.empty(1024, device=dev(), dtype=BF)
    return NS(op="tn", args=(A, Bm, Cw, M, N1, N2, N1, ldb, N2 + 8), kw=kw,
              outs=[("C += A^T B", lambda: Cw[:N1, :N2], ref, None, False), ("colsum_a", lambda: cs[:N1], integral(Am.sum(0)) + 3.0, None, False)],
              guards=std_guards(Cw, N1, N2, 3.0) + [("colsum guard", lambda: cs[N1:] == 3.0)])


BIG_M, BIG_BLOCK = 1 << 24, 4096


def make_big(perturb=None):
    """gemm_tn_kernel<bf16, 128>: bf16 operands leave the LDS-DMA kernel at M = 2^24 rows, and N2 = 72 > 64 takes the 128-wide B tile.  A [2^24, 8] is 268 MB and
    B [2^24, 72] is 2.4 GB: a 4096-row block repeated 4096 times, A nonzero in every 16th row, so |C| <= 2^20 x 9.  (On the CPU the operands are shapes without
    storage: the plan needs no more.)  The scratch only keeps ops.gemm_tn from swapping the narrow N1 away"""
    N1, N2 = 8, 72
    a, b = ints((BIG_BLOCK, N1), -3, 3, BF, 670), ints((BIG_BLOCK, N2), -3, 3, BF, 671)
    a[torch.arange(BIG_BLOCK, device=dev()) % 16 != 0] = 0
    reps = BIG_M // BIG_BLOCK
    if dev().type == "cpu":
        A, Bm = torch.empty(BIG_M, N1, dtype=BF, device="meta"), torch.empty(BIG_M, N2, dtype=BF, device="meta")
    else:
        A, Bm = a.repeat(reps, 1), b.repeat(reps, 1)
    bd = b.double()
    if perturb == "halo":
        bd = bd.clone()
        bd[:16] = 0                                                          # the first sixteen rows of every block dropped
    ref = integral((a.double().t() @ bd) * reps) + 3.0
    Cw = guarded(N1, N2, F32, fill=3.0)
    cs = torch.full((N1 + 1,), 3.0, device=dev())
    return NS(op="tn", args=(A, Bm, Cw, BIG_M, N1, N2, N1, N2, N2 + 8), kw=dict(colsum=cs, partials=torch.empty(1024, device=dev(), dtype=BF)),
              outs=[("C += A^T B", lambda: Cw[:N1, :N2], ref, None, False), ("colsum_a", lambda: cs[:N1], integral(a.double().sum(0) * reps) + 3.0, None, False)],
              guards=std_guards(Cw, N1, N2, 3.0) + [("colsum guard", lambda: cs[N1:] == 3.0)])


BIG_KERNEL = "_ZN12_GLOBAL__N_114gemm_tn_kernelIDF16bLi128EEEv17mvlt_gemm_tn_argsi"
BIG_FAMILY = "gemm_tn_kernel<__hip_bfloat16, 128>"       # what ran() is asked for: the mangled name above is compared as a whole besides


# ---------------------------------------------------------------------------------------------------------------- the table
def _case(group, kernel, fn, *a, perturb):
    ident = "-".join([group] + [str(x).replace("torch.", "") for x in a])
    return NS(id=ident, group=group, kernel=kernel, make=lambda perturb=None: fn(*a, perturb=perturb), perturb=perturb)


CASES = (
    [_case("epi0", nt_name(bn, am, 0), make_epi0, bn, am, perturb="factor") for bn, am in ((64, 2), (128, 1), (128, 2))]
    + [_case("epi2", nt_name(bn, 1, 2), make_epi2, bn, alias, perturb="r_twice") for bn in (64, 128) for alias in (False, True)]
    + [_case("epi5", nt_name(bn, 1, 5), make_epi5, bn, odt, perturb="halo") for bn in (64, 128) for odt in (F32, F16)]
    + [_case("scatter", nt_name(bn, am, epi), make_scatter, bn, am, epi, perturb="w_out") for bn in (64, 128) for am in (1, 2) for epi in (6, 7)]
    + [_case("act", nt_name(bn, am, epi), make_act, bn, am, epi, perturb="halo") for bn in (64, 128) for am in (0, 1, 2) for epi in (3, 4) if (bn, am) != (128, 0)]
    + [_case("halo", f"conv3_nt_kernel<{w}, {192 if N == 192 else 128}, {epi}>", make_halo, h, w, N, epi, odt, perturb="halo") for h, w, N, epi, odt in HALO_NT]
    + [_case("tn", f"gemm_tn_dma_kernel<{bmt}, {bn}, {bmode}, 3, false>", make_tn, bmt, bn, bmode, perturb="halo") for bmt, bn, bmode in ((128, 64, 0), (128, 64, 1), (64, 128, 0))]
    + [_case("big", BIG_KERNEL, make_big, perturb="halo")]
)
GROUPS = ("epi0", "epi2", "epi5", "scatter", "act", "halo", "tn", "big")
CLAIMED = {c.kernel for c in CASES}
UNREACHABLE = "gemm_tn_dma_kernel<128, 64, 2, 3, false>"          # a 3x3 gather has N2 = 9 c_seg >= 72 > 64 columns (tests/test_gemm_plan_cpu.py proves it)
ALREADY_RUN = {nt_name(64, 0, 3), nt_name(64, 0, 4)}              # reached by name in tests/test_mlp_exact_gpu.py and tests/test_gelu_range_gpu.py before this table


def group(name):
    return [c for c in CASES if c.group == name]

"""What the trunk, the heads and the MIM decoder share: parameter access by name over the flat store, and a Linear's forward / backward launches with
every dimension and pitch read off the operands.  The GEMM entries are reached through `ops.` / this module's attributes at call time (the launch-counting
tests replace them there)."""
import torch

from . import ops


def _empty(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)


class StoreAccess:
    """parameter access by name over the flat store `self.S`"""

    def __init__(self, S):
        self.S = S

    def w(self, name):
        return self.S.comp(name)

    def wT(self, name):
        return self.S.extra[name + "::T"]

    def wK(self, name):
        return self.S.extra[name + "::K"]

    def wKT(self, name):
        return self.S.extra[name + "::KT"]

    def f32(self, name):
        return self.S.master(name)

    def g(self, name):
        return self.S.grad(name)

    def gl(self, name):
        """LayerNorm weight / bias gradient: slot of the interleaved accumulators (FlatStore.grad_copies)"""
        return self.S.grad_copies(name)

    def lnk(self):
        return self.S.ln_kwargs()


def saved(v):
    """what a node's forward kept for its backward, or a loud refusal: the node gives it up when its backward has run (ctx.pack / ctx.step = None), so a second
    backward() over a retained graph has nothing to compute from -- and must not leave the partial sums of the nodes that still could"""
    if v is None:
        raise RuntimeError("mvlt_amd: second backward over a retained graph is not supported: this node released what its forward saved when its first "
                           "backward ran (run the forward again; gradients accumulate over separate forward / backward pairs)")
    return v


def _rows(t):
    return t.numel() // t.shape[-1]


def linear(x, W, y, M=None, **epi):
    """y[M, N] = epi(x[M, K] @ W[N, K]^T) (ops.gemm_nt): N and K are the weight's (out, everything else -- nn.Linear's, a conv's (out, taps * cin) copy, a
    zero-padded W^T table), the pitches are the operands' own row strides (a column slice of a wider buffer carries its buffer's), M the rows of x unless
    a row map selects them (then it is given).  Also every Linear's input gradient: dx = dy @ W with W^T as the weight."""
    N = W.shape[0]
    K = W.numel() // N
    return ops.gemm_nt(x, W, y, _rows(x) if M is None else M, N, K, x.stride(-2), K, y.stride(-2), **epi)


def linear_bwd(on, dy, x, gW, gb, wT=None, dx=None, M=None, *, fuse=False, tn=None, dy_map=None, x_map=None, dx_map=None, overwrite=False, **epi):
    """backward of y = x @ W^T + b: if the unit's launch flag `on` says so the weight gradient gW += dy^T x with the bias gradient gb as its column sum
    (ops.gemm_tn; `tn`: the store whose scratch takes the split reduction as bf16 partial tiles, folded in a few batched launches -- FlatStore.fold_copies flushes), then,
    where dx is given, the input gradient dx = epi(dy @ W) through `linear` (wT: the W^T operand copy).  The maps select the rows of dy, x and dx.  fuse: stages 1-2
    (C = 64 / 128, HBM-bound) -- both come out of ONE pass over dy; a frozen weight + bias has no weight gradient, and the fused launch gives way to the plain GEMM."""
    if on:
        rows, N1 = _rows(dy) if M is None else M, gW.shape[0]            # (the weight's own extents: dy may be a zero-padded copy wider than N1)
        N2 = gW.numel() // N1
        if fuse:
            return ops.gemm_tn(dy, x, gW, rows, N1, N2, dy.stride(-2), x.stride(-2), N2, colsum=gb, dgrad=(wT, dx))
        ops.gemm_tn(dy, x, gW, rows, N1, N2, dy.stride(-2), x.stride(-2), N2, a_map=dy_map, b_map=x_map, colsum=gb,
                    partials=None if tn is None else tn.tn_partials(), defer_fold=tn is not None, overwrite=overwrite)
    if dx is not None:
        linear(dy, wT, dx, M, a_map=dy_map, c_map=dx_map, **epi)


def conv_wgrad(S, name, dz, xin, bmap, colsum=None):
    """weight gradient of a gathered-row convolution into the G slice of nn.Conv2d's (out, cin, kh, kw) weight `name`: accumulated in
    the gather's (out, kh, kw, cin) order in the store's tap arena, which S.fold_copies() adds to G at the (out, cin, kh, kw) places (bmap: the r x r gather of cin channels)"""
    cout, taps, cin = dz.shape[-1], bmap.r * bmap.r, bmap.c_seg
    ops.gemm_tn(dz, xin, S.grad_taps(name, cout, taps, cin), _rows(dz), cout, taps * cin, dz.stride(-2), xin.stride(-2), taps * cin, b_map=bmap, colsum=colsum,
                partials=S.tn_partials(), defer_fold=True)

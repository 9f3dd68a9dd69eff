"""Test infrastructure: the DEFINITIONS of every copy the forward reads instead of a Parameter, as plain torch on the fp32 masters and the BatchNorm
buffers, and `audit(model)`, which holds a model's copies against them bit for bit (tests/test_coherence_gpu.py runs every writer of the parameters in
front of it on the GPU; tests/test_coherence_cases_cpu.py plants staleness it must catch, on the CPU).  docs/coherence.md has the writer x copy table.

The library is not imported at module level (and by `audit` not at all): the definitions read `store.P`, `store.master(name)` and the buffers, never the
code that builds the copies.

    C                    bf16(P), element by element, for every parameter (bf16 path; the alignment gaps are nobody's)
    name::T              W^T of a 2-D weight, [cols][ld] with ld = rows padded to a multiple of 8, the padding columns zero
    name::K              conv weight as [out][kh][kw][cin]  (the patch / 3x3 GEMM operand)
    name::KT             its transpose [kh][kw][cin][out]   (kernel == stride convs)
    name::F              flipped dgrad taps [cin][2-dy][2-dx][out]  (3x3 convs)
    score::W / score::T  the 1x1 score conv as [3][K] and as [K][8] (W^T, rows padded to 8 with zeros)
    model._mim_fold      eval-mode BatchNorm folded into its conv: W' = W * gamma * rsqrt(var + eps) in ::K order rounded ONCE to the operand dtype,
                         b' = beta - mean * gamma * rsqrt(var + eps) in fp32
"""
import torch

BN_EPS = 1e-5
SCORE = "t2i_head.score.0.weight"


# ================================================================================================ definitions
def t_copy(w):
    """W^T of a [R][C] weight: [C][ld], ld = R rounded up to 8, columns [R, ld) zero"""
    R, C = w.shape
    out = torch.zeros(C, (R + 7) // 8 * 8, dtype=w.dtype, device=w.device)
    out[:, :R] = w.t()
    return out


def k_copy(w):
    out, cin, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(out, kh * kw * cin)


def kt_copy(w):
    out, cin, kh, kw = w.shape
    return w.permute(2, 3, 1, 0).reshape(kh * kw * cin, out)


def f_copy(w):
    out, cin, kh, kw = w.shape
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(cin, kh * kw * out)


def score_w_copy(w):
    return w.reshape(3, -1)


def score_t_copy(w):
    K = w.numel() // 3
    out = torch.zeros(K, 8, dtype=w.dtype, device=w.device)
    out[:, :3] = w.reshape(3, K).t()
    return out


def fold(w, gamma, beta, mean, var, dt, eps=BN_EPS):
    """(W', b') of mim._folded's docstring from the fp32 conv weight [out][cin][3][3], the BatchNorm affine pair and its running statistics"""
    scale = gamma.float() * torch.rsqrt(var.float() + eps)
    shift = beta.float() - mean.float() * scale
    wk = (k_copy(w.float()) * scale[:, None]).to(dt)
    return wk, shift


def definition(key, w):
    """the copy `key` (a key of FlatStore.extra) of the master `w`, already in the operand dtype; None for a key this file does not know"""
    name, suffix = key.rsplit("::", 1)
    if name == SCORE:
        return {"W": score_w_copy, "T": score_t_copy}.get(suffix, lambda _: None)(w)
    if suffix == "T" and w.dim() == 2:
        return t_copy(w)
    if w.dim() == 4:
        return {"K": k_copy, "KT": kt_copy, "F": f_copy}.get(suffix, lambda _: None)(w)
    return None


# ================================================================================================ the judge
class StaleCopy(AssertionError):
    """raised by audit: `.copy` names the first stale copy, `.index` is the flat index of its first differing element"""

    def __init__(self, copy, index, note=""):
        super().__init__(f"stale copy {copy} at element {index}{note}")
        self.copy, self.index = copy, index


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def first_difference(got, want):
    """flat index of the first element whose BITS differ, None when there is none (shape or dtype apart: index 0)"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return 0
    a, b = _bits(got).reshape(-1), _bits(want).reshape(-1)
    if torch.equal(a, b):
        return None
    return int(torch.nonzero(a != b)[0])


def first_stale(model, fold_too=True):
    """-> None, or (name of the first stale copy, flat index of its first differing element).  Call after a forward (so after refresh()) and a
    device synchronisation.  fold_too: the forward was an eval, no-grad one with the MIM head -- `model._mim_fold` is judged too."""
    S = model.store
    dt = S.compute_dtype
    if S.C is not None:
        want = S.P.to(torch.bfloat16)
        bad = _bits(S.C) != _bits(want)
        if bool(bad.any()):
            for name, (off, n, _) in S.offsets.items():        # the alignment gaps are not judged
                if bool(bad[off:off + n].any()):
                    return f"C[{name}]", int(torch.nonzero(bad[off:off + n])[0])
    for key in S.extra:
        if "::" not in key:
            continue
        want = definition(key, S.master(key.rsplit("::", 1)[0]).to(dt))
        if want is None:
            return key, -1                                     # a copy without a definition here is a gap of this file: loud
        i = first_difference(S.extra[key], want)
        if i is not None:
            return key, i
    if fold_too:
        for name, hit in getattr(model, "_mim_fold", {}).items():
            p = f"t2i_head.{name}"
            bn = getattr(model.t2i_head, name)[1]
            wk, shift = fold(S.master(p + ".0.weight"), S.master(p + ".1.weight"), S.master(p + ".1.bias"), bn.running_mean, bn.running_var, dt)
            for part, got, want in ((".weight", hit[1], wk), (".shift", hit[2], shift)):
                i = first_difference(got, want)
                if i is not None:
                    return f"fold[{name}]{part}", i
    return None


def audit(model, fold_too=True):
    """raises StaleCopy naming the first stale copy and its first differing element; returns the number of copies judged"""
    bad = first_stale(model, fold_too)
    if bad is not None:
        raise StaleCopy(*bad)
    S = model.store
    return (len(S.offsets) if S.C is not None else 0) + sum("::" in k for k in S.extra) + (2 * len(getattr(model, "_mim_fold", {})) if fold_too else 0)


# ================================================================================================ a stand-in store on the CPU
class StandInStore:
    """What audit reads of a FlatStore, made of CPU tensors: P, C, offsets, params, extra, compute_dtype, master().  `fill()` derives every copy from the
    definitions above."""

    def __init__(self, shapes, dt, seed=0, align=8):
        g = torch.Generator().manual_seed(seed)
        self.compute_dtype = dt
        self.offsets, self.params, self.extra = {}, {}, {}
        off = 0
        for name, shape in shapes.items():
            n = 1
            for d in shape:
                n *= d
            self.offsets[name] = (off, n, tuple(shape))
            off += (n + align - 1) // align * align
        self.total = off
        self.P = torch.zeros(off)
        for name, (o, n, shape) in self.offsets.items():
            self.P[o:o + n] = torch.randn(n, generator=g) * 0.5 + (1.0 if name.endswith(".1.weight") else 0.0)
            self.params[name] = self.master(name)
        self.C = torch.full((off,), 7.0, dtype=torch.bfloat16) if dt == torch.bfloat16 else None     # (the gaps keep the sentinel: not judged)

    def master(self, name):
        o, n, shape = self.offsets[name]
        return self.P[o:o + n].view(shape)

    def fill(self, copies):
        """copies: the extra keys to build.  C too."""
        if self.C is not None:
            for o, n, _ in self.offsets.values():
                self.C[o:o + n] = self.P[o:o + n].to(torch.bfloat16)
        for key in copies:
            self.extra[key] = definition(key, self.master(key.rsplit("::", 1)[0]).to(self.compute_dtype)).contiguous().clone()


STAND_IN_SHAPES = {                                   # one parameter of every kind that has a copy, ragged sizes so that the gaps and the ::T padding exist
    "block1.0.attn.q.weight": (13, 16),               # ::T with 3 padding columns
    "block1.0.attn.q.bias": (13,),
    "patch_embed2.proj.weight": (6, 5, 2, 2),         # ::K / ::KT
    "t2i_head.conv4.0.weight": (5, 3, 3, 3),          # ::K / ::F and the fold
    "t2i_head.conv4.1.weight": (5,),
    "t2i_head.conv4.1.bias": (5,),
    SCORE: (3, 7, 1, 1),                              # ::W / ::T
}
STAND_IN_COPIES = ("block1.0.attn.q.weight::T", "patch_embed2.proj.weight::K", "patch_embed2.proj.weight::KT", "t2i_head.conv4.0.weight::K",
                   "t2i_head.conv4.0.weight::F", SCORE + "::W", SCORE + "::T")


def stand_in_model(dt, seed=0):
    """a model-shaped object around a StandInStore with every copy current: .store, .t2i_head.conv4 = (conv, BatchNorm with running statistics), ._mim_fold"""
    import types
    import torch.nn as nn
    S = StandInStore(STAND_IN_SHAPES, dt, seed)
    S.fill(STAND_IN_COPIES)
    g = torch.Generator().manual_seed(seed + 1)
    bn = nn.BatchNorm2d(5)
    bn.running_mean.copy_(torch.randn(5, generator=g))
    bn.running_var.copy_(torch.rand(5, generator=g) + 0.5)
    head = types.SimpleNamespace(conv4=nn.Sequential(nn.Conv2d(3, 5, 3, padding=1, bias=False), bn))
    p = "t2i_head.conv4"
    wk, shift = fold(S.master(p + ".0.weight"), S.master(p + ".1.weight"), S.master(p + ".1.bias"), bn.running_mean, bn.running_var, dt)
    return types.SimpleNamespace(store=S, t2i_head=head, _mim_fold={"conv4": (("key",), wk.clone(), shift.clone())})

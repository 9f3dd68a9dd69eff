"""Test infrastructure: inputs and the float64 reference of the SR-attention kernel tests (tests/test_attention_edges_gpu.py; the premises
of the inputs are pinned on the CPU by tests/test_attention_cases_cpu.py).

`decisive()` builds inputs in which single keys decide single queries, so that one key wrongly admitted, dropped or misaddressed is an
error of order one with a query and a key to print -- N(0,1) data spreads the softmax over all keys and hides such a fault under the
parity bars.  Per head (head_dim 64), with nb = 11 address bits; every value is a small integer or a power of two, exact in bf16:

  keys     dims 0..10 the +-1 binary code of an address (the key's index; key 1 carries key 0's address: a tie), dim 11 = -1,
           dims 12..63 integers in [-3, 3]
  V, dO    integers in [-3, 3]
  queries  by i % 4:
           0  selector: dims 0..10 = amp x code(address of key pi(i)), rest 0; pi from a seeded generator, query 0 -> key M-1 and
              query 4 -> key 0 (the tie).  Score 11 amp scale on the selected key, 2 amp scale less per differing address bit
              (amp 64, scale 0.125: 88 against at most 72)
           1  repelled: dim 11 = 256, rest 0: every valid key scores exactly -32 (scale 0.125), O = mean(V), lse = -32 + log M; a
              padded zero key admitted by mistake scores 0 and takes the row
           2  selector of a key of the last 32-key tile: the ragged tail is always somebody's answer
           3  generic: N(0,1), keeps dS, dQ and dK generic
"""
import functools
import math
import types

import torch

HD = 64
NB = 11                       # address bits: 2048 keys
AMP = 64.0
REPEL = 256.0
SCALE = 0.125
VMAX = 3                      # bound of |V|, |dO| and the free key dims

# both sides of every rung of every dispatch ladder of csrc/attn_plan.h (32-key tiles of the forwards, the <NW,TPW> ladder of the
# backward at 64 / 128 / 192 / 256 / 288 / 320, the resident ranges' ends 288 (fp32) and 320 (bf16), past one streamed key block)
LADDER_M = [1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 288, 289, 320, 321, 385]
# every M at which the GPU tests use decisive inputs: test_attention_cases_cpu.py pins the premises for each
GPU_M = sorted(set(LADDER_M + [29, 150, 272]))


def code(addr):
    """+-1 binary code (float64, [..., NB]) of integer addresses"""
    bits = (addr.unsqueeze(-1) >> torch.arange(NB)) & 1
    return (2 * bits - 1).double()


def key_addresses(M):
    a = torch.arange(M)
    if M >= 2:
        a[1] = 0
    return a


def last_tile(M):
    """first key of the last 32-key tile"""
    return 32 * ((M - 1) // 32)


def decisive(B, H, N, M, dtype, seed, amp=AMP, pi=None):
    """-> namespace(q [B,N,C], kv [B,M,2C] (K | V), do [B,N,C] in `dtype` on the CPU; pi [B,H,N]: the key a selector row asks for, -1 on
    the other rows; kind [N] = i % 4).  `pi` ([N] or [B,H,N]) overrides the drawn selections of the selector rows."""
    assert M <= 2 ** NB
    g = torch.Generator(device="cpu").manual_seed(seed)
    ints = lambda *shape: torch.randint(-VMAX, VMAX + 1, shape, generator=g).double()
    addr = key_addresses(M)
    k = ints(B, M, H, HD)
    k[..., :NB] = code(addr)[None, :, None, :]
    k[..., NB] = -1.0
    v = ints(B, M, H, HD)
    do = ints(B, N, H, HD)
    kind = torch.arange(N) % 4
    drawn = torch.randint(0, M, (B, H, N), generator=g)
    tail = last_tile(M) + torch.randint(0, M - last_tile(M), (B, H, N), generator=g)
    sel = torch.where(kind == 2, tail, drawn)
    sel[:, :, 0] = M - 1
    if N > 4:
        sel[:, :, 4] = 0
    if pi is not None:
        sel = pi.expand(B, H, N).clone()
    is_sel = (kind == 0) | (kind == 2)
    sel = torch.where(is_sel, sel, torch.full_like(sel, -1))
    q = torch.zeros(B, N, H, HD, dtype=torch.float64)
    q[:, kind == 3] = torch.randn(B, int((kind == 3).sum()), H, HD, generator=g).double()
    q[:, kind == 1, :, NB] = REPEL
    qsel = amp * code(addr[sel.clamp_min(0)])                      # [B,H,N,NB]
    q[:, is_sel, :, :NB] = qsel.permute(0, 2, 1, 3)[:, is_sel]
    C = H * HD
    return types.SimpleNamespace(B=B, H=H, N=N, M=M, C=C, dtype=dtype, scale=SCALE, kind=kind, pi=sel,
                                 q=q.reshape(B, N, C).to(dtype), kv=torch.cat((k.reshape(B, M, C), v.reshape(B, M, C)), -1).to(dtype),
                                 do=do.reshape(B, N, C).to(dtype))


def generic(B, H, N, M, dtype, seed, scale):
    """N(0,1) V and dO; Q and K ~ N(0, 1 / (8 scale)) so that the scaled scores stay N(0,1) whatever the scale"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    C = H * HD
    s = (8.0 * scale) ** -0.5
    q = torch.randn(B, N, C, generator=g) * s
    kv = torch.randn(B, M, 2 * C, generator=g)
    kv[..., :C] *= s
    do = torch.randn(B, N, C, generator=g)
    return types.SimpleNamespace(B=B, H=H, N=N, M=M, C=C, dtype=dtype, scale=scale, kind=torch.full((N,), 3), pi=torch.full((B, H, N), -1),
                                 q=q.to(dtype), kv=kv.to(dtype), do=do.to(dtype))


def heads(t, H):
    """[B, R, H*64] -> [B, H, R, 64]"""
    B, R, C = t.shape
    return t.reshape(B, R, H, HD).permute(0, 2, 1, 3)


def reference(q, kv, do, H, scale):
    """float64 softmax(Q K^T scale) V and its autograd from the operands as the kernel reads them (after the cast to their dtype):
    -> o [B,N,C], lse [B,H,N], dq [B,N,C], dkv [B,M,2C] (dq / dkv None without `do`)"""
    B, N, C = q.shape
    q64, kv64 = q.double().requires_grad_(do is not None), kv.double().requires_grad_(do is not None)
    s = heads(q64, H) @ heads(kv64[..., :C], H).transpose(-1, -2) * scale
    o = (s.softmax(-1) @ heads(kv64[..., C:], H)).permute(0, 2, 1, 3).reshape(B, N, C)
    lse = torch.logsumexp(s, -1)
    if do is None:
        return o.detach(), lse.detach(), None, None
    o.backward(do.double())
    return o.detach(), lse.detach(), q64.grad, kv64.grad


def with_reference(case):
    case.ref = reference(case.q, case.kv, case.do, case.H, case.scale)
    return case


@functools.lru_cache(maxsize=None)
def decisive_case(B, H, N, M, dtype, seed=0, amp=AMP):
    """decisive() with its float64 reference, built once per session and shared (treat it as read-only)"""
    return with_reference(decisive(B, H, N, M, dtype, seed, amp))


def selected_mean_v(case):
    """what a selector row must return: the mean of V over the keys that carry the selected address (one key, or the tie of keys 0 and 1);
    [B,H,N,64] float64, rows of the other kinds zero"""
    addr = key_addresses(case.M)
    hit = (addr[None, None, None, :] == addr[case.pi.clamp_min(0)][..., None]) & (case.pi >= 0)[..., None]      # [B,H,N,M]
    w = hit.double() / hit.sum(-1, keepdim=True).clamp_min(1)
    return w @ heads(case.kv[..., case.C:].double(), case.H)


def repelled_lse(M):
    return -REPEL * SCALE + math.log(M)

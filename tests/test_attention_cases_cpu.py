"""CPU: the premises of the decisive-key attention inputs (tests/attn_cases.py), in float64, for every M at which
tests/test_attention_edges_gpu.py uses them -- so that the inputs cannot drift into something a wrong key mask hides under again."""
import math

import pytest
import torch

from tests import attn_cases as ac

BF, F32 = torch.bfloat16, torch.float32
MS = sorted(set(ac.GPU_M + [200, 1152]))
SHAPES = [(1, 3, 77, M) for M in MS] + [(1, 2, 200, 225), (2, 2, 77, 150), (3, 1, 333, 385)]


def scores(case):
    return ac.heads(case.q.double(), case.H) @ ac.heads(case.kv[..., :case.C].double(), case.H).transpose(-1, -2) * case.scale


def attend(s, v):
    return s.softmax(-1) @ v, torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,H,N,M", SHAPES, ids=[f"{B}x{H}x{N}-M{M}" for B, H, N, M in SHAPES])
def test_decisive_inputs_are_decisive(B, H, N, M):
    c = ac.decisive(B, H, N, M, F32, seed=0)
    cb = ac.decisive(B, H, N, M, BF, seed=0)
    kind, pi = c.kind, c.pi
    made = kind != 3
    # every hand-made value is exact in bf16 (the generic rows are N(0,1) and are compared after their cast)
    assert torch.equal(cb.kv.float(), c.kv) and torch.equal(cb.do.float(), c.do) and torch.equal(cb.q.float()[:, made], c.q[:, made])
    assert c.kv.abs().max() <= ac.VMAX and c.do.abs().max() <= ac.VMAX
    assert bool((pi[:, :, 0] == M - 1).all()) and (N <= 4 or bool((pi[:, :, 4] == 0).all()))
    assert bool((pi[:, :, kind == 2] >= ac.last_tile(M)).all()) and bool((pi[:, :, (kind == 1) | (kind == 3)] == -1).all())

    s = scores(c)                                                       # [B,H,N,M]
    v = ac.heads(c.kv[..., c.C:].double(), H)
    o, lse = attend(s, v)
    assert s.abs().max() <= 88.0
    # selector rows: 88 on the keys that carry the selected address, at most 72 anywhere else, > 0.99999 of the weight, O = their V
    sel = (kind == 0) | (kind == 2)
    addr = ac.key_addresses(M)
    hit = addr[None, None, None, :] == addr[pi.clamp_min(0)][..., None]
    ss, hs = s[:, :, sel], hit[:, :, sel]
    assert bool((ss[hs] == 88.0).all())
    if M > 2:
        assert ss.masked_fill(hs, -math.inf).max() <= 72.0
    assert (ss.softmax(-1) * hs).sum(-1).min() > 0.99999
    assert (o - ac.selected_mean_v(c))[:, :, sel].abs().max() < 6e-6
    # repelled rows: every key at exactly -32: the plain mean of V (to a few float64 roundings of values up to 3) and lse = -32 + log M
    rep = kind == 1
    if rep.any():
        assert bool((s[:, :, rep] == -32.0).all())
        assert (o[:, :, rep] - v.mean(2, keepdim=True)).abs().max() < 4 * 3 * 2.3e-16
        assert (lse[:, :, rep] - ac.repelled_lse(M)).abs().max() < 1e-12
        # one padded (zero) key admitted: it scores 0, takes the row (O -> 0: 100 % of the value) and moves lse by ~ 32 - log M
        s1 = torch.cat((s, torch.zeros(B, H, N, 1, dtype=torch.float64)), -1)
        v1 = torch.cat((v, torch.zeros(B, H, 1, ac.HD, dtype=torch.float64)), 2)
        o1, lse1 = attend(s1, v1)
        assert bool(((o1 - o)[:, :, rep].abs() >= 0.999999 * o[:, :, rep].abs()).all()) and o[:, :, rep].abs().max() > 0
        assert (lse1 - lse)[:, :, rep].min() > 20.0
    # the last key dropped: the output row of query 0 (which selects it; all heads) moves by more than 4
    if M > 2:
        o2, _ = attend(s[..., : M - 1], v[:, :, : M - 1])
        assert (o2 - o)[:, :, 0].abs().amax((1, 2)).min() > 4.0


def test_reference_matches_the_closed_forms():
    """the float64 reference on the inputs whose answers are known: selectors, repelled rows, and the zero-query softmax"""
    c = ac.decisive_case(1, 3, 77, 150, F32)
    o, lse, dq, dkv = c.ref
    oh = ac.heads(o, c.H)
    sel = (c.kind == 0) | (c.kind == 2)
    assert (oh - ac.selected_mean_v(c))[:, :, sel].abs().max() < 6e-6
    assert (lse[:, :, c.kind == 1] - ac.repelled_lse(150)).abs().max() < 1e-12
    assert dq.shape == c.q.shape and dkv.shape == c.kv.shape
    o0, lse0, _, _ = ac.reference(torch.zeros_like(c.q), c.kv, None, c.H, c.scale)
    assert (ac.heads(o0, c.H) - ac.heads(c.kv[..., c.C:].double(), c.H).mean(2, keepdim=True)).abs().max() < 1e-14
    assert (lse0 - math.log(150)).abs().max() < 1e-12

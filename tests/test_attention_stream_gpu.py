"""GPU: the key-streamed SR-attention kernels (csrc/attention_stream.hip: attn_fwd_stream_kernel / attn_bwd_stream_kernel; routed by csrc/attn_plan.h) against a plain
PyTorch fp32 reference -- through the public entry points past the LDS-resident range (bf16 M > 320 keys, fp32 M > 288), and through
the streamed exports at small M, next to the resident kernels on the same data.
Tolerances as tests/test_kernels_gpu.py: forward 2e-2 (bf16) / 1e-3 (fp32) max-relative, lse 2e-2 / 1e-3 absolute, dQ / dKV 3e-2 / 2e-3."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
TOL = {F32: 1e-3, BF: 2e-2}
LSE_TOL = {F32: 1e-3, BF: 2e-2}
GRAD_TOL = {F32: 2e-3, BF: 3e-2}
SCALE = 0.125


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def maxrel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rnd(*shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dev()).to(dtype)


def attn_ref(q, kv, H, scale):
    B, N, Cdim = q.shape
    M = kv.shape[1]
    hd = Cdim // H
    qh = q.float().reshape(B, N, H, hd).permute(0, 2, 1, 3)
    k = kv.float()[..., :Cdim].reshape(B, M, H, hd).permute(0, 2, 1, 3)
    v = kv.float()[..., Cdim:].reshape(B, M, H, hd).permute(0, 2, 1, 3)
    s = (qh @ k.transpose(-1, -2)) * scale
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, Cdim)
    return o, torch.logsumexp(s, dim=-1)


def ref_grads(q, kv, do, H):
    qr, kvr = q.float().requires_grad_(True), kv.float().requires_grad_(True)
    o, _ = attn_ref(qr, kvr, H, SCALE)
    o.backward(do.float())
    return qr.grad, kvr.grad


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as _ops
    return _ops


def fwd(ops, q, kv, B, H, N, M, streamed):
    C = 64 * H
    o = torch.empty_like(q)
    lse = torch.empty(B, H, N, device=dev())
    (ops.sr_attention_fwd_streamed if streamed else ops.sr_attention_fwd)(q, kv, o, lse, B, H, N, M, C, 2 * C, C, 0, C, SCALE)
    return o, lse


def bwd(ops, q, kv, o, do, lse, B, H, N, M, streamed, dkv=None):
    C = 64 * H
    dq = torch.empty_like(q)
    if dkv is None:
        dkv = torch.zeros(B, M, 2 * C, device=dev(), dtype=F32)
    (ops.sr_attention_bwd_streamed if streamed else ops.sr_attention_bwd)(q, kv, o, do, lse, dq, dkv, B, H, N, M, C, 2 * C, C, 2 * C, 0, C, SCALE)
    return dq, dkv


def data(B, H, N, M, dtype):
    C = 64 * H
    return rnd(B, N, C, dtype=dtype), rnd(B, M, 2 * C, dtype=dtype, seed=1), rnd(B, N, C, dtype=dtype, seed=2)


def check_fwd(o, lse, ref, ref_lse, dtype, what=""):
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), what
    e = maxrel(o.float(), ref)
    assert e < TOL[dtype], (what, "O", e)
    el = (lse - ref_lse).abs().max().item()
    assert el < LSE_TOL[dtype], (what, "lse", el)


def check_bwd(dq, dkv, gq, gkv, dtype, what=""):
    assert torch.isfinite(dq.float()).all() and torch.isfinite(dkv.float()).all(), what
    e1, e2 = maxrel(dq.float(), gq), maxrel(dkv.float(), gkv)
    assert e1 < GRAD_TOL[dtype], (what, "dQ", e1)
    assert e2 < GRAD_TOL[dtype], (what, "dKV", e2)


# shapes of the model's stages past the resident range: stage-1-like (one head, 16 512 queries), stage-4-like (eight heads, N = M), a
# ragged N; M = 324 (448 px, T = 128), 297 and 1152 are not multiples of either dtype's key blocks (bf16 128, fp32 64)
LARGE_M = {BF: [324, 384, 576, 1152], F32: [297, 320, 324, 384, 576, 1152]}
CASES = [(dt, M, shape) for dt in (BF, F32) for M in LARGE_M[dt] for shape in ("stage1", "stage4", "ragged")]


@pytest.mark.parametrize("dtype,M,shape", CASES, ids=[f"{'bf16' if d == BF else 'fp32'}-M{M}-{s}" for d, M, s in CASES])
def test_public_entry_points_past_the_resident_range(ops, dtype, M, shape):
    B, H, N = {"stage1": (1, 1, 16512), "stage4": (2, 8, M), "ragged": (2, 2, 333)}[shape]
    q, kv, do = data(B, H, N, M, dtype)
    o, lse = fwd(ops, q, kv, B, H, N, M, streamed=False)
    ref, ref_lse = attn_ref(q, kv, H, SCALE)
    check_fwd(o, lse, ref, ref_lse, dtype, (M, shape))
    dq, dkv = bwd(ops, q, kv, o, do, lse, B, H, N, M, streamed=False)
    gq, gkv = ref_grads(q, kv, do, H)
    check_bwd(dq, dkv, gq, gkv, dtype, (M, shape))


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("M", [29, 100, 192, 320])
def test_streamed_exports_match_torch_and_the_resident_kernels(ops, dtype, M):
    B, H, N = 2, 2, 333
    q, kv, do = data(B, H, N, M, dtype)
    o, lse = fwd(ops, q, kv, B, H, N, M, streamed=True)
    ref, ref_lse = attn_ref(q, kv, H, SCALE)
    check_fwd(o, lse, ref, ref_lse, dtype, "streamed")
    dq, dkv = bwd(ops, q, kv, o, do, lse, B, H, N, M, streamed=True)
    gq, gkv = ref_grads(q, kv, do, H)
    check_bwd(dq, dkv, gq, gkv, dtype, "streamed")
    if dtype == F32 and M > 288:
        return                                          # no resident fp32 kernel at 320 keys (LDS): the public entry point streams too
    o_r, lse_r = fwd(ops, q, kv, B, H, N, M, streamed=False)
    assert maxrel(o.float(), o_r.float()) < TOL[dtype]
    assert (lse - lse_r).abs().max().item() < LSE_TOL[dtype]
    dq_r, dkv_r = bwd(ops, q, kv, o_r, do, lse_r, B, H, N, M, streamed=False)
    assert maxrel(dq.float(), dq_r.float()) < GRAD_TOL[dtype]
    assert maxrel(dkv.float(), dkv_r.float()) < GRAD_TOL[dtype]


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("boost", [60.0, 3.0])
def test_late_maximum_in_the_last_key_block(ops, dtype, boost):
    """cdna guide rule 26: the online softmax rescales the running sum and O whenever a block raises a query's maximum, which random
    scores rarely do by much.  Key 350 (in the last key block for both dtypes) is aligned with every other query: its score lies far
    above everything in the earlier blocks (boost 60: ~2^80 in exp space) or a little above (boost 3); the odd queries keep their
    maximum where it was.  Streamed export and public entry point (which streams at 384 keys) alike."""
    B, H, N, M = 2, 1, 320, 384
    q = rnd(B, N, 64, dtype=dtype)
    kv = rnd(B, M, 128, dtype=dtype, seed=1)
    do = rnd(B, N, 64, dtype=dtype, seed=2)
    kv[:, 350, :64] = 0
    kv[:, 350, :8] = boost
    q[:, ::2, :8] = q[:, ::2, :8].abs() + 2.0
    ref, ref_lse = attn_ref(q, kv, H, SCALE)
    gq, gkv = ref_grads(q, kv, do, H)
    for streamed in (False, True):
        o, lse = fwd(ops, q, kv, B, H, N, M, streamed)
        assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
        assert maxrel(o.float(), ref) < TOL[dtype], boost
        assert ((lse - ref_lse).abs() / ref_lse.abs().clamp_min(1.0)).max().item() < LSE_TOL[dtype], boost
        dq, dkv = bwd(ops, q, kv, o, do, lse, B, H, N, M, streamed)
        check_bwd(dq, dkv, gq, gkv, dtype, ("late maximum", boost))


def test_one_chunk_bf16_dkv_writes_every_element(ops):
    """where mvlt_sr_attention_bwd_chunks says 1 the caller may hand a bf16 dKV (mvlt_amd/trunk.py does): every element stored once"""
    B, H, N, M = 4, 8, 128, 384
    assert ops.sr_attention_bwd_chunks(B, H, N, M, BF) == 1
    q, kv, do = data(B, H, N, M, BF)
    o, lse = fwd(ops, q, kv, B, H, N, M, streamed=False)
    dkv = torch.full((B, M, 2 * 64 * H), float("nan"), device=dev(), dtype=BF)
    dq, dkv = bwd(ops, q, kv, o, do, lse, B, H, N, M, streamed=False, dkv=dkv)
    assert not torch.isnan(dkv.float()).any()
    gq, gkv = ref_grads(q, kv, do, H)
    check_bwd(dq, dkv, gq, gkv, BF, "bf16 dKV")


def test_bf16_dkv_with_several_chunks_is_refused(ops):
    """past 128 queries the streamed backward splits the queries of a (batch, head) and meets in fp32 atomics: the chunk count says so,
    and a bf16 dKV is refused instead of being written partially"""
    from mvlt_amd._lib import MVLTError
    B, H, N, M = 1, 2, 384, 384
    assert ops.sr_attention_bwd_chunks(B, H, N, M, BF) == 3
    q, kv, do = data(B, H, N, M, BF)
    o, lse = fwd(ops, q, kv, B, H, N, M, streamed=False)
    with pytest.raises(MVLTError):
        bwd(ops, q, kv, o, do, lse, B, H, N, M, streamed=False, dkv=torch.zeros(B, M, 2 * 64 * H, device=dev(), dtype=BF))


@pytest.mark.parametrize("dtype", [BF, F32])
def test_one_chunk_streamed_backward_is_bit_repeatable(ops, dtype):
    """one query chunk: no atomics, every dQ / dK / dV sum in a fixed order -- 10 launches give identical bits"""
    B, H, N, M = 2, 4, 96, 576
    assert ops.sr_attention_bwd_chunks(B, H, N, M, dtype) == 1
    q, kv, do = data(B, H, N, M, dtype)
    o, lse = fwd(ops, q, kv, B, H, N, M, streamed=False)
    first = None
    for _ in range(10):
        dq, dkv = bwd(ops, q, kv, o, do, lse, B, H, N, M, streamed=False,
                      dkv=torch.full((B, M, 2 * 64 * H), float("nan"), device=dev(), dtype=dtype))
        if first is None:
            assert not torch.isnan(dkv.float()).any()
            first = (dq.clone(), dkv.clone())
            continue
        assert torch.equal(dq, first[0]) and torch.equal(dkv, first[1])

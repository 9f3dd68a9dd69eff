"""GPU: the fused weight EMA (docs/ema.md) -- mvlt_ema_update and mvlt_ema_update_buffers bit for bit against fp32 arithmetic rounded operation by operation
(numpy on the host for the kernels, timm's per-entry loop in torch fp32 ops for the engine runs), and optim.FusedModelEma behind train_one_epoch_vl:
the averaged model computes with its own fresh weights, frozen parameters are left alone, nothing waits on the host, a checkpoint resumes.
Model: pvlt_tiny at 96 px / T = 20 (the geometry of the `*96_T20` fixtures), every head on, so that the MIM decoder's BatchNorm buffers exist."""
import types

import numpy as np
import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LT = dict(mlm=1, itm=1, t2i=1, cls=1)
T, B, IMG = 20, 2, 96
NT = 256                                   # threads per workgroup of ema_update_kernel (csrc/ema.hip)
EMA_MAX_WGS = 8192                         # grid cap of mvlt_ema_update (csrc/ema.hip): one trip of the grid-stride loop covers EMA_MAX_WGS * NT * 4 elements
FROZEN = 2                                 # MVLT_ADAMW_FROZEN
GUARD = 8
DECAYS = (0.0, 1.0, 0.5, 0.9999)
SIZES = (4, 4 * NT + 4, EMA_MAX_WGS * NT * 4 + 12)      # one vector; one workgroup and a vector; a second trip of the loop for the first three lanes


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same_f32(got, want):
    """bit for bit; where the expected value is a NaN, any NaN will do"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


def _ema_ref(e, p, d):
    """numpy float32 on the host: two products and one sum, each rounded on its own; the factors as the C interface takes them"""
    d32, o32 = np.float32(d), np.float32(1.0 - d)
    with np.errstate(all="ignore"):
        a = (e * d32).astype(np.float32)
        b = (p * o32).astype(np.float32)
        return (a + b).astype(np.float32)


_SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.17549435e-38, 3.4e38, -3.4e38, 3.4028235e38, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.1],
                    dtype=np.float32)
_INPUTS = {}


def _inputs(n):
    """(ema, p, mask) on the host, made once per size: random values over many binades, the special values at both ends and strewn in between"""
    if n not in _INPUTS:
        rng = np.random.default_rng(n)
        e = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
        p = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
        if n >= 64:
            k = len(_SPECIAL)
            e[:k], p[:k] = _SPECIAL, _SPECIAL[::-1]                        # every special value against another one ...
            e[-k:], p[-k:] = _SPECIAL[::-1], np.roll(_SPECIAL, 3)
            at = rng.integers(k, n - k, 4 * k)
            e[at] = np.tile(_SPECIAL, 4)                                   # ... and against ordinary values, both ways
            at = rng.integers(k, n - k, 4 * k)
            p[at] = np.tile(_SPECIAL, 4)
        else:
            e[:], p[:] = np.array([-0.0, 1e-40, 3.4e38, np.nan], np.float32)[:n], np.array([0.0, -3e-39, 3.4e38, 1.0], np.float32)[:n]
        # mask: all-frozen, frozen-free and mixed vectors; byte values 0 / 1 (and a stray 3: "other values mean update") / 2
        kind = rng.integers(0, 3, n // 4)
        mask = rng.integers(0, 3, (n // 4, 4)).astype(np.uint8)
        mask[kind == 0] = FROZEN
        mask[kind == 1] = rng.integers(0, 2, (int((kind == 1).sum()), 4)).astype(np.uint8)
        mask[0] = [FROZEN, 0, 1, 3]
        if n > 4:
            mask[-1] = FROZEN
        _INPUTS[n] = (e, p, mask.reshape(-1))
    return _INPUTS[n]


@pytest.mark.parametrize("shift", [0, 4], ids=["base32", "base16"])
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_kernel_bit_for_bit(n, shift):
    """shift 4: the three buffers are views that start 4 elements into their allocations -- 16-byte aligned, not 32"""
    from mvlt_amd import ops
    e_h, p_h, m_h = _inputs(n)
    lo, hi = shift + GUARD, shift + GUARD + n
    total = hi + GUARD
    SENT, SENT16 = 123.456, -1.5
    p_d = torch.zeros(total, device=DEV)
    p_d[lo:hi] = torch.from_numpy(p_h).to(DEV)
    e0 = torch.full((total,), SENT, device=DEV)
    e0[lo:hi] = torch.from_numpy(e_h).to(DEV)
    mask_d = torch.zeros(total, dtype=torch.uint8, device=DEV)
    mask_d[lo:hi] = torch.from_numpy(m_h).to(DEV)
    assert e0[lo:].data_ptr() % 32 == (16 if shift else 0)
    fz = m_h == FROZEN
    for d in DECAYS:
        want = _ema_ref(e_h, p_h, d)
        # (a) no mask, no bf16 copy
        e = e0.clone()
        ops.ema_update(e[lo:hi], p_d[lo:hi], None, n, d, 1.0 - d)
        got = e.cpu().numpy()
        assert _same_f32(got[lo:hi], want), (n, d)
        assert (got[:lo] == np.float32(SENT)).all() and (got[hi:] == np.float32(SENT)).all(), (n, d)
        # (b) with the bf16 copy: the bits of cast_bf16 of the new values
        e = e0.clone()
        e16 = torch.full((total,), SENT16, dtype=torch.bfloat16, device=DEV)
        ops.ema_update(e[lo:hi], p_d[lo:hi], e16[lo:hi], n, d, 1.0 - d)
        assert _same_f32(e.cpu().numpy()[lo:hi], want), (n, d)
        cast = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        ops.cast_bf16(e[lo:hi], cast, n)
        isn = torch.isnan(cast)
        assert torch.equal(torch.isnan(e16[lo:hi]), isn) and torch.equal(_bits(e16[lo:hi])[~isn], _bits(cast)[~isn]), (n, d)
        assert (e16[:lo] == SENT16).all().item() and (e16[hi:] == SENT16).all().item(), (n, d)
        # (c) masked: frozen elements keep a sentinel in both outputs (whatever ema / p hold there), the others are updated
        e = e0.clone()
        e[lo:hi][torch.from_numpy(fz).to(DEV)] = SENT
        e16 = torch.full((total,), SENT16, dtype=torch.bfloat16, device=DEV)
        ops.ema_update(e[lo:hi], p_d[lo:hi], e16[lo:hi], n, d, 1.0 - d, mask_d[lo:hi])
        got = e.cpu().numpy()
        assert (got[lo:hi][fz] == np.float32(SENT)).all(), (n, d)
        assert _same_f32(got[lo:hi][~fz], want[~fz]), (n, d)
        assert (got[:lo] == np.float32(SENT)).all() and (got[hi:] == np.float32(SENT)).all(), (n, d)
        g16 = e16[lo:hi]
        fz_d = torch.from_numpy(fz).to(DEV)
        assert (g16[fz_d] == SENT16).all().item(), (n, d)
        ops.cast_bf16(e[lo:hi], cast, n)
        live = ~fz_d & ~torch.isnan(cast)
        assert torch.equal(_bits(g16)[live], _bits(cast)[live]) and torch.equal(torch.isnan(g16)[~fz_d], torch.isnan(cast)[~fz_d]), (n, d)
        assert (e16[:lo] == SENT16).all().item() and (e16[hi:] == SENT16).all().item(), (n, d)


def test_ema_buffers_kernel():
    """fp32 tensors of 1, 3, 64, 192 and 513 elements at odd 4-byte offsets of ONE allocation and two int64 counters, guards in between"""
    from mvlt_amd import ops
    sizes = (1, 3, 64, 192, 513)
    rng = np.random.default_rng(5)
    SENT = np.float32(-77.25)
    starts = (3, 9, 17, 87, 285)                  # odd: the tensors start at 4-byte addresses that are not 8-byte ones; 5 or 6 guard elements in between
    assert all(b - (a + n) >= 5 for a, b, n in zip(starts, starts[1:], sizes))
    total = starts[-1] + sizes[-1] + 8
    src_h = (rng.standard_normal(total) * np.exp2(rng.integers(-20, 20, total))).astype(np.float32)
    dst_h = (rng.standard_normal(total) * np.exp2(rng.integers(-20, 20, total))).astype(np.float32)
    src_h[starts[2]:starts[2] + 6] = [0.0, -0.0, 1e-40, 3.4e38, np.inf, np.nan]
    inside = np.zeros(total, bool)
    for s, n in zip(starts, sizes):
        inside[s:s + n] = True
    dst_h[~inside] = SENT
    src = torch.from_numpy(src_h).to(DEV)
    cnt_src = torch.tensor([-9, 3, -9, 2 ** 40 + 5, 17, -9], dtype=torch.int64, device=DEV)          # two counters: [1:2] and the pair [3:5]
    for d in (0.5, 0.9999, 0.0, 1.0):
        dst = torch.from_numpy(dst_h).to(DEV)
        cnt_dst = torch.full((6,), -1, dtype=torch.int64, device=DEV)
        rows = [[dst[s:s + n].data_ptr(), src[s:s + n].data_ptr(), n, 0] for s, n in zip(starts, sizes)]
        rows += [[cnt_dst[1:2].data_ptr(), cnt_src[1:2].data_ptr(), 1, 1], [cnt_dst[3:5].data_ptr(), cnt_src[3:5].data_ptr(), 2, 1]]
        assert all(r[0] % 8 == 4 for r in rows[:5])
        table = torch.tensor(rows, dtype=torch.int64).to(DEV)
        ops.ema_update_buffers(table, len(rows), d, 1.0 - d)
        got = dst.cpu().numpy()
        want = _ema_ref(dst_h, src_h, d)
        for s, n in zip(starts, sizes):
            assert _same_f32(got[s:s + n], want[s:s + n]), (d, n)
        assert (got[~inside] == SENT).all(), d                                  # the gaps between the tensors, and both ends
        assert cnt_dst.tolist() == [-1, 3, -1, 2 ** 40 + 5, 17, -1], d          # copied, not averaged; their neighbours untouched
    # a row of an unknown kind and an empty tensor are skipped
    dst = torch.from_numpy(dst_h).to(DEV)
    table = torch.tensor([[dst.data_ptr(), src.data_ptr(), 4, 7], [dst.data_ptr(), src.data_ptr(), 0, 0]], dtype=torch.int64).to(DEV)
    ops.ema_update_buffers(table, 2, 0.5, 0.5)
    assert np.array_equal(dst.cpu().numpy().view(np.int32), dst_h.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ engine level
class _Loader:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


_BATCHES = {}


def _batch(seed):
    if seed not in _BATCHES:
        _BATCHES[seed] = O.to_torch_batch(filler.make_batch(seed, B, IMG, T))          # CPU tensors, like a DataLoader's
    return _BATCHES[seed]


def _model(dtype=torch.bfloat16, seed=3):
    from mvlt_amd import pvlt
    torch.manual_seed(seed)
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, img_size=IMG, compute_dtype=dtype)
    return m.cuda().train()


def _train(m, opt, seeds, model_ema, epoch=0):
    from mvlt_amd.engine import BF16Scaler, train_one_epoch_vl
    res = train_one_epoch_vl(m, None, _Loader([_batch(s) for s in seeds]), opt, torch.device(DEV), epoch, BF16Scaler(), 0, model_ema, None, True, False,
                             types.SimpleNamespace(loss_type=LT))
    torch.cuda.synchronize()
    assert all(v == v and abs(v) != float("inf") for v in res.values()), res


def _timm_update(expected, model, decay):
    """timm.utils.ModelEma.update, entry by entry, in torch fp32 ops on the device (three kernels per tensor: nothing fused); integer entries are copied"""
    with torch.no_grad():
        for k, model_v in model.state_dict().items():
            ema_v = expected[k]
            if ema_v.dtype.is_floating_point:
                ema_v.copy_(ema_v * decay + (1. - decay) * model_v)
            else:
                ema_v.copy_(model_v)


def _forward(m, seed=11):
    b = _batch(seed)
    with torch.no_grad():
        out = m(b["image"].to(DEV), b["input_ids"].to(DEV))
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_engine_steps_equal_timms_loop_bit_for_bit(dtype):
    from mvlt_amd.optim import FusedAdamW, FusedModelEma
    m = _model(dtype)
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    ema = FusedModelEma(m, decay=0.5)
    assert ema.ema.store.P is None and not ema.ema.training
    expected = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in ema.state_dict().items():                                  # bit-equal to the source at the start
        assert k == "_ema_updates" or torch.equal(v, expected[k]), k
    fused_update = ema.update

    def update(model):
        fused_update(model)
        _timm_update(expected, model, ema.decay)
    ema.update = update
    _train(m, opt, (21, 22, 23), ema)
    assert ema.updates == 3
    E, S = ema.ema.store, m.store
    assert E.P is not None and E.P.data_ptr() != S.P.data_ptr() and list(E.offsets.items()) == list(S.offsets.items())
    assert (E.C is not None) == (dtype == torch.bfloat16)
    sd, msd = ema.state_dict(), m.state_dict()
    assert list(sd) == list(msd) + ["_ema_updates"] and sd["_ema_updates"] == 3
    n_float = n_int = moved = 0
    for k, want in expected.items():
        got = sd[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        if want.dtype.is_floating_point:
            assert torch.equal(_bits(got.contiguous()), _bits(want.contiguous())), k
            n_float += 1
            moved += int(not torch.equal(got, msd[k]))
        else:
            assert torch.equal(got, msd[k]) and int(got) == 3, k          # num_batches_tracked: the model's, not one behind
            n_int += 1
    assert n_int == 11 and n_float > 250 and moved > 200                   # the average is not the model


def test_ema_model_computes_with_its_own_fresh_weights():
    """a stale bf16 copy, W^T, permuted conv operand or BatchNorm fold of the averaged model would show here"""
    from mvlt_amd import pvlt
    from mvlt_amd.optim import FusedAdamW, FusedModelEma
    m = _model()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    ema = FusedModelEma(m, decay=0.5)
    _train(m, opt, (21, 22), ema)
    first = _forward(ema.ema)
    refreshes = ema.ema.store.refresh_count
    _train(m, opt, (23,), ema, epoch=1)
    second = _forward(ema.ema)
    assert ema.ema.store.refresh_count == refreshes + 1
    assert set(first) == set(second) and len(first) >= 5
    for k in first:
        assert torch.isfinite(second[k]).all().item() and not torch.equal(first[k], second[k]), k
    torch.manual_seed(99)
    fresh = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, img_size=IMG)
    fresh.load_state_dict(ema.state_dict(), strict=True)
    fresh.cuda().eval()
    want = _forward(fresh)
    for k in second:
        assert torch.equal(_bits(second[k].float().contiguous()), _bits(want[k].float().contiguous())), k
    # set(): the average becomes the model
    ema.set(m)
    for k, v in m.state_dict().items():
        assert torch.equal(ema.state_dict()[k], v), k
    m.eval()
    want = _forward(m)
    got = _forward(ema.ema)
    for k in want:
        assert torch.equal(_bits(got[k].float().contiguous()), _bits(want[k].float().contiguous())), k


def test_frozen_parameters_are_left_alone():
    """decay 0.9999: e * 0.9999 + e * 0.0001 is not e in fp32 for most e, so a frozen entry that is still the model's in every bit was skipped, not averaged.
    The averaged model then has to compute with the RIGHT bf16 copy of what the launch skipped: at its first forward (its store has never cast anything),
    after load_state_dict() and after set() rewrote the parameters under it."""
    from mvlt_amd import pvlt
    from mvlt_amd.optim import FusedAdamW, FusedModelEma
    m = _model()
    frozen = ("block1.", "patch_embed1.", "text_embed1.", "pos_embed1", "text_pos_embed1", "text_embeddings.")
    for n, p in m.named_parameters():
        if n.startswith(frozen):
            p.requires_grad_(False)
    tied = "mlm_head.mlm_decoder.weight"                                    # the word table under its second name: frozen with text_embeddings
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    ema = FusedModelEma(m, decay=0.9999)
    _train(m, opt, (21, 22), ema)
    assert ema.updates == 2 and ema._mask is not None and int((ema._mask == FROZEN).sum()) > 10 ** 6
    sd, msd = ema.state_dict(), m.state_dict()
    n_frozen = n_live = 0
    for n, p in m.named_parameters(remove_duplicate=False):
        if not p.requires_grad:
            assert n.startswith(frozen) or n == tied, n
            assert torch.equal(_bits(sd[n].contiguous()), _bits(msd[n].contiguous())), n
            n_frozen += 1
        else:
            assert not torch.equal(sd[n], msd[n]), n
            n_live += 1
    assert n_frozen > 30 and n_live > 150

    torch.manual_seed(98)
    fresh = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, img_size=IMG).cuda().eval()

    def same_as_a_fresh_model(what):
        fresh.load_state_dict(ema.state_dict(), strict=True)
        want, got = _forward(fresh), _forward(ema.ema)
        assert len(want) >= 5
        for k in want:
            assert torch.isfinite(want[k]).all().item(), (what, k)
            assert torch.equal(_bits(got[k].float().contiguous()), _bits(want[k].float().contiguous())), (what, k)

    assert ema.ema.store.refresh_count == 0
    same_as_a_fresh_model("first forward")                                 # the launches above skipped the frozen elements of a bf16 copy nobody had written
    # a checkpoint with other values everywhere, loaded under the built store; then a masked update
    ema.load_state_dict({k: (v * 1.01 if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in ema.state_dict().items()})
    assert not torch.equal(ema.state_dict()["block1.0.attn.q.weight"], m.state_dict()["block1.0.attn.q.weight"])
    _train(m, opt, (23,), ema, epoch=1)
    assert ema._mask is not None
    same_as_a_fresh_model("load_state_dict + update")
    # set(): the frozen values change back to the model's; then a masked update
    ema.set(m)
    _train(m, opt, (24,), ema, epoch=2)
    assert ema._mask is not None and torch.equal(ema.state_dict()["block1.0.attn.q.weight"], m.state_dict()["block1.0.attn.q.weight"])
    same_as_a_fresh_model("set + update")
    _train(m, opt, (25,), ema, epoch=3)                                    # and in steady state: the copy is current, the masked launch keeps it so
    same_as_a_fresh_model("update on a current copy")
    # un-freezing needs no new average: the mask follows requires_grad
    for p in m.parameters():
        p.requires_grad_(True)
    _train(m, opt, (26,), ema, epoch=4)
    assert ema._mask is None and not torch.equal(ema.state_dict()["block1.0.attn.q.weight"], m.state_dict()["block1.0.attn.q.weight"])
    same_as_a_fresh_model("un-frozen")
    # a buffer re-registered as a new tensor is followed
    bn = m.t2i_head.conv4[1]
    bn.register_buffer("running_mean", bn.running_mean.clone() + 1.0)
    before = ema.ema.t2i_head.conv4[1].running_mean.clone()
    ema.update(m)
    torch.cuda.synchronize()
    moved = ema.ema.t2i_head.conv4[1].running_mean - before
    assert float(moved.min()) > 0.5e-4 and float(moved.max()) < 2e-4        # about (1 - decay) * 1.0


def test_update_has_no_stragglers():
    """steady state: no ATen kernel that waits, no read-back -- the call goes through with synchronizing calls turned into errors"""
    import mvlt_amd._lib as L
    from mvlt_amd.optim import FusedAdamW, FusedModelEma
    m = _model()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    ema = FusedModelEma(m, decay=0.9999, warmup=True)
    _train(m, opt, (21,), ema)                                             # the warm-up call: stores, mask and table exist
    before = ema.ema.store.P.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ema.update(m)
        kernel = L.last_kernel()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert kernel == "ema_buffers_kernel", kernel                          # the model has BatchNorm buffers: their launch is the last one
    assert ema.updates == 2 and not torch.equal(before, ema.ema.store.P)
    for b in list(m.buffers()):
        b.data = b.data.clone()                                            # the buffers move: the table is rebuilt, the launch still finds them
    ema.update(m)
    torch.cuda.synchronize()
    assert torch.equal(ema.ema.t2i_head.conv4[1].num_batches_tracked, m.t2i_head.conv4[1].num_batches_tracked)
    # without buffers the parameter launch is the only one
    from mvlt_amd import ops
    z = torch.zeros(8, device=DEV)
    ops.ema_update(z, z.clone(), None, 8, 0.5, 0.5)
    assert L.last_kernel() == "ema_update_kernel"


def test_checkpoint_resumes_bit_for_bit():
    from mvlt_amd import pvlt
    from mvlt_amd.optim import FusedAdamW, FusedModelEma
    m = _model()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    ema = FusedModelEma(m, decay=0.5)
    _train(m, opt, (21, 22), ema)
    ck = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in ema.state_dict().items()}        # as torch.save / torch.load would hand it over
    torch.manual_seed(7)
    other = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, img_size=IMG)
    ema2 = FusedModelEma(other, decay=0.5)
    ema2.load_state_dict(ck)                                               # before that model's first forward: no store yet
    assert ema2.updates == 2 and ema2.ema.store.P is None and other.store.P is None

    fused_update = ema.update

    def both(model):                                                       # one more step: the same batch, the same source weights for both averages
        fused_update(model)
        ema2.update(model)
    ema.update = both
    _train(m, opt, (23,), ema, epoch=1)
    assert ema.updates == ema2.updates == 3 and ema2.ema.store.P is not None and ema2.ema.store.P.data_ptr() != ema.ema.store.P.data_ptr()
    a, b = ema.state_dict(), ema2.state_dict()
    assert list(a) == list(b)
    for k, v in a.items():
        if not torch.is_tensor(v):
            assert v == b[k], k
        elif v.dtype == torch.float32:
            assert torch.equal(_bits(v.contiguous()), _bits(b[k].contiguous())), k
        else:
            assert torch.equal(v, b[k]), k
    assert torch.equal(ema.ema.store.C, ema2.ema.store.C)                  # and so are the bf16 copies the two would compute with

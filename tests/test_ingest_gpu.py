"""GPU: the device-side image ingest (csrc/ingest.hip through mvlt_amd.ops and mvlt_amd.batchprep, docs/ingest.md) against the exact reference of
tests/ingest_cases.py under each case's own bar; the identities that hold bit for bit; guard words; refusals; and the uint8 path through DeviceBatchPrep,
DevicePrefetcher and the engine loop."""
import types

import numpy as np
import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O
from tests import ingest_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = IC.cases()
GUARD, GUARD_WORDS = -7777.25, 64


def _guarded(shape):
    """an fp32 output of `shape` with GUARD_WORDS guard words behind it (and the guard value all over: an element the kernel skips shows as well)"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD_WORDS,), GUARD, dtype=torch.float32, device=DEV)
    return buf, buf[:n].view(*shape)


def _intact(buf):
    return bool((buf[-GUARD_WORDS:] == GUARD).all())


def _run_resize(case):
    """-> (image, masked or None) as numpy, after checking the guard words"""
    from mvlt_amd import ops
    src = torch.from_numpy(case.src).to(DEV)
    rects_host = torch.from_numpy(case.rects)
    flip = None if case.flip is None else torch.from_numpy(case.flip).to(DEV)
    norm = ops.ingest_norm(IC.MEAN, IC.STD).to(DEV) if case.norm else None
    ibuf, image = _guarded((case.B, 3, case.H, case.W))
    mbuf, masked, flags = None, None, None
    if case.flags is not None:
        mbuf, masked = _guarded((case.B, 3, case.H, case.W))
        flags = torch.from_numpy(case.flags).to(DEV).reshape(case.B, -1).contiguous()
    ops.image_ingest_resize(src, rects_host.to(DEV), rects_host, image, masked, flags, flip, norm, IC.PATCH, IC.FILL)
    torch.cuda.synchronize()
    assert _intact(ibuf) and (mbuf is None or _intact(mbuf)), case
    return image.cpu().numpy(), None if masked is None else masked.cpu().numpy()


@pytest.fixture(scope="module")
def results():
    """every case through the resize kernel, once"""
    return {case.name: _run_resize(case) for case in CASES}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_resize_matches_the_reference_under_its_bar(case, results):
    image, masked = results[case.name]
    want = IC.reference(case)
    err = np.abs(image.astype(np.float64) - want)
    bar = IC.bar(case)
    print(f"{case.name}: largest error {err.max():.3e}, bar {bar.min():.3e} ({IC.taps_v(case)} vertical taps)")
    assert not (image == GUARD).any()                             # every element was written
    assert (err <= bar).all(), (case, err.max(), bar.min())
    # a sentinel pixel (255 around every rectangle) read by any tap would lift an output above the dark inside
    ceiling = np.float32(100 / 255) if not case.norm else ((np.float32(100 / 255) - np.asarray(IC.MEAN, np.float32)) / np.asarray(IC.STD, np.float32)).reshape(3, 1, 1)
    assert (image <= ceiling + 2 * bar).all(), case
    if masked is not None:
        assert np.array_equal(masked.view(np.uint32), IC.masked_of(case, image).view(np.uint32))


@pytest.mark.parametrize("case", [c for c in CASES if c.flags is not None], ids=repr)
def test_masked_equals_grid_mask_apply_on_the_ingests_own_image(case, results):
    from mvlt_amd import ops
    image, masked = results[case.name]
    img = torch.from_numpy(image).to(DEV)
    flags = torch.from_numpy(case.flags).to(DEV).reshape(case.B, -1).contiguous()
    want = ops.grid_mask_apply(img, flags, torch.empty_like(img), IC.PATCH, IC.FILL)
    assert torch.equal(want.cpu(), torch.from_numpy(masked))
    assert (want.cpu() == IC.FILL).any() and not (want.cpu() == IC.FILL).all()


@pytest.mark.parametrize("name", ["identity", "identity_norm_flip"])
@pytest.mark.parametrize("layout", [0, 1])
def test_no_resample_kernel_is_the_table_and_the_resize_identity(name, layout, results):
    """bit for bit: mvlt_image_ingest == table[c][pixel] (ToTensor / Normalize by construction) == mvlt_image_ingest_resize at n == m (up to its flip)"""
    from mvlt_amd import ops
    case = {c.name: c for c in CASES}[name]
    table = ops.ingest_table(*case.mean_std)
    hwc = torch.from_numpy(case.src)
    src = (hwc if layout == 0 else hwc.permute(0, 3, 1, 2).contiguous()).to(DEV)
    ibuf, image = _guarded((case.B, 3, case.H, case.W))
    mbuf, masked = _guarded((case.B, 3, case.H, case.W))
    flags = torch.from_numpy(case.flags).to(DEV).reshape(case.B, -1).contiguous()
    ops.image_ingest(src, table.to(DEV), image, masked, flags, layout, IC.PATCH, IC.FILL)
    torch.cuda.synchronize()
    assert _intact(ibuf) and _intact(mbuf)
    chw = case.src.transpose(0, 3, 1, 2).astype(np.int64)
    want = np.stack([table[c].numpy()[chw[:, c]] for c in range(3)], axis=1)
    got = image.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(masked.cpu().numpy().view(np.uint32), IC.masked_of(case, got).view(np.uint32))
    resized = results[name][0]
    if case.flip is not None:
        resized = np.where(case.flip.astype(bool)[:, None, None, None], resized[..., ::-1], resized)          # undo the flip
    assert np.array_equal(resized.view(np.uint32), got.view(np.uint32))
    # without masked / flags, and from an image whose rows start off a 16-byte boundary: the same values by the element-wise stores
    buf = torch.full((case.B * 3 * case.H * case.W + 8,), GUARD, dtype=torch.float32, device=DEV)
    off = buf[1:1 + case.B * 3 * case.H * case.W].view(case.B, 3, case.H, case.W)
    ops.image_ingest(src, table.to(DEV), off, None, None, layout)
    assert torch.equal(off.cpu(), image.cpu()) and float(buf[0]) == GUARD and bool((buf[-7:] == GUARD).all())


def test_no_resample_kernel_at_a_width_that_is_no_multiple_of_four():
    from mvlt_amd import ops
    rng = np.random.default_rng(5)
    hwc = rng.integers(0, 256, size=(3, 7, 13, 3), dtype=np.uint8)
    table = ops.ingest_table(IC.MEAN, IC.STD)
    for layout in (0, 1):
        src = torch.from_numpy(hwc if layout == 0 else np.ascontiguousarray(hwc.transpose(0, 3, 1, 2))).to(DEV)
        ibuf, image = _guarded((3, 3, 7, 13))
        ops.image_ingest(src, table.to(DEV), image, layout=layout)
        torch.cuda.synchronize()
        want = np.stack([table[c].numpy()[hwc[..., c].astype(np.int64)] for c in range(3)], axis=1)
        assert _intact(ibuf) and np.array_equal(image.cpu().numpy().view(np.uint32), want.view(np.uint32)), layout


@pytest.mark.parametrize("p", [0.0, 0.5, 1.0, 0.3])
def test_flip_flags_are_the_restated_draws(p):
    from mvlt_amd import ops
    for seed, sample0, B in ((77, 0, 300), (3, (1 << 33) + 5, 17)):
        buf = torch.full((B + 16,), 9, dtype=torch.uint8, device=DEV)
        got = ops.flip_flags(buf[:B], p, seed, sample0)
        assert np.array_equal(got.cpu().numpy(), IC.flip_flags(seed, sample0, B, p)) and bool((buf[B:] == 9).all())


def test_refusals_leave_the_outputs_alone():
    """every MVLT_REQUIRE of the resize entry point returns its message and launches nothing"""
    from mvlt_amd import _lib as L
    from mvlt_amd import ops
    from mvlt_amd._lib import MVLTError
    src = torch.zeros(2, 64, 64, 3, dtype=torch.uint8, device=DEV)
    ibuf, image = _guarded((2, 3, 32, 48))
    mbuf, masked = _guarded((2, 3, 32, 48))
    flags = torch.zeros(2, 6, dtype=torch.uint8, device=DEV)
    R = lambda *rows: torch.tensor(rows, dtype=torch.int32)
    for rects, msg in ((R((0, 0, 64, 64), (1, 0, 64, 64)), "leaves the 64 x 64 slab"), (R((0, 0, 64, 64), (0, 60, 4, 5)), "leaves the 64 x 64 slab"),
                       (R((0, 0, 0, 4), (0, 0, 4, 4)), "leaves the 64 x 64 slab")):
        with pytest.raises(MVLTError, match=msg):
            ops.image_ingest_resize(src, rects.to(DEV), rects, image, masked, flags)
    big = torch.zeros(1, 300, 400, 3, dtype=torch.uint8, device=DEV)
    for rect in ((0, 0, 257, 384), (0, 0, 256, 385)):
        with pytest.raises(MVLTError, match="maximum downscale factor 8"):
            ops.image_ingest_resize(big, R(rect).to(DEV), R(rect), image[:1], masked[:1], flags[:1])
    _, odd = _guarded((2, 3, 40, 48))
    host = R((0, 0, 64, 64), (0, 0, 64, 64))
    dev = host.to(DEV)
    with pytest.raises(MVLTError, match="multiples of patch"):                    # (the wrapper's own shape checks would stop this one earlier)
        L.check(L.lib.mvlt_image_ingest_resize(src.data_ptr(), 64, 64, dev.data_ptr(), host.data_ptr(), None, None, odd.data_ptr(), odd.data_ptr(), flags.data_ptr(),
                                               2, 40, 48, 16, 1e-6, None), "mvlt_image_ingest_resize")
    torch.cuda.synchronize()
    assert bool((ibuf == GUARD).all()) and bool((mbuf == GUARD).all()) and bool((odd == GUARD).all())
    # a device copy that disagrees with the checked host copy: the kernel skips that sample instead of reading outside the slab
    dev = R((0, 0, 64, 64), (40, 40, 64, 64)).to(DEV)
    ops.image_ingest_resize(src, dev, host, image, masked, flags)
    torch.cuda.synchronize()
    assert bool((image[0] == 0).all()) and bool((image[1] == GUARD).all()) and _intact(ibuf)


def _u8_batch(seed, B, h, w):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, size=(B, h, w, 3), dtype=np.uint8))


def test_batch_prep_uint8_agrees_with_its_fp32_path():
    from mvlt_amd import ops
    from mvlt_amd.batchprep import DeviceBatchPrep
    B, T, seed, sample0 = 4, 32, 77, 1000
    ori = torch.from_numpy(filler.make_batch(9, B, 64, T)["ori_input_ids"]).to(DEV)
    u8 = _u8_batch(1, B, 32, 48).to(DEV)
    out = DeviceBatchPrep(seed)(u8, ori, sample0=sample0)
    assert out["image"].shape == (B, 3, 32, 48) and out["image"].dtype == torch.float32 and not out["flip"].any()
    assert torch.equal(out["image"].cpu(), u8.cpu().permute(0, 3, 1, 2).float().div(255))                     # ToTensor, bit for bit
    ref = DeviceBatchPrep(seed)(out["image"], ori, sample0=sample0)
    n = int(ref["mlm_count_dev"])
    same_tokens = lambda a: all(torch.equal(a[k], ref[k]) for k in ("input_ids", "mlm_labels", "patch_flags", "mlm_count_dev")) and \
        torch.equal(a["mlm_positions_buf"][:n], ref["mlm_positions_buf"][:n])
    assert n > 0 and same_tokens(out) and torch.equal(out["masked_images"], ref["masked_images"])
    # resized, flipped and normalised: the same token / patch decisions, masked_images consistent with the returned image
    slab = _u8_batch(2, B, 70, 90).to(DEV)
    rects = torch.tensor([[0, 0, 70, 90], [3, 4, 50, 60], [10, 10, 32, 48], [1, 2, 64, 80]], dtype=torch.int32)
    prep = DeviceBatchPrep(seed, hflip=0.5, mean=IC.MEAN, std=IC.STD, size=(32, 48))
    res = prep(slab, ori, sample0=sample0, rects=rects)
    assert np.array_equal(res["flip"].cpu().numpy(), IC.flip_flags(seed, sample0, B, 0.5)) and 0 < int(res["flip"].sum()) < B
    assert same_tokens(res)
    want = ops.grid_mask_apply(res["image"], res["patch_flags"].reshape(B, -1), torch.empty_like(res["image"]))
    assert torch.equal(res["masked_images"], want)
    case = types.SimpleNamespace(src=slab.cpu().numpy(), rects=rects.numpy(), B=B, H=32, W=48, flip=res["flip"].cpu().numpy(), norm=True)
    assert (np.abs(res["image"].cpu().numpy() - IC.reference(case)) <= IC.bar(case)).all()
    # a device tensor of rectangles alone, and the whole slab by default
    again = DeviceBatchPrep(seed, hflip=0.5, mean=IC.MEAN, std=IC.STD, size=(32, 48))(slab, ori, sample0=sample0, rects=rects.to(DEV))
    assert torch.equal(again["image"], res["image"])
    whole = DeviceBatchPrep(seed, size=(32, 48))(slab, ori, sample0=sample0)
    case = types.SimpleNamespace(src=slab.cpu().numpy(), rects=np.array([[0, 0, 70, 90]] * B, np.int32), B=B, H=32, W=48, flip=None, norm=False)
    assert (np.abs(whole["image"].cpu().numpy() - IC.reference(case)) <= IC.bar(case)).all()
    # the running sample id advances by the batch, as on the fp32 path
    p = DeviceBatchPrep(seed)
    p(u8, ori), p(u8, ori)
    assert p.sample == 2 * B


def test_launches_of_both_paths(monkeypatch):
    """the fp32 path makes exactly the launches it made before this feature; the uint8 path never launches grid_mask_apply"""
    from mvlt_amd import batchprep, ops
    calls = []
    for name in ("grid_mask_flags", "grid_mask_apply", "token_mask", "masked_select", "image_ingest", "image_ingest_resize", "flip_flags"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    B, T = 2, 32
    ori = torch.from_numpy(filler.make_batch(9, B, 64, T)["ori_input_ids"]).to(DEV)
    batchprep.DeviceBatchPrep(5)(torch.rand(B, 3, 32, 48, device=DEV), ori)
    assert calls == ["grid_mask_flags", "grid_mask_apply", "token_mask", "masked_select"]
    from mvlt_amd import _lib as L
    del calls[:]
    batchprep.DeviceBatchPrep(5)(torch.rand(B, 3, 32, 48, device=DEV), ori, select=False)
    assert calls == ["grid_mask_flags", "grid_mask_apply", "token_mask"] and L.last_kernel() == "token_mask_kernel"
    del calls[:]
    batchprep.DeviceBatchPrep(5)(_u8_batch(1, B, 32, 48).to(DEV), ori)
    assert calls == ["grid_mask_flags", "flip_flags", "image_ingest", "token_mask", "masked_select"]
    del calls[:]
    batchprep.DeviceBatchPrep(5, size=(32, 48))(_u8_batch(1, B, 40, 50).to(DEV), ori, select=False)
    assert calls == ["grid_mask_flags", "flip_flags", "image_ingest_resize", "token_mask"]
    # the prefetcher over fp32 batches: the same launches per batch as before, nothing of the ingest
    del calls[:]
    batches = [O.to_torch_batch(filler.make_batch(40 + i, B, 64, T)) for i in range(2)]
    slim = [{k: v for k, v in b.items() if k not in ("masked_images", "input_ids", "mlm_labels")} for b in batches]
    got = list(batchprep.DevicePrefetcher(slim, DEV, prep=batchprep.DeviceBatchPrep(21)))
    assert calls == ["grid_mask_flags", "grid_mask_apply", "token_mask", "masked_select"] * 2 and all("flip" not in g for g in got)


def _u8_loader(n, B, S, T):
    out = []
    for i in range(n):
        b = O.to_torch_batch(filler.make_batch(40 + i, B, S, T))
        b = {k: v for k, v in b.items() if k not in ("image", "masked_images", "input_ids", "mlm_labels")}
        b["image"] = _u8_batch(60 + i, B, S + 16, S + 32)
        b["image_rects"] = torch.tensor([[i, 2 * i + b_, S + 8 - b_, S + 20] for b_ in range(B)], dtype=torch.int32)
        out.append(b)
    return out


def test_prefetcher_yields_the_engines_schema_from_uint8_slabs():
    from mvlt_amd.batchprep import DeviceBatchPrep, DevicePrefetcher
    B, S, T = 3, 64, 32
    loader = _u8_loader(2, B, S, T)
    got = list(DevicePrefetcher(loader, DEV, prep=DeviceBatchPrep(21, size=S)))
    assert len(got) == 2
    for i, (b, g) in enumerate(zip(loader, got)):
        for k in ("image", "masked_images"):
            assert g[k].is_cuda and g[k].dtype == torch.float32 and g[k].shape == (B, 3, S, S), k
        assert g["input_ids"].shape == g["mlm_labels"].shape == (B, T) and g["patch_flags"].shape == (B, S // 16, S // 16)
        assert g["mlm_count"] == int((g["mlm_labels"] != -1).sum()) and g["mlm_positions"].numel() == g["mlm_count"]
        assert torch.equal(g["itm_labels"].cpu(), b["itm_labels"]) and torch.equal(g["image_rects"].cpu(), b["image_rects"])
        case = types.SimpleNamespace(src=b["image"].numpy(), rects=b["image_rects"].numpy(), B=B, H=S, W=S, flip=None, norm=False)
        assert (np.abs(g["image"].cpu().numpy() - IC.reference(case)) <= IC.bar(case)).all()
        m = g["patch_flags"].bool().repeat_interleave(16, 1).repeat_interleave(16, 2)[:, None].expand(-1, 3, -1, -1)
        assert torch.equal(g["masked_images"], torch.where(m, torch.tensor(IC.FILL, device=DEV), g["image"]))
        want = DeviceBatchPrep(21, size=S)(b["image"].to(DEV), b["ori_input_ids"].to(DEV), sample0=i * B, rects=b["image_rects"])
        assert torch.equal(want["image"], g["image"]) and torch.equal(want["input_ids"], g["input_ids"])


def test_engine_loop_runs_two_steps_on_uint8_slabs():
    """an unmodified train_one_epoch_vl over DevicePrefetcher(uint8 loader): two steps, finite losses"""
    from mvlt_amd import pvlt
    from mvlt_amd.batchprep import DeviceBatchPrep, DevicePrefetcher
    from mvlt_amd.engine import BF16Scaler, train_one_epoch_vl
    from mvlt_amd.optim import FusedAdamW
    lt = dict(mlm=1, itm=1, t2i=1, cls=0)
    B, S, T = 2, 64, 32
    cfg = O.Cfg("pvlt_tiny", lt, 224, 768, T, 0.0)
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=lt, pretrained_pth=None, drop_path_rate=0.0, compute_dtype=torch.float32)
    m.load_state_dict(O.filled_state_dict(cfg, 6), strict=True)
    m.cuda()
    m.injected_masks = dict(bert=torch.ones(B, T, 768), droppath=[torch.ones(B)] * 8, droppath2=[torch.ones(B)] * 8)
    opt = FusedAdamW(m, lr=1e-4, weight_decay=0.01)
    loader = DevicePrefetcher(_u8_loader(2, B, S, T), DEV, prep=DeviceBatchPrep(21, size=S, hflip=0.5))
    stats = train_one_epoch_vl(m, None, loader, opt, torch.device(DEV), 0, BF16Scaler(), None, None, None, True, False, types.SimpleNamespace(loss_type=lt))
    assert stats and all(np.isfinite(v) for v in stats.values()), stats
    assert stats["loss_mlm"] > 0 and stats["loss_itm"] > 0

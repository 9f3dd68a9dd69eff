"""CPU: rectangular (H x W) inputs.  The oracle is pinned to numbers the REAL reference produced at 256 x 192
(tests/golden/rect_tiny256x192.npz, written by tests/golden/make_golden_rect.py after it asserted oracle == reference there); the
oracle refuses 896 x 224 as the reference does; the schedule's input rule (each side a multiple of 32, rectangles allowed) and its
per-stage (h, w) grids; the grid-mask oracle on non-square patch grids."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import batchprep_oracle as BP
from oracle import pvlt_oracle as O
from tests.golden.make_golden_rect import CASE, NAME, rect_batch

LT = dict(mlm=1, itm=1, t2i=1, cls=1)
DIMS = (64, 128, 320, 512)


def _sample(t, n):
    f = t.detach().reshape(-1).to(torch.float32)
    stride = max(1, f.numel() // n) | 1
    return f[::stride][:n].numpy()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return np.linalg.norm(a - b) / max(1e-30, np.linalg.norm(b))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, NAME + ".npz"))
    seed, B, H, W, T = (int(v) for v in g["meta"][:5])
    assert (H, W, T, B) == (CASE["H"], CASE["W"], CASE["T"], CASE["B"]) and H != W
    cfg = O.Cfg("pvlt_tiny", LT, 224, 768, T, float(g["meta"][5]))
    return g, cfg, O.filled_state_dict(cfg, seed), rect_batch(seed, B, H, W, T), seed


def test_rect_batch_is_a_consistent_crop():
    """the masked image differs from the clean one on whole 16-pixel patches only, after the crop too"""
    b = rect_batch(5, 2, 96, 64, 8)
    assert tuple(b["image"].shape) == tuple(b["masked_images"].shape) == (2, 3, 96, 64)
    diff = (b["image"] != b["masked_images"]).any(1).numpy()                       # (B, H, W)
    flags = diff[:, ::16, ::16]
    assert np.array_equal(np.repeat(np.repeat(flags, 16, 1), 16, 2), diff)
    assert flags.any() and not flags.all()


def test_oracle_eval_matches_the_reference_at_256x192(fixture, parity):
    g, cfg, sd, batch, seed = fixture
    B, H, W = batch["image"].shape[0], batch["image"].shape[2], batch["image"].shape[3]
    taps = {}
    with torch.no_grad():
        out = O.forward(sd, cfg, batch["image"], batch["input_ids"], taps=taps)
    for i in range(4):
        assert tuple(taps[f"img_feat{i+1}"].shape) == (B, DIMS[i], H // (4 * 2 ** i), W // (4 * 2 ** i))
        for k in (f"img_feat{i+1}", f"text_feat{i+1}"):
            assert parity("tap/" + k, _rel(_sample(taps[k], 1024), g[f"eval/tap/{k}/sample"]), 5e-5), k
    assert tuple(out["t2i_logits"].shape) == (B, 3, H, W)
    for k, v in out.items():
        assert tuple(v.shape) == tuple(g[f"eval/out/{k}/shape"]), k
        assert parity("out/" + k, _rel(_sample(v, 4096), g[f"eval/out/{k}/sample"]), 5e-5), k
    for k in ("itm_logits", "sup_cls_logits", "sub_cls_logits"):
        assert parity("full/" + k, _rel(out[k].numpy(), g[f"eval/full/{k}"]), 5e-5), k
    assert np.array_equal(O.masked_positions(batch["mlm_labels"]).numpy(), g["masked_positions"])
    assert parity("t2i_grid", _rel(out["t2i_logits"][:, :, ::16, ::16].numpy(), g["eval/t2i/grid"]), 5e-5)


def test_oracle_train_step_matches_the_reference_at_256x192(fixture, parity):
    from tests.golden.make_golden import make_masks
    g, cfg, sd, batch, seed = fixture
    step_idx = int(g["meta"][6])
    masks = make_masks(cfg, batch["image"].shape[0], batch["input_ids"].shape[1], seed + step_idx)
    sdg = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running_" not in k) else v) for k, v in sd.items() if k != O.TIED[0]}
    sdg[O.TIED[0]] = sdg[O.TIED[1]]
    lo, _ = O.step_loss(sdg, cfg, batch, step_idx, train=True, masks=masks, bn_out={})
    lo["total_loss"].backward()
    for k, v in lo.items():
        ref = float(g[f"train{step_idx}/loss/{k}"])
        assert parity("loss/" + k, abs(float(v) - ref) / max(1e-12, abs(ref)), 2e-4), (k, float(v), ref)
    n = 0
    for k, v in sdg.items():
        gk = f"train{step_idx}/grad/{k}/norm"
        if gk not in g.files or float(g[gk]) < 1e-7:
            continue
        n += 1
        refn = float(g[gk])
        assert parity("grad-norm/" + k, abs(v.grad.double().norm().item() - refn) / refn, 2e-4), k
        ref_s = g[f"train{step_idx}/grad/{k}/sample"]
        es = float(np.abs(_sample(v.grad, 32) - ref_s).max() / max(np.abs(ref_s).max(), 1e-3 * refn / max(1.0, v.numel() ** 0.5)))
        assert parity("grad-sample/" + k, es, 8e-4), k
    assert n > 50


def test_oracle_refuses_896x224_like_the_reference():
    """stage 2 has 112 x 28 = 3136 patches = stage 1's constructor count, so reference libs/pvlt.py:292 hands it the 784-row embedding unresized"""
    T = 8
    cfg = O.Cfg("pvlt_tiny", LT, 224, 768, T, 0.0)
    sd = O.filled_state_dict(cfg, 3)
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            O.forward(sd, cfg, torch.zeros(1, 3, 896, 224), torch.zeros(1, T, dtype=torch.long))


def test_input_rule_names_both_sides():
    from mvlt_amd.plan import check_input_size, stage_grids
    m = types.SimpleNamespace(patch_size=4)
    for H, W in ((256, 192), (192, 320), (1568, 32), (224, 224)):
        check_input_size(m, H, W)
    for H, W in ((448, 112), (112, 448), (250, 256)):
        with pytest.raises(AssertionError) as e:
            check_input_size(m, H, W)
        assert str(H) in str(e.value) and str(W) in str(e.value)
    assert stage_grids(m, 256, 192) == [(64, 48), (32, 24), (16, 12), (8, 6)]
    assert stage_grids(m, 224, 224) == [(56, 56), (28, 28), (14, 14), (7, 7)]


@pytest.mark.parametrize("gh,gw", [(16, 12), (12, 20), (98, 2), (2, 98)])
@pytest.mark.parametrize("mode", [0, 1])
def test_grid_mask_oracle_on_non_square_grids(gh, gw, mode):
    """exact mode masks exactly num_mask patches on any grid; the reference generator's window quirk stays inside the shuffled list"""
    n = int(0.5 * gh * gw)
    f = BP.grid_flags(11, 4, gh, gw, n, mode)
    assert f.shape == (gh, gw) and f.dtype == np.uint8
    if mode == 0:
        assert int(f.sum()) == n
    img = np.random.RandomState(0).rand(3, gh * 16, gw * 16).astype(np.float32)
    masked = BP.apply_grid_mask(img, f)
    m = np.repeat(np.repeat(f.astype(bool), 16, 0), 16, 1)
    assert (masked[:, m] == np.float32(1e-6)).all() and np.array_equal(masked[:, ~m], img[:, ~m])

"""CPU: the host side of fused gradient clipping -- the four entry points are declared, exported and bound; BF16Scaler keeps torch's clip_grad_norm_ for
optimizers that are not FusedAdamW; a clip nobody stepped does not outlive the next backward pass."""
import os
import re

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mvlt_grad_sumsq", "mvlt_clip_coef", "mvlt_scale_by_dev", "mvlt_adamw_step")


def test_entry_points_are_declared_exported_and_bound():
    import inspect
    import mvlt_amd._lib as L
    from mvlt_amd import ops
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    declared = set(re.findall(r"\b(mvlt_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in L.EXPORTS, name
        assert hasattr(L.lib, name), name
        assert callable(getattr(ops, name[len("mvlt_"):])), name
    assert re.search(r"mvlt_adamw_step\([^;]*const float\* gscale_dev[^;]*void\* stream\);", hdr, re.S)
    assert "engine_grid_masking.py:126" in hdr[hdr.index("Gradient clipping"):hdr.index("int mvlt_grad_sumsq")]
    sig = inspect.signature(ops.adamw_step)
    assert sig.parameters["gscale_dev"].default is None and sig.parameters["gscale_dev"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig.parameters)[:8] == ["p", "g", "m", "v", "p16", "n", "hp", "decay_mask"]          # every existing positional call keeps working
    assert L.ABI_VERSION == 8
    # bad arguments come back as error codes (no launch without a GPU)
    assert L.lib.mvlt_grad_sumsq(None, 4, None, None, 1, None) < 0
    assert L.lib.mvlt_grad_sumsq(16, 4, None, 16, 1025, None) < 0 and b"n_partials" in L.lib.mvlt_last_error()
    assert L.lib.mvlt_grad_sumsq(16, 6, None, 16, 4, None) < 0
    assert L.lib.mvlt_clip_coef(None, 1, 1.0, 1.0, None, None) < 0
    assert L.lib.mvlt_scale_by_dev(None, 4, None, None) < 0


class _StubOptimizer:
    def __init__(self):
        self.steps = 0

    def step(self):
        self.steps += 1


def test_scaler_keeps_torchs_clipping_for_other_optimizers(monkeypatch):
    from mvlt_amd.engine import BF16Scaler
    w = nn.Parameter(torch.tensor([3.0, 4.0]))
    calls = []
    real = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda params, max_norm, *a, **k: (calls.append(max_norm), real(params, max_norm, *a, **k))[1])
    opt, scaler = _StubOptimizer(), BF16Scaler()
    assert scaler.last_grad_norm is None
    scaler((w * w).sum() / 2, opt, clip_grad=1.0, parameters=[w])             # gradient = w, norm 5
    assert calls == [1.0] and opt.steps == 1
    assert scaler.last_grad_norm is None                                      # the fused path's device scalar only
    assert abs(float(w.grad.norm()) - 1.0) < 1e-5
    w.grad = None
    for off in (None, 0):
        scaler((w * w).sum() / 2, opt, clip_grad=off, parameters=[w])
        w.grad = None
    assert calls == [1.0] and opt.steps == 3


def test_begin_backward_drops_a_stale_clip():
    from tests.test_host_cpu import _toy_store
    S = _toy_store().store
    assert S.pending_clip is None
    S.pending_clip = torch.tensor([0.25])                 # a clip whose step never ran
    S.pending_grad_scale = 0.5
    S.begin_backward()                                    # every .grad is None: G starts from zero, nothing is owed to it
    assert S.pending_clip is None and S.pending_grad_scale == 1.0
    assert float(S.G.abs().sum()) == 0.0

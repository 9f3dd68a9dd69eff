"""CPU: the host side of the non-finite-gradient guard (docs/nonfinite_guard.md) -- include/mvlt_hip_ext.h and mvlt_amd/_lib.py EXT_PROTOTYPES agree, the
library exports the entry points and refuses bad arguments without a launch, BF16Scaler(skip_nonfinite=True) skips a stock optimizer's step on Inf / NaN
gradients, a gate nobody stepped does not outlive the next backward pass, and FusedAdamW's checkpoint grows only when the guard is on."""
import ctypes as C
import os
import re

import torch
import torch.nn as nn

from tests.test_host_cpu import _header_abi, _toy_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = ("mvlt_ext_version", "mvlt_step_gate", "mvlt_adamw_step_gated")


def _ext_header():
    return open(os.path.join(ROOT, "include", "mvlt_hip_ext.h")).read()


def test_ext_header_and_binding_agree():
    """name by name, parameter by parameter (the rule tests/test_host_cpu.py applies to mvlt_hip.h and PROTOTYPES)"""
    import mvlt_amd._lib as L
    hdr = _ext_header()
    protos, structs = _header_abi(hdr)
    assert set(protos) == set(L.EXT_PROTOTYPES) == set(EXT) and not structs
    assert not set(L.EXT_PROTOTYPES) & set(L.PROTOTYPES)                        # additions, not overrides: the ABI table is what it was
    scalars = {"int": C.c_int, "long": C.c_long, "float": C.c_float}
    for name, (ret, params) in protos.items():
        restype, argtypes = L.EXT_PROTOTYPES[name]
        fn = getattr(L.lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (ctype, written) in enumerate(zip(argtypes, params)):
            want = scalars[written] if written in scalars else C.c_void_p
            assert written in scalars or written.endswith("*"), (name, i, written)
            assert ctype is want, (name, i, written, ctype)
    # the gated step has mvlt_adamw_step's parameters with the gate in front of the stream
    main, _ = _header_abi(open(os.path.join(ROOT, "include", "mvlt_hip.h")).read())
    assert protos["mvlt_adamw_step_gated"][1] == main["mvlt_adamw_step"][1]
    assert re.search(r"mvlt_adamw_step_gated\([^;]*const float\* gate[^;]*void\* stream\);", hdr, re.S)
    assert "engine_grid_masking.py:116-120" in hdr and "engine_grid_masking.py:126-127" in hdr


def test_ext_version_and_exports():
    import mvlt_amd._lib as L
    from mvlt_amd import ops
    assert L.lib.mvlt_ext_version() == L.EXT_VERSION == int(re.search(r"#define MVLT_EXT_VERSION (\d+)", _ext_header()).group(1)) == 1
    for name in EXT:
        assert hasattr(L.lib, name), name
    assert callable(ops.step_gate) and callable(ops.adamw_step_gated)
    assert L.ABI_VERSION == 8 and not set(EXT) & set(L.EXPORTS)


def test_bad_arguments_are_error_codes():
    """no launch without a GPU: every call below must come back from the argument checks"""
    import mvlt_amd._lib as L
    lib, err = L.lib, lambda: L.lib.mvlt_last_error()
    p = 4096                                                   # any non-null address: the checks never dereference
    assert lib.mvlt_step_gate(None, 4, 1.0, 1.0, p, p, None) < 0 and b"mvlt_step_gate" in err()
    assert lib.mvlt_step_gate(p, 4, 1.0, 1.0, None, p, None) < 0 and b"mvlt_step_gate" in err()
    assert lib.mvlt_step_gate(p, 4, 1.0, 1.0, p, None, None) < 0 and b"mvlt_step_gate" in err()
    for bad in (0, 1025, -1):
        assert lib.mvlt_step_gate(p, bad, 1.0, 1.0, p, p, None) < 0 and b"n_partials" in err() and str(bad).encode() in err()
    args = [p, p, p, p, None, 8, p, None, p, None]                # p, g, m, v, p_bf16, n, hp, decay_mask, gate, stream
    for i in (0, 1, 2, 3, 6, 8):                                  # each required pointer missing in turn
        a = list(args)
        a[i] = None
        assert lib.mvlt_adamw_step_gated(*a) < 0 and b"mvlt_adamw_step_gated" in err(), i
    a = list(args)
    a[5] = 6
    assert lib.mvlt_adamw_step_gated(*a) < 0 and b"multiple of 4" in err()
    a[5] = 0
    assert lib.mvlt_adamw_step_gated(*a) == 0                     # nothing to do: no launch


class _StubSGD:
    """the smallest optimizer: p -= lr * grad, and a count of the calls"""

    def __init__(self, params, lr=0.5):
        self.params, self.lr, self.steps = list(params), lr, 0

    def step(self):
        self.steps += 1
        with torch.no_grad():
            for p in self.params:
                p -= self.lr * p.grad


def _loss(w, factor=1.0):
    return (w * w).sum() / 2 * factor            # gradient = w * factor


def test_scaler_skips_a_stock_optimizers_step_on_nonfinite_gradients():
    from mvlt_amd.engine import BF16Scaler
    for clip in (None, 0, 10.0):
        w = nn.Parameter(torch.tensor([3.0, 4.0]))
        opt, scaler = _StubSGD([w]), BF16Scaler(skip_nonfinite=True)
        assert scaler.skipped_steps == 0 and scaler.state_dict() == {}
        scaler(_loss(w), opt, clip_grad=clip, parameters=[w])
        assert opt.steps == 1 and scaler.skipped_steps == 0
        assert torch.equal(w.detach(), torch.tensor([1.5, 2.0]))              # norm 5 < 10: the clip does not bite, max_norm=inf does not either
        w.grad = None
        before = w.detach().clone()
        scaler(_loss(w, float("inf")), opt, clip_grad=clip, parameters=[w])
        assert opt.steps == 1 and scaler.skipped_steps == 1
        assert torch.equal(w.detach().view(torch.int32), before.view(torch.int32))
        w.grad = None
        scaler(_loss(w, float("nan")), opt, clip_grad=clip, parameters=[w])
        assert opt.steps == 1 and scaler.skipped_steps == 2
        assert torch.equal(w.detach().view(torch.int32), before.view(torch.int32))
        w.grad = None
        scaler(_loss(w), opt, clip_grad=clip, parameters=[w])                  # and the next clean step steps
        assert opt.steps == 2 and scaler.skipped_steps == 2
        assert torch.equal(w.detach(), torch.tensor([0.75, 1.0]))
    # with a clip that bites, the guarded step is the clipped step
    w = nn.Parameter(torch.tensor([3.0, 4.0]))
    opt, scaler = _StubSGD([w]), BF16Scaler(skip_nonfinite=True)
    scaler(_loss(w), opt, clip_grad=1.0, parameters=[w])
    assert abs(float(w.grad.norm()) - 1.0) < 1e-5 and opt.steps == 1


def test_without_the_guard_both_steps_run():
    """today's behaviour, and the proof that the test above bites: the poisoned step reaches the parameter"""
    from mvlt_amd.engine import BF16Scaler
    w = nn.Parameter(torch.tensor([3.0, 4.0]))
    opt, scaler = _StubSGD([w]), BF16Scaler()
    assert scaler.skip_nonfinite is False
    scaler(_loss(w), opt, clip_grad=None, parameters=[w])
    w.grad = None
    scaler(_loss(w, float("inf")), opt, clip_grad=None, parameters=[w])
    assert opt.steps == 2 and scaler.skipped_steps == 0
    assert not torch.isfinite(w).any()


def test_begin_backward_drops_a_stale_gate():
    S = _toy_store().store
    assert S.pending_gate is None
    S.pending_gate = torch.tensor([float("inf"), 0.0, 0.0, 0.0])       # a gate whose step never ran
    S.pending_grad_scale = 0.5
    S.begin_backward()                                                 # every .grad is None: G starts from zero, nothing is owed to it
    assert S.pending_gate is None and S.pending_clip is None and S.pending_grad_scale == 1.0
    assert float(S.G.abs().sum()) == 0.0


def test_fused_adamw_checkpoint_grows_only_with_the_guard():
    from mvlt_amd.optim import FusedAdamW
    off = FusedAdamW(_toy_store())
    assert off.skip_nonfinite is False
    assert set(off.state_dict()["fused"]) == {"step", "m", "v"}
    on = FusedAdamW(_toy_store(), skip_nonfinite=True)
    sd = on.state_dict()
    assert set(sd["fused"]) == {"step", "m", "v", "applied", "skipped"}
    assert sd["fused"]["applied"] == 0 and sd["fused"]["skipped"] == 0 and on.skipped_steps == 0 and on.applied_steps == 0
    # both kinds of checkpoint load into both kinds of optimizer
    on.load_state_dict(off.state_dict())
    off.load_state_dict(sd)
    assert set(off.state_dict()["fused"]) == {"step", "m", "v"}

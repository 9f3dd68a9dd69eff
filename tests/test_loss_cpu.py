"""CPU: the host side of the loss options (docs/loss_options.md) -- include/mvlt_hip_loss.h and mvlt_amd/_lib.py LOSS_PROTOTYPES agree and the older tables are
as they were; loss.hip is built and hashed; the entry points refuse bad arguments without a launch; the CPU path of engine.cross_entropy hands both options to
F.cross_entropy; and `set_loss_options` / `compute_losses(options=)` on a CPU model."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests.test_host_cpu import _header_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS = ("mvlt_loss_version", "mvlt_ce_smooth_fwd", "mvlt_ce_smooth_bwd")


def _loss_header():
    return open(os.path.join(ROOT, "include", "mvlt_hip_loss.h")).read()


def test_loss_header_and_binding_agree():
    """name by name, parameter by parameter (the rule tests/test_lamb_cpu.py applies to mvlt_hip_lamb.h and LAMB_PROTOTYPES)"""
    import mvlt_amd._lib as L
    protos, structs = _header_abi(_loss_header())
    assert set(protos) == set(L.LOSS_PROTOTYPES) == set(LOSS) and not structs
    older = set(L.PROTOTYPES) | set(L.EXT_PROTOTYPES) | set(L.EMA_PROTOTYPES) | set(L.PLAN_PROTOTYPES) | set(L.OPT_PROTOTYPES) | set(L.LAMB_PROTOTYPES)
    assert not set(LOSS) & older                                 # an addition, not an override
    scalars = {"int": C.c_int, "long": C.c_long, "float": C.c_float}
    for name, (ret, params) in protos.items():
        restype, argtypes = L.LOSS_PROTOTYPES[name]
        fn = getattr(L.lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (ctype, written) in enumerate(zip(argtypes, params)):
            want = scalars[written] if written in scalars else C.c_void_p
            assert written in scalars or written.endswith("*"), (name, i, written)
            assert ctype is want, (name, i, written, ctype)
    assert protos["mvlt_ce_smooth_fwd"][1] == ["const void*", "const long*", "long", "float", "const float*", "float*", "float*", "float*", "int", "int", "int", "int",
                                              "void*"]
    assert protos["mvlt_ce_smooth_bwd"][1] == ["const void*", "const long*", "long", "float", "const float*", "const float*", "const float*", "const float*", "void*",
                                              "int", "int", "int", "int", "int", "int", "void*"]


def test_loss_version_sources_and_the_older_tables():
    import mvlt_amd._lib as L
    from mvlt_amd import build, ops
    hdr = _loss_header()
    assert L.lib.mvlt_loss_version() == L.LOSS_VERSION == int(re.search(r"#define MVLT_LOSS_VERSION (\d+)", hdr).group(1)) == 1
    assert L.ABI_VERSION == 8 == L.lib.mvlt_abi_version() and L.EXT_VERSION == 1 and L.EMA_VERSION == 1 and L.OPT_VERSION == 1 and L.PLAN_VERSION == 3
    assert L.LAMB_VERSION == 1 == L.lib.mvlt_lamb_version()
    assert len(L.PROTOTYPES) == 61 and len(L.EXT_PROTOTYPES) == 3 and len(L.EMA_PROTOTYPES) == 3 and len(L.PLAN_PROTOTYPES) == 14 and len(L.OPT_PROTOTYPES) == 2
    assert len(L.LAMB_PROTOTYPES) == 5
    for name in LOSS:
        assert hasattr(L.lib, name) and name not in L.EXPORTS, name
    assert callable(ops.ce_smooth_fwd) and callable(ops.ce_smooth_bwd)
    src = open(build.__file__).read()
    assert src.count('"mvlt_hip_loss.h"') == 2                   # source_hash and _deps_mtime
    assert "loss.hip" in build._sources() and "elementwise.hip" in build._sources()
    kernels = open(os.path.join(ROOT, "mvlt_amd", "csrc", "loss.hip")).read()
    assert not re.search(r"atomic\w*\s*\(", kernels)             # no atomic call: plain stores in a fixed order
    for k in ("ce_smooth_fwd_kernel", "ce_smooth_finish_kernel", "ce_smooth_bwd_kernel"):
        assert k in kernels, k


def test_entry_points_refuse_bad_arguments_without_a_device():
    """no launch without a GPU: every call below must come back from the argument checks"""
    import mvlt_amd._lib as L
    lib, err = L.lib, lambda: L.lib.mvlt_last_error()
    a = 4096                                                     # any non-null, aligned address: the checks never dereference
    bad = lambda good, i, v: good[:i] + [v] + good[i + 1:]
    # logits, labels, ignore, e, weight, lse, smooth, acc, rows, V, ld, dtype, stream
    fwd = [a, a, -1, 0.1, None, a, a, a, 4, 8, 8, 1, None]
    f = lib.mvlt_ce_smooth_fwd
    for i in (0, 1, 5, 6, 7):
        assert f(*bad(fwd, i, None)) < 0 and b"mvlt_ce_smooth_fwd: null pointer" in err(), i
    for v in (0, -1):
        assert f(*bad(fwd, 9, v)) < 0 and b"V must be positive" in err(), v
    assert f(*bad(fwd, 10, 7)) < 0 and b"ld = 7 is smaller than V = 8" in err()
    for e in (-0.5, 1.0, 1.5, float("nan"), float("inf")):
        assert f(*bad(fwd, 3, e)) < 0 and b"label_smoothing must be in [0, 1)" in err(), e
    for d in (0, 2, -1):
        assert f(*bad(fwd, 11, d)) < 0 and b"must be fp32" in err(), d
    assert f(*bad(fwd, 8, -1)) < 0 and b"rows must not be negative" in err()
    for i, v in ((0, a + 2), (1, a + 4), (4, a + 2), (5, a + 1), (7, a + 2)):
        assert f(*bad(fwd, i, v)) < 0 and b"aligned" in err(), i
    # logits, labels, ignore, e, weight, lse, gscale, acc, dlogits, rows, V, ld, ldd, dtype, out_dtype, stream
    bwd = [a, a, -1, 0.1, None, a, a, a, a, 4, 8, 8, 8, 1, 0, None]
    f = lib.mvlt_ce_smooth_bwd
    for i in (0, 1, 5, 6, 7, 8):
        assert f(*bad(bwd, i, None)) < 0 and b"mvlt_ce_smooth_bwd: null pointer" in err(), i
    assert f(*bad(bwd, 10, 0)) < 0 and b"V must be positive" in err()
    assert f(*bad(bwd, 11, 7)) < 0 and b"ld = 7 is smaller" in err()
    assert f(*bad(bwd, 12, 7)) < 0 and b"ldd = 7 is smaller" in err()
    assert f(*bad(bwd, 3, 1.0)) < 0 and b"label_smoothing must be in [0, 1)" in err()
    assert f(*bad(bwd, 13, 0)) < 0 and b"must be fp32" in err()
    for d in (2, -1):
        assert f(*bad(bwd, 14, d)) < 0 and b"out_dtype" in err(), d
    assert f(*bad(bwd, 9, -1)) < 0 and b"rows must not be negative" in err()
    assert f(*bad(bwd, 9, 0)) == 0                               # nothing to do: no launch


def test_ops_have_no_cpu_path():
    from mvlt_amd import ops
    from mvlt_amd._lib import MVLTError
    z = lambda n: torch.zeros(n)
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.ce_smooth_fwd(z(32), lab, z(4), z(4), z(3), 4, 8, 8, label_smoothing=0.1)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.ce_smooth_bwd(z(32), lab, z(4), z(1), z(3), z(32), 4, 8, 8, 8, label_smoothing=0.1, weight=z(8))


def test_cpu_cross_entropy_forwards_both_options():
    from mvlt_amd import engine
    g = torch.Generator().manual_seed(0)
    x, lab = torch.randn(9, 48, generator=g), torch.randint(0, 48, (9,), generator=g)
    lab[3] = -100
    w = 0.5 + torch.rand(48, generator=g)
    assert torch.equal(engine.cross_entropy(x, lab), F.cross_entropy(x, lab))
    for kw in (dict(label_smoothing=0.1), dict(weight=w), dict(label_smoothing=0.3, weight=w)):
        got, want = engine.cross_entropy(x, lab, **kw), F.cross_entropy(x, lab, **kw)
        assert torch.equal(got, want) and not torch.equal(got, F.cross_entropy(x, lab)), kw
    lab[3] = -1
    assert torch.equal(engine.cross_entropy(x, lab, ignore_index=-1, label_smoothing=0.1, weight=w), F.cross_entropy(x, lab, ignore_index=-1, label_smoothing=0.1, weight=w))


def test_set_loss_options_and_compute_losses_on_the_cpu():
    """the options object, its validation, and the fallback path of compute_losses (CPU tensors take F.cross_entropy) with and without options"""
    from mvlt_amd import engine, pvlt
    from mvlt_amd._lib import MVLTError
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=20, loss_type=dict(mlm=1, itm=1, t2i=0, cls=1), pretrained_pth=None, img_size=96)
    assert isinstance(m.loss_options, pvlt.LossOptions) and not m.loss_options.active
    with pytest.raises(MVLTError, match=r"must be in \[0, 1\)"):
        m.set_loss_options(mlm_label_smoothing=1.0)
    with pytest.raises(MVLTError, match="48 entries"):
        m.set_loss_options(sup_cls_weight=torch.ones(122))
    with pytest.raises(MVLTError, match="positive and finite"):
        m.set_loss_options(sub_cls_weight=torch.zeros(122))
    assert not m.loss_options.active
    g = torch.Generator().manual_seed(1)
    w_sup, w_sub = 0.5 + torch.rand(48, generator=g), 0.5 + torch.rand(122, generator=g)
    keys = set(m.state_dict())
    opts = m.set_loss_options(mlm_label_smoothing=0.1, cls_label_smoothing=0.2, sup_cls_weight=w_sup, sub_cls_weight=w_sub.double())
    assert opts.active and opts.sub_cls_weight.dtype == torch.float32 and set(m.state_dict()) == keys and not any("weight" in n for n, _ in m.named_buffers())
    w_sup[0] = 99.0
    assert float(opts.sup_cls_weight[0]) != 99.0                 # a copy: the caller's tensor is not aliased
    Bn, Tn = 3, 20
    out = dict(mlm_logits=torch.randn(Bn, Tn, 30522, generator=g), itm_logits=torch.randn(Bn, 1, 2, generator=g), sup_cls_logits=torch.randn(Bn, 1, 48, generator=g),
               sub_cls_logits=torch.randn(Bn, 1, 122, generator=g), t2i_logits=None)
    mlm = torch.full((Bn, Tn), -1)
    mlm[:, ::4] = torch.randint(0, 30522, (Bn, 5), generator=g)
    itm, sup, sub = torch.randint(0, 2, (Bn,), generator=g), torch.randint(0, 48, (Bn,), generator=g), torch.randint(0, 122, (Bn,), generator=g)
    img = torch.zeros(Bn, 3, 8, 8)
    _, plain = engine.compute_losses(out, img, mlm, itm, sup, sub)
    _, none = engine.compute_losses(out, img, mlm, itm, sup, sub, options=pvlt.LossOptions())
    total, parts = engine.compute_losses(out, img, mlm, itm, sup, sub, options=opts)
    assert all(torch.equal(plain[k], none[k]) for k in plain)
    assert torch.equal(parts["loss_mlm"], F.cross_entropy(out["mlm_logits"].reshape(-1, 30522), mlm.view(-1), ignore_index=-1, label_smoothing=0.1))
    assert torch.equal(parts["loss_sup_cls"], F.cross_entropy(out["sup_cls_logits"].view(-1, 48), sup, weight=opts.sup_cls_weight, label_smoothing=0.2))
    assert torch.equal(parts["loss_sub_cls"], F.cross_entropy(out["sub_cls_logits"].view(-1, 122), sub, weight=opts.sub_cls_weight, label_smoothing=0.2))
    assert torch.equal(parts["loss_itm"], plain["loss_itm"])     # ITM has no options
    assert not torch.equal(parts["loss_mlm"], plain["loss_mlm"]) and float(total) == pytest.approx(sum(float(v) for v in parts.values()), rel=1e-6)
    m.set_loss_options()
    assert not m.loss_options.active and m.loss_options.sup_cls_weight is None

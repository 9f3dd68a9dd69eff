"""CPU: the host side of the fused weight EMA (docs/ema.md) -- include/mvlt_hip_ema.h and mvlt_amd/_lib.py EMA_PROTOTYPES agree, the library exports the
entry points and refuses bad arguments without a launch, FusedModelEma has no CPU path, and its state works before the averaged model's store exists."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_host_cpu import _header_abi, _toy_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMA = ("mvlt_ema_version", "mvlt_ema_update", "mvlt_ema_update_buffers")


def _ema_header():
    return open(os.path.join(ROOT, "include", "mvlt_hip_ema.h")).read()


def test_ema_header_and_binding_agree():
    """name by name, parameter by parameter (the rule tests/test_host_cpu.py applies to mvlt_hip.h and PROTOTYPES)"""
    import mvlt_amd._lib as L
    hdr = _ema_header()
    protos, structs = _header_abi(hdr)
    assert set(protos) == set(L.EMA_PROTOTYPES) == set(EMA) and not structs
    # three disjoint tables: additions, not overrides
    assert not set(L.EMA_PROTOTYPES) & set(L.PROTOTYPES) and not set(L.EMA_PROTOTYPES) & set(L.EXT_PROTOTYPES) and not set(L.EXT_PROTOTYPES) & set(L.PROTOTYPES)
    scalars = {"int": C.c_int, "long": C.c_long, "float": C.c_float}
    for name, (ret, params) in protos.items():
        restype, argtypes = L.EMA_PROTOTYPES[name]
        fn = getattr(L.lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (ctype, written) in enumerate(zip(argtypes, params)):
            want = scalars[written] if written in scalars else C.c_void_p          # every pointer (`const int64_t*` -- the device table -- included) is c_void_p
            assert written in scalars or written.endswith("*"), (name, i, written)
            assert ctype is want, (name, i, written, ctype)
    assert protos["mvlt_ema_update"][1] == ["float*", "const float*", "void*", "long", "float", "float", "const uint8_t*", "void*"]
    assert protos["mvlt_ema_update_buffers"][1] == ["const int64_t*", "int", "float", "float", "void*"]
    for cite in ("engine_grid_masking.py:130-131", "main_vl.py:16", "main_vl.py:295", "main_vl.py:452"):
        assert cite in hdr, cite


def test_ema_version_and_exports():
    import mvlt_amd._lib as L
    from mvlt_amd import ops
    assert L.lib.mvlt_ema_version() == L.EMA_VERSION == int(re.search(r"#define MVLT_EMA_VERSION (\d+)", _ema_header()).group(1)) == 1
    for name in EMA:
        assert hasattr(L.lib, name), name
    assert callable(ops.ema_update) and callable(ops.ema_update_buffers)
    assert L.ABI_VERSION == 8 and L.EXT_VERSION == 1 and not set(EMA) & set(L.EXPORTS)


def test_ema_bad_arguments_are_error_codes():
    """no launch without a GPU: every call below must come back from the argument checks"""
    import mvlt_amd._lib as L
    lib, err = L.lib, lambda: L.lib.mvlt_last_error()
    p = 4096                                                   # any non-null, aligned address: the checks never dereference
    nan, inf = float("nan"), float("inf")
    good = [p, p, None, 8, 0.5, 0.5, None, None]               # ema, p, ema_bf16, n, decay, one_minus_decay, mask, stream
    bad = lambda i, v: good[:i] + [v] + good[i + 1:]
    for args in (bad(0, None), bad(1, None)):                  # each required pointer missing in turn
        assert lib.mvlt_ema_update(*args) < 0 and b"mvlt_ema_update:" in err()
    for n in (6, 2, 9):
        assert lib.mvlt_ema_update(*bad(3, n)) < 0 and b"mvlt_ema_update:" in err() and b"multiple of 4" in err()
    for n in (-4, -1):
        assert lib.mvlt_ema_update(*bad(3, n)) < 0 and b"mvlt_ema_update:" in err()
    for d in (-0.001, 1.001, nan, inf, -inf):
        assert lib.mvlt_ema_update(*bad(4, d)) < 0 and b"mvlt_ema_update:" in err() and b"[0, 1]" in err(), d
        assert lib.mvlt_ema_update(*bad(5, d)) < 0 and b"mvlt_ema_update:" in err() and b"[0, 1]" in err(), d
    assert lib.mvlt_ema_update(*bad(3, 0)) == 0                # nothing to do: no launch
    for d in (0.0, 1.0):                                       # the ends of the interval are decays
        assert lib.mvlt_ema_update(*bad(3, 0)[:4], d, 1.0 - d, None, None) == 0

    assert lib.mvlt_ema_update_buffers(None, 2, 0.5, 0.5, None) < 0 and b"mvlt_ema_update_buffers:" in err()
    assert lib.mvlt_ema_update_buffers(p, -1, 0.5, 0.5, None) < 0 and b"mvlt_ema_update_buffers:" in err()
    for d in (-0.001, 1.001, nan, inf):
        assert lib.mvlt_ema_update_buffers(p, 2, d, 0.5, None) < 0 and b"mvlt_ema_update_buffers:" in err() and b"[0, 1]" in err(), d
        assert lib.mvlt_ema_update_buffers(p, 2, 0.5, d, None) < 0 and b"mvlt_ema_update_buffers:" in err() and b"[0, 1]" in err(), d
    assert lib.mvlt_ema_update_buffers(p, 0, 0.5, 0.5, None) == 0


def test_ema_has_no_cpu_path():
    from mvlt_amd import ops
    from mvlt_amd._lib import MVLTError
    from mvlt_amd.optim import FusedModelEma
    m = _toy_store()                                           # its store is materialised on the CPU
    e = FusedModelEma(m, decay=0.5)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        e.update(m)
    assert e.updates == 0
    z = torch.zeros(8)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.ema_update(z, z.clone(), None, 8, 0.5, 0.5)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.ema_update_buffers(torch.zeros(4, dtype=torch.int64), 1, 0.5, 0.5)


def test_ema_state_before_its_store_exists():
    from mvlt_amd.optim import FusedModelEma
    m = _toy_store()
    e = FusedModelEma(m)
    assert e.module is e.ema and type(e.ema) is type(m) and not e.ema.training
    assert e.ema.store is not m.store and e.ema.store.P is None and e.ema.store.module is e.ema
    assert all(not p.requires_grad for p in e.ema.parameters()) and all(p.requires_grad for p in m.parameters())
    sd, want = e.state_dict(), m.state_dict()
    assert list(sd) == list(want) + ["_ema_updates"] and sd["_ema_updates"] == 0 and e.updates == 0
    for k, v in want.items():
        assert sd[k].shape == v.shape and torch.equal(sd[k].view(torch.int32), v.view(torch.int32)), k
        assert sd[k].data_ptr() != v.data_ptr(), k                                # a copy, never an alias
    # a checkpoint loaded before the store exists waits in the averaged model's parameters, with or without the counter
    other = _toy_store()
    ck = other.state_dict()
    e.load_state_dict(ck)
    assert e.updates == 0 and e.ema.store.P is None
    ck["_ema_updates"] = 7
    e.load_state_dict(ck)
    assert e.updates == 7 and "_ema_updates" in ck                                # the caller's dict stays as it was
    got = e.state_dict()
    assert got["_ema_updates"] == 7
    for k, v in other.state_dict().items():
        assert torch.equal(got[k], v), k
    # ... and the store picks them up when it is built
    e.ema.store.materialize(torch.device("cpu"))
    for k, v in other.state_dict().items():
        assert torch.equal(e.ema.state_dict()[k], v), k
    assert list(e.ema.store.offsets.items()) == list(m.store.offsets.items())


def test_ema_checkpoint_loads_into_a_plain_model():
    """the extra key does not stand in the way of model.load_state_dict(model_ema.state_dict()), strict"""
    from mvlt_amd import pvlt
    from mvlt_amd.optim import FusedModelEma
    lt = dict(mlm=1, itm=1, t2i=1, cls=1)
    build = lambda: pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=20, loss_type=lt, pretrained_pth=None, img_size=96)
    m = build()
    e = FusedModelEma(m)
    sd, want = e.state_dict(), m.state_dict()
    assert list(sd) == list(want) + ["_ema_updates"]
    assert all(torch.equal(sd[k], v) and sd[k].dtype == v.dtype for k, v in want.items())
    assert sd["mlm_head.mlm_decoder.weight"].data_ptr() == sd["text_embeddings.word_embeddings.weight"].data_ptr()       # still tied, to its own copy
    assert sd["mlm_head.mlm_decoder.weight"].data_ptr() != want["mlm_head.mlm_decoder.weight"].data_ptr()
    assert any(k.endswith("num_batches_tracked") for k in sd) and any(k.endswith("running_var") for k in sd)
    plain = build()
    plain.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, want[k]) for k, v in plain.state_dict().items())


def test_ema_warmup_decay_sequence():
    from mvlt_amd.optim import FusedModelEma
    e = FusedModelEma(_toy_store(), decay=0.9999, warmup=True)
    assert [e.decay_at(t) for t in (1, 2, 3, 4, 5)] == [2 / 11, 3 / 12, 4 / 13, 5 / 14, 6 / 15]
    assert e.decay_at(10 ** 9) == 0.9999 and e.decay_at(89_989) < 0.9999 and e.decay_at(89_991) == 0.9999      # (1 + t) / (10 + t) reaches 0.9999 at t = 89,990
    e.decay = 0.2                                              # a plain attribute: the cap moves with it
    assert [e.decay_at(t) for t in (1, 2, 3)] == [2 / 11, 0.2, 0.2]
    flat = FusedModelEma(_toy_store(), decay=0.99)
    assert [flat.decay_at(t) for t in (1, 5, 10 ** 9)] == [0.99] * 3

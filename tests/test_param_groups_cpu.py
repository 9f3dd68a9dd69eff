"""CPU: the host side of per-group learning rates (docs/param_groups.md) -- include/mvlt_hip_opt.h and mvlt_amd/_lib.py OPT_PROTOTYPES agree and the older
tables are as they were, mvlt_adamw_step_groups refuses bad arguments without a launch, FusedAdamW(param_groups=...) validates its groups and builds the
group byte from a CPU store, layer_ids / layer_decay_groups give the closed-form ids and rates, and CosineLRScheduler keeps them."""
import ctypes as C
import math
import os
import re
import types

import pytest
import torch

from tests.test_host_cpu import _header_abi, _toy_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = ("mvlt_opt_version", "mvlt_adamw_step_groups")
LT = dict(mlm=1, itm=1, t2i=1, cls=1)


def _opt_header():
    return open(os.path.join(ROOT, "include", "mvlt_hip_opt.h")).read()


@pytest.fixture(scope="module")
def tiny():
    from mvlt_amd import pvlt
    return pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=20, loss_type=LT, pretrained_pth=None, img_size=96)


# ------------------------------------------------------------------------------------------------------------------ header, binding, guards
def test_opt_header_and_binding_agree():
    """name by name, parameter by parameter (the rule tests/test_ema_cpu.py applies to mvlt_hip_ema.h and EMA_PROTOTYPES)"""
    import mvlt_amd._lib as L
    hdr = _opt_header()
    protos, structs = _header_abi(hdr)
    assert set(protos) == set(L.OPT_PROTOTYPES) == set(OPT) and not structs
    older = set(L.PROTOTYPES) | set(L.EXT_PROTOTYPES) | set(L.EMA_PROTOTYPES) | set(L.PLAN_PROTOTYPES)
    assert not set(OPT) & older                                  # an addition, not an override
    scalars = {"int": C.c_int, "long": C.c_long, "float": C.c_float}
    for name, (ret, params) in protos.items():
        restype, argtypes = L.OPT_PROTOTYPES[name]
        fn = getattr(L.lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (ctype, written) in enumerate(zip(argtypes, params)):
            want = scalars[written] if written in scalars else C.c_void_p
            assert written in scalars or written.endswith("*"), (name, i, written)
            assert ctype is want, (name, i, written, ctype)
    assert protos["mvlt_adamw_step_groups"][1] == ["float*", "const float*", "float*", "float*", "void*", "long", "const float*", "const uint8_t*",
                                                   "const float*", "int", "const float*", "const float*", "void*"]


def test_opt_version_and_the_older_tables():
    import mvlt_amd._lib as L
    from mvlt_amd import ops
    assert L.lib.mvlt_opt_version() == L.OPT_VERSION == int(re.search(r"#define MVLT_OPT_VERSION (\d+)", _opt_header()).group(1)) == 1
    assert L.ABI_VERSION == 8 == L.lib.mvlt_abi_version() and L.EXT_VERSION == 1 == L.lib.mvlt_ext_version() and L.EMA_VERSION == 1 == L.lib.mvlt_ema_version()
    assert len(L.PROTOTYPES) == 61 and set(L.EXT_PROTOTYPES) == {"mvlt_ext_version", "mvlt_step_gate", "mvlt_adamw_step_gated"}
    assert set(L.EMA_PROTOTYPES) == {"mvlt_ema_version", "mvlt_ema_update", "mvlt_ema_update_buffers"}
    for name in OPT:
        assert hasattr(L.lib, name) and name not in L.EXPORTS, name
    assert callable(ops.adamw_step_groups)
    hdr = _opt_header()
    assert int(re.search(r"#define MVLT_OPT_FROZEN (\d+)", hdr).group(1)) == ops.OPT_FROZEN == 255
    assert int(re.search(r"#define MVLT_OPT_MAX_GROUPS (\d+)", hdr).group(1)) == ops.OPT_MAX_GROUPS == 254
    from mvlt_amd import build
    src = open(build.__file__).read()
    assert src.count('"mvlt_hip_opt.h"') == 2                    # source_hash and _deps_mtime


def test_step_groups_refusals_are_error_codes():
    """no launch without a GPU: every call below must come back from the argument checks"""
    import mvlt_amd._lib as L
    lib, err = L.lib, lambda: L.lib.mvlt_last_error()
    a = 4096                                                    # any non-null, aligned address: the checks never dereference
    good = [a, a, a, a, None, 8, a, a, a, 3, None, None, None]  # p, g, m, v, p_bf16, n, hp, group_of, table, n_groups, gscale_dev, gate, stream
    bad = lambda i, v: good[:i] + [v] + good[i + 1:]
    f = lib.mvlt_adamw_step_groups
    for i in (0, 1, 2, 3, 6, 7, 8):                             # each required pointer missing in turn
        assert f(*bad(i, None)) < 0 and b"mvlt_adamw_step_groups:" in err(), i
    for n in (6, 2, 9, -4):
        assert f(*bad(5, n)) < 0 and b"mvlt_adamw_step_groups:" in err() and b"multiple of 4" in err(), n
    for k in (255, 256, 0, -1):
        assert f(*bad(9, k)) < 0 and b"n_groups" in err(), k
    both = bad(10, a)
    both[11] = a
    assert f(*both) < 0 and b"both gscale_dev and gate" in err()
    for i, v in ((0, a + 8), (1, a + 4), (4, a + 2), (7, a + 1), (8, a + 4)):
        assert f(*bad(i, v)) < 0 and b"aligned" in err(), i
    assert f(*bad(5, 0)) == 0                                   # nothing to do: no launch
    assert f(*bad(9, 254)[:5], 0, *bad(9, 254)[6:]) == 0        # 254 groups are taken


def test_step_groups_has_no_cpu_path():
    from mvlt_amd import ops
    from mvlt_amd._lib import MVLTError
    z = lambda: torch.zeros(8)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.adamw_step_groups(z(), z(), z(), z(), None, 8, z(), torch.zeros(8, dtype=torch.uint8), torch.zeros(2), 1)


# ------------------------------------------------------------------------------------------------------------------ FusedAdamW(param_groups=...)
def test_constructor_without_the_keyword_builds_the_two_groups(tiny):
    from mvlt_amd.optim import FusedAdamW
    opt = FusedAdamW(tiny, lr=2e-3, weight_decay=0.05)
    same = FusedAdamW(tiny, lr=2e-3, weight_decay=0.05, param_groups=None)
    named = list(tiny.named_parameters())
    nd = [p for n, p in named if p.dim() == 1 or n.endswith(".bias")]
    dec = [p for n, p in named if not (p.dim() == 1 or n.endswith(".bias"))]
    for o in (opt, same):
        g0, g1 = o.param_groups
        assert [id(p) for p in g0["params"]] == [id(p) for p in nd] and [id(p) for p in g1["params"]] == [id(p) for p in dec]
        assert g0["weight_decay"] == 0.0 and g1["weight_decay"] == 0.05 and g0["lr"] == g1["lr"] == 2e-3
        assert g0["betas"] == g1["betas"] == (0.9, 0.999) and g0["eps"] == g1["eps"] == 1e-8


def test_group_validation_names_the_offender(tiny):
    from mvlt_amd.optim import FusedAdamW
    named = list(tiny.named_parameters())
    ps = [p for _, p in named]
    with pytest.raises(ValueError, match=re.escape(repr(named[-1][0])) + " is in no group"):
        FusedAdamW(tiny, param_groups=[dict(params=ps[:-1])])
    with pytest.raises(ValueError, match=re.escape(repr(named[3][0])) + r" is in two groups, group 0 \('a'\) and group 1"):
        FusedAdamW(tiny, param_groups=[dict(params=ps[:4], name="a"), dict(params=ps[3:])])
    singles = lambda k: [dict(params=[p], lr=1e-4 * (i + 1), name=f"g{i}", lr_scale=0.5) for i, p in enumerate(ps[:k])]
    assert 200 < len(ps) < 254                                   # (the model has fewer tensors than the byte has values: empty groups make up the count)
    with pytest.raises(ValueError, match="255 parameter groups"):
        FusedAdamW(tiny, param_groups=singles(len(ps)) + [dict(params=[]) for _ in range(255 - len(ps))])
    with pytest.raises(ValueError, match=r"group 1 \('heads'\) has betas .* eps 1e-06"):
        FusedAdamW(tiny, param_groups=[dict(params=ps[:4]), dict(params=ps[4:], eps=1e-6, name="heads")])
    with pytest.raises(ValueError, match=r"group 0 has betas \(0.8, 0.999\)"):
        FusedAdamW(tiny, param_groups=[dict(params=ps, betas=(0.8, 0.999))])
    with pytest.raises(ValueError, match="not a parameter of the model"):
        FusedAdamW(tiny, param_groups=[dict(params=ps + [torch.nn.Parameter(torch.zeros(3))])])
    # 254 groups are taken, and keys the optimizer does not know stay in the group untouched
    opt = FusedAdamW(tiny, lr=1e-3, weight_decay=0.05,
                     param_groups=singles(200) + [dict(params=ps[200:])] + [dict(params=[]) for _ in range(53)])
    assert len(opt.param_groups) == 254 and opt.param_groups[7]["name"] == "g7" and opt.param_groups[7]["lr_scale"] == 0.5
    assert opt.param_groups[7]["lr"] == 8e-4 and opt.param_groups[7]["weight_decay"] == 0.05 and opt.param_groups[200]["lr"] == 1e-3
    sd = opt.state_dict()
    assert sd["param_groups"][7]["name"] == "g7" and sd["fused"]["step"] == 0
    opt.load_state_dict(sd)
    assert opt.param_groups[7]["lr_scale"] == 0.5 and opt.param_groups[7]["lr"] == 8e-4


def test_group_byte_and_decay_mask_from_a_cpu_store():
    """both byte maps are built from the store's layout alone (tests/test_freeze_cpu.py does the same for the mask)"""
    from mvlt_amd import ops
    from mvlt_amd.optim import FusedAdamW
    m = _toy_store()
    named = dict(m.named_parameters())
    heads = [n for n in named if n.startswith("head")]
    biases = [n for n in named if n.endswith(".bias")]
    rest = [n for n in named if n not in heads and n not in biases]
    groups = [dict(params=[named[n] for n in rest], lr=1e-4, weight_decay=0.05), dict(params=[named[n] for n in biases], lr=1e-4, weight_decay=0.0),
              dict(params=[named[n] for n in heads], lr=1e-3, weight_decay=0.01)]
    named["block2.bias"].requires_grad_(False)
    named["text_embed3.weight"].requires_grad_(False)
    opt = FusedAdamW(m, param_groups=groups)
    S = opt._ensure()
    assert opt._hp.numel() == 8 + 2 * 3
    want_g = {**{n: 0 for n in rest}, **{n: 1 for n in biases}, **{n: 2 for n in heads}}
    covered = torch.zeros(S.total, dtype=torch.bool)
    for name, p in S.params.items():
        off, n, _ = S.offsets[name]
        covered[off:off + n] = True
        gb, mk = opt._group_of[off:off + n], opt._wd_mask[off:off + n]
        if not p.requires_grad:
            assert bool((gb == ops.OPT_FROZEN).all()) and bool((mk == ops.ADAMW_FROZEN).all()), name
        else:
            assert bool((gb == want_g[name]).all()) and bool((mk == (0 if name in biases else 1)).all()), name
    assert int(covered.sum()) < S.total                          # the toy has alignment gaps (3-element biases)
    assert bool((opt._group_of[~covered] == ops.OPT_FROZEN).all()) and bool((opt._wd_mask[~covered] == 0).all())
    first = opt._group_of
    opt._ensure()
    assert opt._group_of is first                                # nothing flipped: not rebuilt
    named["block2.bias"].requires_grad_(True)
    opt._ensure()
    off, n, _ = S.offsets["block2.bias"]
    assert opt._group_of is not first and bool((opt._group_of[off:off + n] == 1).all())


# ------------------------------------------------------------------------------------------------------------------ layer-wise lr decay
def _forward_rank(name, depths):
    """where a parameter first acts in the forward pass: (stage, 0 = the stage's embeddings / 1 + j = block j / big = closing norm); the BERT block first, heads last"""
    top, _, rest = name.partition(".")
    if top == "text_embeddings":
        return (0, 0)
    if "head" in top:
        return (len(depths) + 1, 0)
    stage = int(re.search(r"(\d+)$", top).group(1))
    if top.startswith("block"):
        return (stage, 1 + int(rest.split(".")[0]))
    return (stage, 10 ** 6 if top.startswith("norm") else 0)


def test_layer_ids_on_pvlt_tiny(tiny):
    from mvlt_amd.optim import layer_ids
    ids = layer_ids(tiny)
    depths = tuple(tiny.depths)
    L = sum(depths)
    names = [n for n, _ in tiny.named_parameters()]
    assert sorted(ids) == sorted(names) and all(isinstance(i, int) and 0 <= i <= L + 1 for i in ids.values())
    assert set(ids.values()) == set(range(L + 2))
    order = sorted(names, key=lambda n: _forward_rank(n, depths))
    seq = [ids[n] for n in order]
    assert seq == sorted(seq)                                    # monotone along the forward order
    heads = [n for n in names if "head" in n.split(".")[0]]
    assert len(heads) > 40 and {ids[n] for n in heads} == {L + 1} and all(ids[n] <= L for n in names if n not in heads)
    assert any(n.startswith("t2i_head.") for n in heads) and any(n.startswith("mlm_head_embed.") for n in heads)
    for n in ("text_embeddings.word_embeddings.weight", "text_embeddings.LayerNorm.bias", "patch_embed1.proj.weight", "text_embed1.0.weight", "pos_embed1",
              "text_pos_embed1"):
        assert ids[n] == 0, n
    first = 1
    for s, d in enumerate(depths, start=1):
        for j in range(d):
            assert ids[f"block{s}.{j}.attn.q.weight"] == ids[f"block{s}.{j}.mlp.fc2.bias"] == first + j
        if s > 1:
            for n in (f"patch_embed{s}.proj.weight", f"patch_embed{s}.norm.bias", f"text_embed{s}.0.weight", f"pos_embed{s}", f"text_pos_embed{s}"):
                assert ids[n] == first, n
        first += d


def test_layer_ids_is_a_function_of_names_and_depths():
    from mvlt_amd.optim import layer_ids
    names = ["text_embeddings.word_embeddings.weight", "pos_embed1", "block1.0.w", "block1.2.w", "norm1.weight", "patch_embed2.proj.weight", "block2.0.w",
             "block2.1.w", "norm2.bias", "cls_head.weight"]
    fake = types.SimpleNamespace(depths=(3, 2), named_parameters=lambda: [(n, None) for n in names], store=None)
    assert layer_ids(fake) == dict(zip(names, [0, 0, 1, 3, 3, 4, 4, 5, 5, 6]))
    for bad in ("block3.0.w", "block2.2.w", "mystery.weight", "stem9.weight"):
        fake.named_parameters = lambda bad=bad: [(bad, None)]
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            layer_ids(fake)


def test_layer_decay_groups_closed_form(tiny):
    from mvlt_amd.optim import FusedAdamW, layer_decay_groups, layer_ids
    lr, wd, ld = 2e-3, 0.05, 0.75
    groups = layer_decay_groups(tiny, lr, wd, ld)
    ids, L = layer_ids(tiny), sum(tiny.depths)
    assert len(groups) <= 2 * (L + 2) <= 254 and len({g["name"] for g in groups}) == len(groups)
    names = {id(p): n for n, p in tiny.named_parameters()}
    seen = []
    for g in groups:
        i, kind = re.fullmatch(r"layer_(\d+)_(decay|no_decay)", g["name"]).groups()
        i = int(i)
        assert g["lr_scale"] == ld ** (L + 1 - i) and g["lr"] == lr * ld ** (L + 1 - i)
        assert g["weight_decay"] == (wd if kind == "decay" else 0.0) and g["params"]
        for p in g["params"]:
            n = names[id(p)]
            assert ids[n] == i and (p.dim() == 1 or n.endswith(".bias")) == (kind == "no_decay"), n
            seen.append(n)
    assert sorted(seen) == sorted(names.values())                # every parameter in exactly one group
    assert [g["lr"] for g in groups] == sorted(g["lr"] for g in groups) and groups[-1]["lr"] == lr and groups[0]["lr"] == lr * ld ** (L + 1)
    opt = FusedAdamW(tiny, param_groups=groups)                  # goes straight in
    assert [g["name"] for g in opt.param_groups] == [g["name"] for g in groups]
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in groups]
    # pvlt_large (depths 3, 8, 27, 3) stays under the kernel's 254 groups
    assert 2 * (3 + 8 + 27 + 3 + 2) <= 254


def test_cosine_scheduler_keeps_the_group_rates(tiny):
    from mvlt_amd.optim import FusedAdamW, layer_decay_groups
    from mvlt_amd.sched import create_scheduler
    lr, ld, L = 2e-3, 0.75, sum(tiny.depths)
    opt = FusedAdamW(tiny, param_groups=layer_decay_groups(tiny, lr, 0.05, ld))
    base = [lr * g["lr_scale"] for g in opt.param_groups]
    args = types.SimpleNamespace(sched="cosine", epochs=20, min_lr=1e-6, warmup_lr=1e-7, warmup_epochs=4, cooldown_epochs=3)
    sched, num_epochs = create_scheduler(args, opt)
    assert num_epochs == 23 and all(g["lr"] == 1e-7 for g in opt.param_groups)            # timm's warm-up start value
    for epoch in (2, 11, 21):                                    # warm-up, mid-cosine, cool-down
        sched.step(epoch)
        for g, b in zip(opt.param_groups, base):
            if epoch < 4:
                want = 1e-7 + epoch * (b - 1e-7) / 4
            elif epoch < 20:
                want = 1e-6 + 0.5 * (b - 1e-6) * (1 + math.cos(math.pi * epoch / 20))
            else:
                want = 1e-6
            assert g["lr"] == pytest.approx(want, rel=1e-12), (epoch, g["name"])
        lrs = [g["lr"] for g in opt.param_groups]
        assert (len(set(lrs)) == 1) == (epoch == 21)             # the ratios hold while the schedule is above its floor

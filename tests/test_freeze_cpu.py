"""No GPU: frozen parameters (requires_grad=False) -- the pure-Python backward plan (mvlt_amd.plan.backward_plan) for the settings a fine-tune run
uses, the third value of mvlt_adamw_step's mask byte in the header, and FusedAdamW's mask following requires_grad (built here from a CPU store)."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

LT = dict(mlm=1, itm=1, t2i=0, cls=0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMBEDS = ("patch_embed{}", "text_embed{}", "pos_embed{}", "text_pos_embed{}")


@pytest.fixture
def model():
    from mvlt_amd import pvlt
    return pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=16, loss_type=LT, pretrained_pth=None, drop_path_rate=0.0)


def freeze(m, *prefixes):
    for n, p in m.named_parameters():
        if n.startswith(prefixes):
            p.requires_grad_(False)


def stage_prefixes(*stages):
    return tuple(f"block{i}." for i in stages) + tuple(e.format(i) for i in stages for e in EMBEDS)


def plan_of(m):
    from mvlt_amd.plan import backward_plan
    return backward_plan(m)


def test_unit_order(model):
    p = plan_of(model)
    want = ["mlm_head", "itm_head"]
    for i in (4, 3, 2, 1):
        want += [f"block{i}.1", f"block{i}.0", f"embed{i}"]
    want.append("text_embeddings")
    assert [u.name for u in p.units] == want
    # every parameter of the model belongs to exactly one launch group of one unit -- but for the tied table, which the MLM decoder writes as well
    seen = [n for u in p.units for g in u.params.values() for n in g]
    names = [n for n, _ in model.named_parameters()]
    assert sorted(set(seen)) == sorted(names)
    assert sorted(n for n in seen if seen.count(n) > 1) == ["text_embeddings.word_embeddings.weight"] * 2


def test_everything_trainable(model):
    p = plan_of(model)
    assert p.cut_unit.name == "text_embeddings" and p.trunk_save
    for u in p.units:
        assert u.wgrad and u.save, u
        assert u.dgrad == (u.name != "text_embeddings"), u
        assert all(on for k, on in u.launches.items() if u.params[k]), u


def test_only_heads_trainable(model):
    freeze(model, *stage_prefixes(1, 2, 3, 4), "text_embeddings.")
    p = plan_of(model)
    assert p.cut_unit.name == "itm_head" and not p.trunk_save
    for u in p.units:
        if u.kind == "head":
            assert u.wgrad and u.save and not u.dgrad, u
        else:
            assert not (u.wgrad or u.dgrad or u.save), u
    assert p.by["mlm_head"].launches["table"] is False            # the tied table is frozen with text_embeddings
    assert p.by["mlm_head"].launches["bias"] and p.by["mlm_head"].launches["dense"]


def test_text_embeddings_frozen(model):
    ref = plan_of(model).signature()
    freeze(model, "text_embeddings.")
    p = plan_of(model)
    assert p.cut_unit.name == "embed1"
    assert p.by["mlm_head"].launches["table"] is False and p.by["mlm_head"].wgrad
    assert not p.by["embed1"].dgrad and p.by["embed1"].wgrad and p.by["embed1"].save
    bert = p.by["text_embeddings"]
    assert not (bert.wgrad or bert.dgrad or bert.save)
    skip = {"mlm_head", "embed1", "text_embeddings"}
    assert [s for s in p.signature() if s[0] not in skip] == [s for s in ref if s[0] not in skip]


def test_lower_stages_and_text_embeddings_frozen(model):
    ref = plan_of(model)
    freeze(model, *stage_prefixes(1, 2), "text_embeddings.")
    p = plan_of(model)
    assert p.cut_unit.name == "embed3"
    e3 = p.by["embed3"]
    assert e3.wgrad and e3.save and not e3.dgrad
    for name in ("block4.1", "block4.0", "embed4", "block3.1", "block3.0"):
        a, b = p.by[name], ref.by[name]
        assert (a.wgrad, a.dgrad, a.save, a.launches) == (b.wgrad, b.dgrad, b.save, b.launches), name
    for u in p.units[p.cut + 1:]:
        assert not (u.wgrad or u.dgrad or u.save), u


def test_one_frozen_weight_changes_nothing(model):
    ref = plan_of(model).signature()
    model.block2[1].mlp.fc1.weight.requires_grad_(False)
    assert plan_of(model).signature() == ref                       # fc1.bias keeps the launch: the optimizer's mask protects the weight


def test_one_trainable_weight(model):
    for q in model.parameters():
        q.requires_grad_(False)
    model.block2[1].mlp.fc1.weight.requires_grad_(True)
    p = plan_of(model)
    cut = p.cut_unit
    assert cut.name == "block2.1" and cut.wgrad and cut.save and not cut.dgrad
    assert cut.launches == dict(fc1=True, fc2=False, proj=False, q=False, kv=False, sr=False, ln=False)
    assert cut.only("fc1", "fc2")
    above = p.units[:p.cut]
    assert [u.name for u in above] == ["mlm_head", "itm_head", "block4.1", "block4.0", "embed4", "block3.1", "block3.0", "embed3"]
    for u in above:
        assert u.dgrad and u.save and not u.wgrad and not any(u.launches.values()), u
    for u in p.units[p.cut + 1:]:
        assert not (u.wgrad or u.dgrad or u.save), u
    assert [u.name for u in p.units if u.wgrad] == ["block2.1"]


def test_nothing_trainable(model):
    for q in model.parameters():
        q.requires_grad_(False)
    p = plan_of(model)
    assert p.cut is None and p.cut_unit is None and not p.trunk_save and not any(u.save for u in p.units)


def test_header_documents_the_frozen_mask_value():
    from mvlt_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    assert re.search(r"#define\s+MVLT_ABI_VERSION\s+8\b", hdr) and _lib.ABI_VERSION == 8
    assert re.search(r"#define\s+MVLT_ADAMW_FROZEN\s+2\b", hdr) and ops.ADAMW_FROZEN == 2
    doc = hdr[hdr.index("torch.optim.AdamW step over a flat fp32 buffer"):hdr.index("int mvlt_adamw_step(")]
    assert "MVLT_ADAMW_FROZEN" in doc and "NOT written" in doc and "decay_mask" in doc


def test_fused_adamw_mask_follows_requires_grad(model):
    """the mask is built from the store's layout alone, so a CPU-materialised store is enough"""
    from mvlt_amd.optim import FusedAdamW
    freeze(model, "block2.")
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.05)
    named = dict(model.named_parameters())
    assert sum(len(g["params"]) for g in opt.param_groups) == len(named)           # frozen parameters are in the groups: requires_grad decides per step
    S = model.store
    S.materialize(torch.device("cpu"))
    opt._ensure()

    def check():
        mask = opt._wd_mask
        covered = torch.zeros(S.total, dtype=torch.bool)
        for name, p in S.params.items():
            off, n, _ = S.offsets[name]
            want = 2 if not p.requires_grad else (0 if (p.dim() == 1 or name.endswith(".bias")) else 1)
            assert bool((mask[off:off + n] == want).all()), name
            covered[off:off + n] = True
        assert bool((mask[~covered] == 0).all())                                 # alignment gaps: as before
    check()
    lo, hi = S.prefix_range(("block2.",))
    assert opt._all_frozen(lo, hi) and opt._all_frozen(lo + 8, hi - 8) and not opt._all_frozen(lo - 8, hi) and not opt._all_frozen(0, S.total)
    first = opt._wd_mask
    opt._ensure()
    assert opt._wd_mask is first                                                 # nothing flipped: not rebuilt
    model.block2[0].attn.q.weight.requires_grad_(True)
    model.block1[0].norm1.bias.requires_grad_(False)
    opt._ensure()
    assert opt._wd_mask is not first
    check()
    assert not opt._all_frozen(lo, hi)
    o, n, _ = S.offsets["block1.0.norm1.bias"]
    assert opt._all_frozen(o, o + n)


_PLAN_CHILD = """
import json, sys
import mvlt_amd.plan as plan
assert not any(m in sys.modules for m in ("mvlt_amd._lib", "mvlt_amd.ops", "mvlt_amd.pvlt")), sorted(m for m in sys.modules if m.startswith("mvlt_amd"))
spec = json.load(sys.stdin)

class P:
    def __init__(self, on):
        self.requires_grad = on

class M:
    depths, loss_type = spec["depths"], spec["loss_type"]
    def named_parameters(self):
        return [(n, P(on)) for n, on in spec["params"]]

print(json.dumps(plan.backward_plan(M()).signature()))
"""


def _child(code, stdin="", **env):
    return subprocess.run([sys.executable, "-c", code], input=stdin, capture_output=True, text=True, cwd=ROOT, env={**os.environ, **env}, timeout=120)


def test_plan_needs_no_library(model):
    """a fresh process whose MVLT_HIP_LIB names no file imports mvlt_amd.plan and plans pvlt_tiny (its parameter names, flags, depths and loss types handed
    over as data: the model classes live behind the library) -- the same plan as in this process"""
    freeze(model, *stage_prefixes(1, 2), "text_embeddings.")
    spec = dict(depths=list(model.depths), loss_type=dict(model.loss_type), params=[(n, p.requires_grad) for n, p in model.named_parameters()])
    r = _child(_PLAN_CHILD, json.dumps(spec), MVLT_HIP_LIB=os.path.join(ROOT, "no", "such", "libmvlt_hip.so"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == json.loads(json.dumps(plan_of(model).signature()))
    r = _child("import mvlt_amd._lib", MVLT_HIP_LIB=os.path.join(ROOT, "no", "such", "libmvlt_hip.so"))
    assert r.returncode != 0 and "is missing" in r.stderr                     # (the variable does reach the child: the binding itself refuses)


@pytest.mark.parametrize("module", ["schedule", "mim", "trunk", "heads"])
def test_imports_first_in_a_fresh_process(module):
    """no import-order dependence among the schedule's modules: each one comes up as the first mvlt_amd import of a process"""
    r = _child(f"import mvlt_amd.{module}")
    assert r.returncode == 0, r.stderr[-2000:]

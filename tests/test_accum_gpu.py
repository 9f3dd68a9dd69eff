"""GPU: several backward passes of the real model into one flat gradient buffer (docs/accumulation.md).  Every scenario of tests/accum_cases.py runs on
`small96_T20_ragged` (pvlt_small, 96 px, T = 20, B = 3, all heads) in both compute dtypes and on both MLM paths; the reference is the CPU oracle's own
gradients of the two batches, combined by `accum_cases.expected` -- never a GPU run.  `tiny256_pretrain_b64` (the size that selects partial-tile weight
gradients with deferred folds) runs the plain, in-flight and dead-pass scenarios against 1.5 x (or 1 x) its fixture's norms and samples.

Bars: the gradient bars of test_train_step_parity (fp32 path 2e-4, bf16 path 8e-2; fixture samples at 4 x), the bf16 ITM tensors whose batch sum cancels gated
as there.  Besides, every result is compared with the same combination of two FRESH single-pass GPU gradients at 2e-5 / 3e-2 (the bounds of
test_full_batch_gradients_equal_the_mean_of_its_chunks / test_full_batch_step_is_repeatable): an identity, not the reference -- it shows a lost part of a
contribution on the bf16 path, below the oracle bar."""
import gc

import numpy as np
import pytest
import torch

from oracle import filler
from oracle import pvlt_oracle as O
from tests import accum_cases as A
from tests.test_model_gpu import _losses_like_engine, build, oracle_train, sample

pytestmark = pytest.mark.gpu

PRIMARY, SECONDARY = "small96_T20_ragged", "tiny256_pretrain_b64"
GTOL = {torch.float32: 2e-4, torch.bfloat16: 8e-2}           # test_train_step_parity's gtol
IDENT = {torch.float32: 2e-5, torch.bfloat16: 3e-2}
ITM_CANCEL = ("itm_head.linear.bias", "itm_head.linear_bias", "itm_head_embed.1.bias")
SENTINEL = 12345.678
_CACHE = {}            # oracle gradients on the device, fresh single-pass GPU gradients: computed once per file


class _Case:
    """the model of a fixture case, its two batches and their injected masks"""

    def __init__(self, name, golden_dir, dtype, fused):
        from tests.golden.make_golden import make_masks
        self.name, self.dtype, self.fused = name, dtype, fused
        self.model, self.cfg, self.sd, batch, self.g, self.seed = build(name, golden_dir, dtype)
        self.B, self.T = batch["image"].shape[0], batch["input_ids"].shape[1]
        self.step_idx = 1 if self.cfg.loss_type["t2i"] else 0
        self.batches = {"a": batch}
        self.masks = {"a": make_masks(self.cfg, self.B, self.T, self.seed + self.step_idx)}
        if name == PRIMARY:
            self.batches["b"] = O.to_torch_batch(filler.make_batch(self.seed + 1, self.B, batch["image"].shape[-1], self.T))
            self.masks["b"] = make_masks(self.cfg, self.B, self.T, self.seed + 1 + self.step_idx)
        else:                                                   # the same batch and masks twice
            self.batches["b"], self.masks["b"] = self.batches["a"], self.masks["a"]
        self.dev = torch.device("cuda:0")
        self.model.train()
        self.S = self.model.store
        self.S.ensure(self.dev)
        self.names = [n for n, _ in self.S.fn_params]
        self.ids = torch.cat([self.batches[k]["input_ids"].reshape(-1) for k in ("a", "b")])
        self.groups = {n: A.row_groups(n, self.ids, self.T) for n in self.names}


class _Driver:
    """the steps of a script (tests/accum_cases.py) on the real model, with the checks of each scenario along the way"""

    def __init__(self, cx, scenario, extra, monkeypatch):
        from mvlt_amd import ops
        from mvlt_amd.params import ZeroPool
        self.cx, self.scenario, self.extra, self.mp = cx, scenario, extra, monkeypatch
        self.loss, self.resid, self.passes, self.tn_calls, self.aborted = {}, {}, 0, [], []
        self.frozen_clone, self.alias_checked = None, False
        cx.S.on_pass_aborted = lambda st: self.aborted.append(1)
        real_tn = ops.gemm_tn

        def spy(*a, **kw):
            self.tn_calls.append((self.passes, bool(kw.get("overwrite")), bool(kw.get("defer_fold"))))
            return real_tn(*a, **kw)

        monkeypatch.setattr(ops, "gemm_tn", spy)
        gc.collect()
        self.pool = ZeroPool.of(cx.dev)
        self.pending0 = self.pool.pending
        self.k_die = self._dry_run() if scenario == "died" else None

    # ---- steps
    def _forward(self, batch):
        cx = self.cx
        b = cx.batches[batch]
        cx.model.injected_masks = cx.masks[batch]
        img = b["masked_images"] if cx.step_idx == 1 else b["image"]
        return cx.model(img.to(cx.dev), b["input_ids"].to(cx.dev), mlm_labels=b["mlm_labels"].to(cx.dev) if cx.fused else None)

    def fwd(self, tag, batch):
        cx = self.cx
        out = self._forward(batch)
        self.loss[tag] = _losses_like_engine(out, cx.batches[batch], cx.dev)["total_loss"]
        if out.get("itm_logits") is not None:              # the signed per-pair residuals of the ITM loss (test_train_step_parity's cancellation gate)
            pr = out["itm_logits"].detach().float().reshape(cx.B, 2).softmax(-1).cpu().numpy().astype(np.float64)
            self.resid[batch] = pr[:, 0] - (cx.batches[batch]["itm_labels"].reshape(-1).numpy() == 0)

    def bwd(self, tag, factor):
        (factor * self.loss.pop(tag)).backward()
        self.passes += 1

    def zero(self):
        self.cx.model.zero_grad(set_to_none=False)

    def none(self, key):
        for n in A.subset(key, self.cx.names):
            self.cx.S.params[n].grad = None

    def foreign(self, key):
        for n in A.subset(key, self.cx.names):
            self.cx.S.params[n].grad = self.extra["r"][n].clone()

    def clip(self):
        self.cx.S.clip_grad_norm(self.extra["max_norm"])
        assert self.cx.S.pending_clip is not None

    def freeze(self, key):
        for n in A.subset(key, self.cx.names):
            self.cx.S.params[n].requires_grad_(False)

    def eval(self, batch):
        self.cx.model.eval()
        with torch.no_grad():
            self._forward(batch)
        self.cx.model.train()

    def drop(self, tag):
        del self.loss[tag]

    def _dry_run(self):
        """a counting pass: the number of ops.layernorm_bwd calls a backward has made when stage 4 of the trunk is through (the heads and the MIM decoder run
        before the trunk's node) -> the call at which `die` raises, the first one of stage 3"""
        from mvlt_amd import ops, trunk
        n, at = [0], {}
        real_ln, real_stage = ops.layernorm_bwd, trunk.TrunkStep._stage_backward

        def count(*a, **kw):
            n[0] += 1
            return real_ln(*a, **kw)

        def stage(step, i, *a, **kw):
            r = real_stage(step, i, *a, **kw)
            at[i] = n[0]
            return r

        with self.mp.context() as m:
            m.setattr(ops, "layernorm_bwd", count)
            m.setattr(trunk.TrunkStep, "_stage_backward", stage)
            self.fwd("dry", "a")
            self.bwd("dry", 1.0)
        self.none("all")
        assert at[3] >= 5 and n[0] > at[3] + 4, (at, n)          # the heads' five and stage 4's own came first, stages 3-1 follow
        return at[3] + 1

    def die(self, tag):
        from mvlt_amd import ops
        S = self.cx.S
        n, seen = [0], {}
        real_ln = ops.layernorm_bwd

        def dying(*a, **kw):
            n[0] += 1
            if n[0] == self.k_die:
                seen.update(ln_lo=S._ln_lo, tap_lo=S._tap_lo)
                raise RuntimeError("accumulation test: the pass dies here")         # a host exception before the launch
            return real_ln(*a, **kw)

        with self.mp.context() as m:
            m.setattr(ops, "layernorm_bwd", dying)
            with pytest.raises(RuntimeError, match="the pass dies here"):
                self.loss.pop(tag).backward()
        # the premise: the dead pass left both arenas dirty and its final callback never ran
        assert seen["ln_lo"] is not None and seen["tap_lo"] is not None, seen
        assert S._finalize_queued and S._ln_lo is not None and S._tap_lo is not None
        dead = [c for c in self.tn_calls if c[0] == self.passes]
        assert dead and any(c[2] for c in dead), "no weight-gradient launch of the dead pass deferred its fold"
        self.passes += 1
        gc.collect()                # (the raised exception's traceback holds the dead pass's frames in a cycle of Python's own)

    # ---- checks
    def _arenas_clean(self):
        S = self.cx.S
        assert S._ln_lo is None and S._tap_lo is None
        assert not bool(S._ln_arena.any()) and not bool(S._tap_arena.any())

    def _gap_bits(self):
        S = self.cx.S
        return torch.cat([S.G[lo:hi] for lo, hi in A.gaps(S.offsets)]).view(torch.int32).clone()

    def check(self, label):
        S, cx = self.cx.S, self.cx
        if label.startswith("pending"):
            assert self.pool.pending - self.pending0 == int(label[-1]), (label, self.pool.pending, self.pending0)
        elif label == "after_pass1":
            for n, p in S.fn_params:
                gv = S.grad(n)
                assert p.grad is not None and p.grad.data_ptr() == gv.data_ptr() and p.grad.untyped_storage().data_ptr() == S.G.untyped_storage().data_ptr(), n
            assert S.all_zeroed_this_pass
            for lo, hi in A.gaps(S.offsets):
                S.G[lo:hi] = SENTINEL
            self.gap_bits = self._gap_bits()
            assert self.gap_bits.numel() >= 8
        elif label == "after_pass2":
            assert torch.equal(self._gap_bits(), self.gap_bits)                     # no writer of pass 2 reached into an alignment gap
            self._arenas_clean()
        elif label == "sync":
            want = A.coefficients(self.scenario, cx.names, self.extra)
            self._check_alias(want)
            foreign = [n for n in cx.names if want[n][2]]
            keep = {n: S.params[n].grad.clone() for n in foreign}
            S.sync_grads()
            for n in cx.names:
                assert S.params[n].grad.data_ptr() == S.grad(n).data_ptr(), n
            for n in foreign:
                assert torch.equal(S.grad(n), keep[n]), n
        elif label == "nothing_pending":
            assert S.pending_clip is None and S.pending_gate is None and S.pending_grad_scale == 1.0 and not S.grad_works
        elif label == "clone_frozen":
            self.frozen_clone = {n: S.params[n].grad.clone() for n in A.subset("stages12", cx.names)}
            assert len(self.frozen_clone) > 20
        elif label == "after_dead":
            assert self.aborted == [1]
            self._arenas_clean()
            before = S.G.clone()
            S.tn_fold_flush()
            torch.cuda.synchronize()
            assert torch.equal(S.G.view(torch.int32), before.view(torch.int32))     # nothing of the dead pass was still owed to G
        else:
            raise KeyError(label)

    def _check_alias(self, want):
        S = self.cx.S
        for n in self.cx.names:
            p = S.params[n]
            assert p.grad is not None, n
            assert (p.grad.data_ptr() == S.grad(n).data_ptr()) == want[n][3], (n, "must alias" if want[n][3] else "must not alias")
        self.alias_checked = True

    def finish(self):
        """what holds after every script"""
        S, cx = self.cx.S, self.cx
        torch.cuda.synchronize()
        if not self.alias_checked:
            self._check_alias(A.coefficients(self.scenario, cx.names, self.extra))
        assert not self.loss and self.pool.pending == self.pending0
        assert not S._finalize_queued and len(self.aborted) == (1 if self.scenario == "died" else 0)
        self._arenas_clean()
        # the first-writer store of the decoder's weight gradient: once per pass that started from an all-zero buffer on the bf16 path, never in a pass that accumulates
        zeroed_passes = {"died": [0, 1, 2]}.get(self.scenario, [0])
        assert sorted(c[0] for c in self.tn_calls if c[1]) == (zeroed_passes if cx.dtype == torch.bfloat16 else []), [c for c in self.tn_calls if c[1]]
        if self.scenario not in ("died", "inflight_dropped"):
            assert self.passes == 2 and not S.all_zeroed_this_pass
        if self.frozen_clone is not None:
            for n, c in self.frozen_clone.items():
                assert torch.equal(S.params[n].grad.view(torch.int32), c.view(torch.int32)), n       # bit for bit what pass 1 left
        return {n: S.params[n].grad.detach() for n in cx.names}


# ------------------------------------------------------------------ references
def _oracle_grads(cx):
    """the CPU oracle's gradients of batch a and batch b (one oracle run per batch for the whole file, shared with tests/test_model_gpu.py), on the device"""
    key = ("oracle", cx.name)
    if key not in _CACHE:
        res = {}
        for k in ("a", "b"):
            _, og = oracle_train(cx.name if k == "a" else cx.name + "#b", cx.sd, cx.cfg, cx.batches[k], cx.step_idx, cx.masks[k])
            res[k] = {n: og[n].to(cx.dev) for n in cx.names if og.get(n) is not None}
        _CACHE[key] = res
    return _CACHE[key]


def _fresh_grads(cx, golden_dir):
    """single-pass GPU gradients of a and b from `.grad = None`, one pass each, on a model of their own"""
    key = ("fresh", cx.name, cx.dtype, cx.fused)
    if key not in _CACHE:
        fx = _Case(cx.name, golden_dir, cx.dtype, cx.fused)
        res = {}
        for k in ("a", "b") if cx.name == PRIMARY else ("a",):
            for p in fx.model.parameters():
                p.grad = None
            b = fx.batches[k]
            fx.model.injected_masks = fx.masks[k]
            img = b["masked_images"] if fx.step_idx == 1 else b["image"]
            out = fx.model(img.to(fx.dev), b["input_ids"].to(fx.dev), mlm_labels=b["mlm_labels"].to(fx.dev) if fx.fused else None)
            _losses_like_engine(out, b, fx.dev)["total_loss"].backward()
            torch.cuda.synchronize()
            res[k] = {n: fx.S.params[n].grad.detach().clone() for n in fx.names}
        res.setdefault("b", res["a"])
        _CACHE[key] = res
    return _CACHE[key]


def _norm(grads, names):
    return float(torch.sqrt(sum(grads[n].double().pow(2).sum() for n in names)))


def _cancel(cx, drv, coef, per_pair_ok):
    """the bf16 ITM tensors whose batch sum cancels, gated as test_train_step_parity gates them: c from the combined per-pair residuals of the passes in the sum.
    One Linear further back the factor is the fixture's, measured on the reference's per-pair gradients of batch a: it holds for a result that is a multiple of
    g_a alone (`per_pair_ok`); a sum with another batch is compared plainly there."""
    if cx.dtype != torch.bfloat16 or "a" not in drv.resid or "itm_head.linear.bias" not in cx.names:
        return {}
    ca, cb, adds_r, _ = coef["itm_head.linear.bias"]
    c = A.cancel_factor([(ca + (0.25 if adds_r else 0.0), drv.resid["a"]), (cb, drv.resid.get("b", drv.resid["a"]))])
    res = {k: c for k in ITM_CANCEL}
    ck = f"train{cx.step_idx}/cancel/itm_head_embed.0.bias"
    if per_pair_ok and ck in cx.g.files:
        res["itm_head_embed.0.bias"] = max(1.0, float(cx.g[ck]) / np.sqrt(cx.B))
    return res


def _extras(cx, og):
    """scenario inputs that come from the reference: the clip threshold (half the reference norm of g_a) and the foreign tensors r = 0.25 g_a"""
    norm_a = _norm(og["a"], list(og["a"]))
    max_norm = 0.5 * norm_a
    r = {n: (0.25 * og["a"][n]).float() if n in og["a"] else torch.zeros_like(cx.S.params[n]) for n in cx.names}
    return dict(max_norm=max_norm, c=max_norm / (norm_a + 1e-6), r=r)


# ------------------------------------------------------------------ primary case: the oracle's own gradients
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "logits"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("scenario", list(A.SCENARIOS))
def test_accumulation_against_the_oracle(golden_dir, parity, monkeypatch, scenario, dtype, fused):
    """every scenario on small96_T20_ragged: `.grad` of every parameter against the oracle's gradients of the two batches combined the way stock PyTorch
    combines them, and against the same combination of two fresh single-pass GPU gradients"""
    cx = _Case(PRIMARY, golden_dir, dtype, fused)
    og = _oracle_grads(cx)
    names = [n for n in cx.names if n in og["a"] and n in og["b"]]
    assert len(names) > 300 and A.WORD_TABLE in names
    extra = _extras(cx, og)
    drv = _Driver(cx, scenario, extra, monkeypatch)
    A.run_script(scenario, drv)
    got = drv.finish()
    coef = A.coefficients(scenario, cx.names, extra)
    only_a = all(cb == 0 and not r for _, cb, r, _ in coef.values())
    want = {n: v for n, (v, _) in A.expected(scenario, og["a"], og["b"], names, extra).items()}
    bad = A.compare(got, want, GTOL[dtype], cx.groups, _cancel(cx, drv, coef, only_a), parity, "accum-vs-oracle")
    fresh = _fresh_grads(cx, golden_dir)
    norm_f = _norm(fresh["a"], cx.names)
    extra_f = dict(extra, c=extra["max_norm"] / (norm_f + 1e-6))                   # the coefficient the fresh gradients themselves give
    want_f = {n: v for n, (v, _) in A.expected(scenario, fresh["a"], fresh["b"], cx.names, extra_f).items()}
    bad_f = A.compare(got, want_f, IDENT[dtype], cx.groups, None, parity, "accum-vs-fresh")
    top = lambda d: sorted(d.items(), key=lambda kv: -kv[1])[:10]
    assert not bad and not bad_f, (scenario, str(dtype), fused, "oracle", top(bad), "fresh", top(bad_f))


# ------------------------------------------------------------------ secondary case: the fixture's norms and samples
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "logits"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("scenario", ["plain", "inflight_ba", "inflight_ab", "inflight_dropped", "died"])
def test_accumulation_with_deferred_folds(golden_dir, parity, monkeypatch, scenario, dtype, fused):
    """tiny256_pretrain_b64 -- partial-tile weight gradients with deferred folds: the same batch and masks twice, loss factors 1 and 0.5, against 1.5 x the
    reference's gradient norms and strided samples of one step (1 x where the scenario ends with a single pass)"""
    cx = _Case(SECONDARY, golden_dir, dtype, fused)
    g, pre = cx.g, f"train{cx.step_idx}/grad/"
    drv = _Driver(cx, scenario, {}, monkeypatch)
    A.run_script(scenario, drv)
    got = drv.finish()
    assert any(c[2] for c in drv.tn_calls)                                          # the deferred folds were in play
    names = [n for n in cx.names if pre + n + "/norm" in g.files and float(g[pre + n + "/norm"]) >= 1e-7]
    assert len(names) > 50
    ref_n = {n: float(g[pre + n + "/norm"]) for n in names}
    ref_s = {n: np.asarray(g[pre + n + "/sample"], dtype=np.float64) for n in names}
    coef = A.coefficients(scenario, cx.names, {})
    want_n = A.expected(scenario, ref_n, ref_n, names)
    want_s = A.expected(scenario, ref_s, ref_s, names)
    cancel = _cancel(cx, drv, coef, True)                                           # (the same batch twice: the per-pair gradients of the sum are multiples of batch a's)
    gtol = GTOL[dtype]
    bad = {}
    for n in names:
        refn, refs, c_k = want_n[n][0], want_s[n][0], cancel.get(n, 1.0)
        gn = got[n].double().norm().item()
        es = float(np.abs(sample(got[n], 32) - refs).max() / max(np.abs(refs).max(), 1e-3 * refn / max(1.0, got[n].numel() ** 0.5))) / c_k
        ok_n = parity("accum-grad-norm/" + n, abs(gn - refn) / (refn * c_k), gtol)
        ok_s = parity("accum-grad-sample/" + n, es, 4 * gtol)
        if not (ok_n and ok_s):
            bad[n] = (gn, refn, es)
    fresh = _fresh_grads(cx, golden_dir)
    want_f = {n: v for n, (v, _) in A.expected(scenario, fresh["a"], fresh["b"], cx.names).items()}
    bad_f = A.compare(got, want_f, IDENT[dtype], cx.groups, None, parity, "accum-vs-fresh")
    assert not bad and not bad_f, (scenario, str(dtype), fused, sorted(bad.items())[:10], sorted(bad_f.items(), key=lambda kv: -kv[1])[:10])


# ------------------------------------------------------------------ refused loudly: a second backward over a retained graph
def test_second_backward_over_a_retained_graph_is_refused(golden_dir):
    """a node gives up its saved step when its backward has run; a second backward() over the same (retained) graph cannot be computed and must say so instead
    of leaving a partial sum"""
    cx = _Case(PRIMARY, golden_dir, torch.float32, True)
    b = cx.batches["a"]
    cx.model.injected_masks = cx.masks["a"]
    out = cx.model(b["masked_images"].to(cx.dev), b["input_ids"].to(cx.dev), mlm_labels=b["mlm_labels"].to(cx.dev))
    loss = _losses_like_engine(out, b, cx.dev)["total_loss"]
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()

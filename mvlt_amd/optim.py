"""Fused AdamW over the model's flat fp32 parameter / gradient buffers (one HIP kernel per step, plus the bf16
re-cast of the updated weights in the same pass).

Semantics = torch.optim.AdamW as the reference builds it through timm.optim.create_optimizer (main_vl.py:308):
decoupled weight decay, bias-corrected moments, eps 1e-8, and timm's param-group split -- 1-D tensors and `.bias`
get weight_decay 0, everything else args.weight_decay.  It is a torch.optim.Optimizer, so GradScaler.step(),
lr schedulers (`param_groups[i]['lr']`) and state_dict()/load_state_dict() keep working; `param_groups[0]` is the
no-decay group and `[1]` the decay group, like timm's add_weight_decay.

param_groups=[...] (docs/param_groups.md): the caller's own groups, each with its `lr` and `weight_decay` -- a head that trains faster than the backbone, or
layer-wise lr decay (`layer_decay_groups` below).  While every group has the same lr and at most one non-zero weight decay the step is the launch above;
otherwise it is one launch of mvlt_adamw_step_groups (include/mvlt_hip_opt.h), which looks both up per element.  betas and eps are one for all groups.

Frozen parameters (requires_grad=False) are left alone, as torch.optim.AdamW leaves a parameter without `.grad` alone: the groups hold every
parameter of the model, and the per-element mask of the kernel carries a third value for the elements of frozen ones (neither they nor their
moments nor their bf16 copies are written).  The mask follows requires_grad from step to step, so un-freezing needs no new optimizer.

FusedLamb (docs/lamb.md): the same store, groups, masks, ring and checkpoints, stepped with LAMB -- AdamW's moments, then every tensor's update scaled by its
own trust ratio ||p|| / ||update|| -- in three launches (include/mvlt_hip_lamb.h).

skip_nonfinite=True (docs/nonfinite_guard.md): with engine.BF16Scaler(skip_nonfinite=True) in front, a step whose gradients hold Inf / NaN changes nothing
-- the decision is taken on the device (FlatStore.gate_grads) and obeyed by the kernel, the host never reads it.  One difference from GradScaler follows:
`_step`, the host count behind the bias corrections, counts ATTEMPTED steps, so after a skip the corrections are those of t + 1.
"""
import re

import torch

from . import ops
from .params import ALIGN


def _unwrap(model):
    return model.module if hasattr(model, "module") and not hasattr(model, "store") else model


def phased_ranges(S):
    """The element ranges of the flat buffers in the order the optimizer may step them.  Without gradient collectives in flight: the whole buffer.
    With them (mvlt_amd.dist.DataParallel hands them over un-waited when this optimizer is the next reader): first the ranges whose collectives were
    issued DURING the backward pass -- by now (mostly) complete -- then the ones issued at its end, each group after `wait()` on its works (a
    stream-side wait for RCCL: the host keeps enqueuing).  The first launch then runs while the tail is still on the wire; element-wise AdamW makes the
    result bit-identical to one launch over everything.  Anything the collectives do not cover exactly once falls back to wait-all + one range.
    With a clip or a step gate pending (FlatStore.clip_grad_norm / gate_grads ran: the global norm needs every gradient) the collectives are already
    waited and this yields the single whole range."""
    works, S.grad_works = S.grad_works, []
    if not works:
        yield 0, S.total
        return
    def finish(ws):
        for w, lo, hi, g, t, early in ws:
            w.wait()
            if t is not None:
                g.copy_(t)
    cov = sorted((lo, hi) for _, lo, hi, _, _, _ in works)
    exact = cov[0][0] == 0 and cov[-1][1] == S.total and all(a[1] == b[0] for a, b in zip(cov, cov[1:]))
    groups = [[x for x in works if x[5]], [x for x in works if not x[5]]]
    if not exact or not groups[0] or not groups[1]:
        finish(works)
        yield 0, S.total
        return
    for ws in groups:
        finish(ws)
        merged = []
        for lo, hi in sorted((x[1], x[2]) for x in ws):
            if merged and merged[-1][1] == lo:
                merged[-1][1] = hi
            else:
                merged.append([lo, hi])
        for lo, hi in merged:
            yield lo, hi


def clip_grad_norm_(model, max_norm):
    """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) for loops that do not go through engine.BF16Scaler: the global norm in one pass
    over the flat gradient buffer (FlatStore.clip_grad_norm), then settled at once -- G is scaled in place by the coefficient and by an owed 1/world,
    so `.grad`, logging and any optimizer see final, clipped gradients.  `model`: the model, a DataParallel / DDP wrapper around it, or its store.
    Returns the total norm as a 0-dim device tensor (no host read)."""
    S = model if hasattr(model, "clip_grad_norm") else _unwrap(model).store
    norm = S.clip_grad_norm(max_norm).clone()           # (the store's own scalar is overwritten by the next clipping)
    S.apply_pending_scale()
    return norm


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, skip_nonfinite=False, param_groups=None):
        model = _unwrap(model)
        self.model = model
        self.skip_nonfinite = bool(skip_nonfinite)
        self._pending_counts = None           # (applied, skipped) of a checkpoint loaded before the flat store exists
        # every parameter of the model is in a group, frozen ones too: `requires_grad` decides per step (the mask byte of mvlt_adamw_step), so a
        # parameter frozen now and un-frozen later starts stepping without a new optimizer
        if param_groups is None:
            no_decay, decay = [], []
            for name, p in model.named_parameters():
                (no_decay if (p.dim() == 1 or name.endswith(".bias")) else decay).append(p)
            groups = [dict(params=no_decay, weight_decay=0.0), dict(params=decay, weight_decay=weight_decay)]
        else:
            groups = self._checked_groups(model, param_groups, tuple(betas), eps)
        super().__init__(groups, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._step = 0
        self._m = self._v = self._wd_mask = self._group_of = self._mask_key = None
        self._frozen_ranges = []              # maximal [lo, hi) runs of the flat buffer whose every element is frozen (gaps inside a run included)
        self._hp = self._hp_pin = None
        self._hp_ev = [None] * 4
        self._pending = None                  # (m, v) of a checkpoint loaded before the flat store exists

    @staticmethod
    def _checked_groups(model, param_groups, betas, eps):
        """the caller's groups as torch.optim.Optimizer takes them (`params` a list; every other key -- lr, weight_decay, name, lr_scale, ... -- as it
        came), or a ValueError that names the offender"""
        groups = [dict(g, params=list(g["params"])) if isinstance(g, dict) and "params" in g else g for g in param_groups]
        if not groups or not all(isinstance(g, dict) and "params" in g for g in groups):
            raise ValueError("FusedAdamW: param_groups must be a non-empty list of dicts with a 'params' entry")
        if len(groups) > ops.OPT_MAX_GROUPS:
            raise ValueError(f"FusedAdamW: {len(groups)} parameter groups, the kernel's group byte takes {ops.OPT_MAX_GROUPS} at the most")
        label = lambda i: f"group {i}" + (f" ({groups[i]['name']!r})" if "name" in groups[i] else "")
        names = {id(p): n for n, p in model.named_parameters()}
        where = {}
        for i, g in enumerate(groups):
            if tuple(g.get("betas", betas)) != betas or g.get("eps", eps) != eps:
                raise ValueError(f"FusedAdamW: {label(i)} has betas {g.get('betas', betas)} / eps {g.get('eps', eps)}, the optimizer {betas} / {eps}: "
                                 "one betas and one eps for all groups (lr and weight_decay may differ)")
            for p in g["params"]:
                if id(p) not in names:
                    raise ValueError(f"FusedAdamW: {label(i)} holds a tensor of shape {tuple(p.shape)} that is not a parameter of the model")
                if id(p) in where:
                    raise ValueError(f"FusedAdamW: parameter {names[id(p)]!r} is in two groups, {label(where[id(p)])} and {label(i)}")
                where[id(p)] = i
        missing = [n for k, n in names.items() if k not in where]
        if missing:
            raise ValueError(f"FusedAdamW: parameter {missing[0]!r} is in no group ({len(missing)} in all; frozen parameters are listed too: "
                             "requires_grad decides per step)")
        return groups

    def _ensure(self):
        S = self.model.store
        if S.P is None:
            raise RuntimeError("FusedAdamW: run a forward first (the flat parameter store is built lazily)")
        if self._m is None or self._m.numel() != S.total or self._m.device != S.P.device:
            self._m = torch.zeros_like(S.P)
            self._v = torch.zeros_like(S.P)
            if self._pending is not None:        # moments of a checkpoint that was loaded before the first forward
                pm, pv = self._pending
                if pm.numel() != S.total:
                    raise RuntimeError(f"FusedAdamW: checkpoint moments have {pm.numel()} elements, the model's flat store {S.total}")
                self._m.copy_(pm)
                self._v.copy_(pv)
                self._pending = None
            self._hp = None
        width = 8 + 2 * len(self.param_groups)   # the hp row of mvlt_adamw_step, then {lr, weight_decay} of every group: the table of mvlt_adamw_step_groups
        if self._hp is None or self._hp.numel() != width:          # (the second: add_param_group)
            self._hp = torch.zeros(width, device=S.P.device)
            # the step's scalars reach the device through a ring of PINNED rows: from a pageable source hipMemcpyAsync stages the copy on
            # the host and the call returns only when the stream has drained -- the host then enqueues the optimizer kernel and the whole
            # next forward behind an idle GPU (1.3 ms per fine-tune step, tools/host_time.py).  An event per row guards its reuse.
            self._hp_pin = torch.zeros(4, width).pin_memory() if S.P.is_cuda else None
            self._hp_ev = [None] * 4
        if self._pending_counts is not None:     # step counters of a checkpoint that was loaded before the first forward
            S._gate_buffers()[1].copy_(torch.tensor(self._pending_counts, dtype=torch.int32))
            self._pending_counts = None
        key = (S.P.data_ptr(), tuple(p.requires_grad for p in S._plist), tuple(g["weight_decay"] != 0 for g in self.param_groups))
        if self._mask_key != key:                # the store was re-materialised, or a parameter was frozen / un-frozen (as FlatStore's norm mask)
            # one byte per element: 1 = weight decay applies (the parameter's group has a non-zero one; timm's split: not for 1-D tensors / biases), 0 = it
            # does not (alignment gaps too), 2 = the parameter is frozen: the kernel leaves it, its moments and its bf16 copy alone
            # ... and next to it the byte mvlt_adamw_step_groups reads: the index of the parameter's group, 255 for frozen parameters and alignment gaps
            group_ix = {id(p): i for i, g in enumerate(self.param_groups) for p in g["params"]}
            ids_nd = {k for k, i in group_ix.items() if not key[2][i]}
            lost = [name for name, p in S.params.items() if id(p) not in group_ix]
            if lost:       # a Parameter (or the module holding it) was replaced after this optimizer was built: the store re-materialised around the new one
                raise RuntimeError(f"{type(self).__name__}: parameter {lost[0]!r} of the model is in no parameter group ({len(lost)} in all) -- it was replaced "
                                   "after the optimizer was built; build a new optimizer (or add_param_group the new parameters)")
            mask = torch.zeros(S.total, dtype=torch.uint8)
            group_of = torch.full((S.total,), ops.OPT_FROZEN, dtype=torch.uint8)
            runs = []
            for name, p in S.params.items():
                off, n, _ = S.offsets[name]
                if p.requires_grad:
                    group_of[off:off + n] = group_ix[id(p)]
                if not p.requires_grad:
                    mask[off:off + n] = ops.ADAMW_FROZEN
                    hi = off + (n + ALIGN - 1) // ALIGN * ALIGN
                    if runs and runs[-1][1] == off:
                        runs[-1][1] = hi
                    else:
                        runs.append([off, hi])
                elif id(p) not in ids_nd:
                    mask[off:off + n] = 1
            self._wd_mask = mask.to(S.P.device)
            self._group_of = group_of.to(S.P.device)
            self._frozen_ranges = [(lo, hi) for lo, hi in runs]
            self._mask_key = key
        return S

    def _all_frozen(self, lo, hi):
        return any(a <= lo and hi <= b for a, b in self._frozen_ranges)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        S = self._ensure()
        S.sync_grads()
        self._step += 1
        groups = self.param_groups
        g0 = groups[0]
        b1, b2 = g0["betas"]
        # One learning rate and at most one non-zero weight decay (the default two groups under timm's scheduler, or the caller's groups when they agree):
        # mvlt_adamw_step with the decay mask.  Anything else: mvlt_adamw_step_groups, which looks both up per element.
        decays = {g["weight_decay"] for g in groups if g["weight_decay"] != 0}
        uniform = len(decays) <= 1 and all(g["lr"] == g0["lr"] for g in groups)
        wd = decays.pop() if uniform and decays else 0.0
        gscale, S.pending_grad_scale = S.pending_grad_scale, 1.0      # 1/world of the data-parallel mean, applied in the kernel
        clip, S.pending_clip = S.pending_clip, None                   # clip coefficient (device scalar) of FlatStore.clip_grad_norm: one more factor in the kernel
        gate, S.pending_gate = S.pending_gate, None                   # [norm, coef, ok, 0] of FlatStore.gate_grads: the gated kernel obeys ok and applies coef
        if gate is not None and clip is not None:
            raise RuntimeError("FusedAdamW: both a clip and a step gate are pending (FlatStore.gate_grads(max_norm) does the clipping itself)")
        row = [g0["lr"], b1, b2, g0["eps"], wd, 1 - b1 ** self._step, 1 - b2 ** self._step, gscale]
        for g in groups:                         # the table rides behind the row: one copy through the ring for both
            row += (g["lr"], g["weight_decay"])
        if self._hp_pin is None:
            self._hp.copy_(torch.tensor(row, dtype=torch.float32))
        else:
            k = self._step % 4
            if self._hp_ev[k] is not None:
                self._hp_ev[k].synchronize()              # the copy that last used this row has run (four steps ago: a no-op wait)
            self._hp_pin[k].copy_(torch.tensor(row, dtype=torch.float32))
            self._hp.copy_(self._hp_pin[k], non_blocking=True)
            ev = self._hp_ev[k] = self._hp_ev[k] or torch.cuda.Event()
            ev.record()
        c_current = S.c_is_current()             # before the launch: was the bf16 copy current for the parameters this step starts from?
        self._launch(S, uniform, clip, gate)
        # W^T / permuted conv operand copies are refreshed by the next forward.  The plain bf16 copy S.C is declared current only when the launches
        # left it so: frozen elements and a closed step gate keep the copy they had, which is the parameters' only if nothing wrote them since the last
        # forward (FlatStore.c_written_by_kernel).  Afterwards it holds as long as nothing else writes the parameters (FlatStore.versions() notices)
        S.c_written_by_kernel(c_current, wrote_all=gate is None and all(self._mask_key[1]))
        return loss

    def _launch(self, S, uniform, clip, gate):
        """the launches of one step, behind the hyper-parameter row that is already on its way to the device (FusedLamb replaces this part alone)"""
        groups = self.param_groups
        for lo, hi in phased_ranges(S):
            if self._all_frozen(lo, hi):         # nothing in the range steps: no launch
                continue
            if not uniform:                      # (a pending gate: gate_grads waited for every collective, this is the single whole range)
                ops.adamw_step_groups(S.P[lo:hi], S.G[lo:hi], self._m[lo:hi], self._v[lo:hi], None if S.C is None else S.C[lo:hi], hi - lo, self._hp,
                                      self._group_of[lo:hi], self._hp[8:], len(groups), gscale_dev=clip, gate=gate)
                continue
            if gate is not None:                 # (gate_grads waited for every collective: this is the single whole range)
                ops.adamw_step_gated(S.P[lo:hi], S.G[lo:hi], self._m[lo:hi], self._v[lo:hi], None if S.C is None else S.C[lo:hi], hi - lo, self._hp,
                                     self._wd_mask[lo:hi], gate)
                continue
            ops.adamw_step(S.P[lo:hi], S.G[lo:hi], self._m[lo:hi], self._v[lo:hi], None if S.C is None else S.C[lo:hi], hi - lo, self._hp, self._wd_mask[lo:hi],
                           gscale_dev=clip)

    def zero_grad(self, set_to_none=True):
        super().zero_grad(set_to_none=set_to_none)

    def _counts(self):
        """(applied, skipped): the device counters of FlatStore.gate_grads (one read-back), or what a checkpoint left while there is no store yet"""
        if self._pending_counts is not None:
            return self._pending_counts
        S = self.model.store
        if getattr(S, "_gate", None) is None:
            return (0, 0)
        a, k = S._gate[1].tolist()
        return (a, k)

    @property
    def applied_steps(self):
        """guarded steps that were applied (finite gradient norm).  Reads the device: for logging, not for the step path"""
        return self._counts()[0]

    @property
    def skipped_steps(self):
        """guarded steps the device skipped (Inf / NaN in a trainable gradient).  Reads the device: for logging, not for the step path"""
        return self._counts()[1]

    def state_dict(self):
        sd = super().state_dict()
        m, v = (self._m, self._v) if self._m is not None else (self._pending or (None, None))
        sd["fused"] = dict(step=self._step, m=None if m is None else m.cpu(), v=None if v is None else v.cpu())
        if self.skip_nonfinite:
            sd["fused"]["applied"], sd["fused"]["skipped"] = self._counts()
        return sd

    def load_state_dict(self, sd):
        """Works before the first forward too (the reference resumes in that order: main_vl.py:308 builds the optimizer,
        :340 loads its state, the first forward comes later): the moments then wait in `_pending` until `_ensure`."""
        sd = dict(sd)                                  # the caller's checkpoint dict stays as it was
        fused = sd.pop("fused", None)
        super().load_state_dict(sd)
        if fused is not None:
            self._step = fused["step"]
            if "applied" in fused or "skipped" in fused:       # checkpoints of a guarded run carry the counters; others leave them as they are
                counts = (int(fused.get("applied", 0)), int(fused.get("skipped", 0)))
                if self.model.store.P is not None:
                    self._pending_counts = None
                    self.model.store._gate_buffers()[1].copy_(torch.tensor(counts, dtype=torch.int32))
                else:
                    self._pending_counts = counts
            if fused["m"] is not None:
                if self.model.store.P is not None:
                    self._pending = None
                    self._ensure()
                    self._m.copy_(fused["m"])
                    self._v.copy_(fused["v"])
                else:
                    self._m = self._v = None
                    self._pending = (fused["m"].detach().clone(), fused["v"].detach().clone())


LAMB_MAX_CHUNKS = 64 * 256        # chunks of one tensor (268 M elements): 64 sequential additions per lane of the fold, which keeps the reduction depth at 99 (docs/lamb.md)


def lamb_tables(layout, n, n_groups):
    """The two tables that describe a flat buffer of n elements to the LAMB launches (include/mvlt_hip_lamb.h), as HOST tensors.
    layout: [(offset, length, group, frozen)] per tensor, ascending.  Returns (tensors int64 [T, ops.LAMB_ROW] = {offset, length, group, frozen,
    first_chunk, n_chunks}, chunks int32 [C, 2] = {tensor, index of the chunk in it}): a tensor is cut into ops.LAMB_CHUNK-element chunks counted from ITS
    first element, so how a tensor is summed does not depend on where it stands or on what stands next to it; a short tensor is one short chunk, an
    empty one none.  Checked by mvlt_lamb_check_tables before they are returned."""
    rows, first = [], 0
    for off, length, group, frozen in layout:
        cnt = (length + ops.LAMB_CHUNK - 1) // ops.LAMB_CHUNK
        if cnt > LAMB_MAX_CHUNKS:
            raise ValueError(f"FusedLamb: a tensor of {length} elements is {cnt} chunks, more than the {LAMB_MAX_CHUNKS} the fold's error bound is stated for")
        rows.append([off, length, group, 1 if frozen else 0, first, cnt])
        first += cnt
    tensors = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), ops.LAMB_ROW)
    counts = tensors[:, 5]
    owner = torch.repeat_interleave(torch.arange(len(rows)), counts)
    index = torch.arange(first) - tensors[owner, 4]
    chunks = torch.stack([owner, index], 1).to(torch.int32).contiguous()
    ops.lamb_check_tables(tensors, chunks, n, n_groups)
    return tensors, chunks


class FusedLamb(FusedAdamW):
    """LAMB over the flat store (docs/lamb.md) -- what the reference's `--opt fusedlamb` asks apex for through timm.optim.create_optimizer (main_vl.py:308),
    for the large-batch regime its linear lr scaling leads to.  AdamW's moments, then every tensor's update is scaled by its own trust ratio:

        g = G * gs;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  u = (m / bc1) / (sqrt(v / bc2) + eps) + wd p
        r = ||p|| / ||u||  if (wd != 0 or always_adapt) and ||p|| > 0 and ||u|| > 0 else 1;  trust_clip: r = min(r, 1);  p = p - lr r u

    with lr / wd of the tensor's group and both norms over the tensor's own elements.  Three launches per step (moments + partial norms per chunk, one fold
    per tensor, apply + bf16 copy), no atomics and no host read: two runs from the same state give the same bits.  eps defaults to apex's 1e-6.  apex's own
    max_grad_norm is not re-implemented: clipping is BF16Scaler(...)(loss, opt, clip_grad=...), whose coefficient rides in gs as it does for FusedAdamW.

    Everything else is FusedAdamW's: param_groups / layer_decay_groups, frozen parameters (left alone, their NaNs reach no neighbour's norm), skip_nonfinite
    (all three launches obey the gate), the pinned hyper-parameter ring, state_dict / load_state_dict, FusedModelEma behind it.  One difference: a trust
    ratio needs the whole tensor, so `step` WAITS for every gradient collective the data-parallel wrapper handed over and steps the single whole range --
    the overlap of the first AdamW launch with the tail of the all-reduce (`phased_ranges`) is given up.

    `trust_ratios()`: {parameter name: 0-dim device view} of the ratios the last applied step used (1 before the first step, and for frozen tensors what
    they last trained with); reading a value is a host read, for logging only."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False, trust_clip=False, skip_nonfinite=False,
                 param_groups=None):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, skip_nonfinite=skip_nonfinite, param_groups=param_groups)
        self.always_adapt, self.trust_clip = bool(always_adapt), bool(trust_clip)
        self._lamb_key = self._tensors = self._chunks = self._partials = self._ratios = None
        self._n_chunks = 0
        self._any_live = False

    def _ensure(self):
        S = super()._ensure()
        key = (S.P.data_ptr(), tuple(p.requires_grad for p in S._plist), len(self.param_groups))
        if self._lamb_key != key:                # the store was re-materialised, or a parameter was frozen / un-frozen (as the group byte above)
            group_ix = {id(p): i for i, g in enumerate(self.param_groups) for p in g["params"]}
            layout = [(S.offsets[name][0], S.offsets[name][1], group_ix[id(p)], not p.requires_grad) for name, p in S.params.items()]
            tensors, chunks = lamb_tables(layout, S.total, len(self.param_groups))
            dev = S.P.device
            same = self._ratios is not None and self._ratios.device == dev and self._ratios.numel() == len(layout)
            self._tensors, self._chunks, self._n_chunks = tensors.to(dev), chunks.to(dev), chunks.shape[0]
            self._partials = torch.zeros(max(self._n_chunks, 1), 2, device=dev)
            if not same:
                self._ratios = torch.ones(len(layout), device=dev)
            self._any_live = any(not fz and n > 0 for _, n, _, fz in layout)
            self._lamb_key = key
        return S

    def _launch(self, S, uniform, clip, gate):
        S.wait_grads()                           # every collective: a trust ratio is a norm over whole tensors (no phased ranges)
        if not self._any_live:                   # nothing steps: no launch
            return
        k = len(self.param_groups)
        table = self._hp[8:]
        flags = (ops.LAMB_ALWAYS_ADAPT if self.always_adapt else 0) | (ops.LAMB_TRUST_CLIP if self.trust_clip else 0)
        ops.lamb_moments(S.P, S.G, self._m, self._v, S.total, self._hp, self._tensors, self._chunks, table, k, self._partials, gscale_dev=clip, gate=gate)
        ops.lamb_fold(self._partials, self._tensors, self._n_chunks, table, k, flags, self._ratios, gate=gate)
        ops.lamb_apply(S.P, self._m, self._v, S.C, S.total, self._hp, self._tensors, self._chunks, table, k, self._ratios, gate=gate)

    def trust_ratios(self):
        """{parameter name: 0-dim view of its trust ratio on the device}, in the store's order; empty before the first step"""
        if self._ratios is None:
            return {}
        return {name: self._ratios[i] for i, name in enumerate(self.model.store.params)}


_STAGE_NAME = re.compile(r"([A-Za-z_]+?)_?(\d+)")


def layer_ids(model):
    """{parameter name: layer id} for layer-wise lr decay down the pyramid -- a function of the parameter names and `model.depths` alone.  With
    L = sum(depths):
        0           the BERT embedding block (text_embeddings.*) and what stage 1 has in front of its blocks: patch_embed1, text_embed1, pos_embed1, text_pos_embed1
        1 .. L      the blocks in forward order: block{s}.{j} has 1 + depths[0] + ... + depths[s - 2] + j
        later stages' patch / text embeddings, position embeddings and any other tensor named <something>{s}: the id of block{s}.0, the first block they feed
        norm{s}     a stage's closing norm: the id of the stage's last block
        L + 1       every head (a top-level name with `head` in it: mlm_head*, itm_head*, sup_cls_head*, sub_cls_head*, t2i_head -- the MIM decoder)
    A name that fits none of these raises ValueError: a new part of the model gets a deliberate id, not the heads' learning rate by default."""
    m = _unwrap(model)
    depths = tuple(m.depths)
    first = [1 + sum(depths[:s]) for s in range(len(depths))]           # id of block{s + 1}.0
    ids = {}
    for name, _ in m.named_parameters():
        top, _, rest = name.partition(".")
        st = _STAGE_NAME.fullmatch(top)
        stage = int(st.group(2)) if st else 0
        if top == "text_embeddings":
            ids[name] = 0
        elif "head" in top:
            ids[name] = sum(depths) + 1
        elif st is None or not 1 <= stage <= len(depths):
            raise ValueError(f"layer_ids: no layer id for parameter {name!r} (not an embedding, a stage-numbered tensor, a block or a head)")
        elif st.group(1) == "block":
            j = int(rest.partition(".")[0])
            if not 0 <= j < depths[stage - 1]:
                raise ValueError(f"layer_ids: {name!r} names block {j} of stage {stage}, which has {depths[stage - 1]}")
            ids[name] = first[stage - 1] + j
        elif st.group(1) == "norm":
            ids[name] = first[stage - 1] + depths[stage - 1] - 1
        else:
            ids[name] = 0 if stage == 1 else first[stage - 1]
    return ids


def layer_decay_groups(model, lr, weight_decay, layer_decay):
    """Parameter groups for FusedAdamW(model, param_groups=...) (or any torch optimizer) with layer-wise lr decay: the group of layer id i (`layer_ids`) gets
    lr * layer_decay ** (L + 1 - i), so the heads train at `lr` and the embeddings at lr * layer_decay ** (L + 1).  Every layer is split by timm's no-decay
    rule (1-D tensors and `.bias`: weight_decay 0), empty halves are left out: at most 2 * (L + 2) groups, ordered by layer id, no-decay half first.  Each
    group carries `name` ("layer_<i>_decay" / "layer_<i>_no_decay") and `lr_scale` for logging; frozen parameters are listed like the others.  A scheduler that
    scales each group from its own base lr (sched.CosineLRScheduler) keeps the ratios."""
    m = _unwrap(model)
    ids = layer_ids(m)
    top = sum(m.depths) + 1
    split = {}
    for name, p in m.named_parameters():
        no_decay = p.dim() == 1 or name.endswith(".bias")
        split.setdefault((ids[name], 0 if no_decay else 1), []).append(p)
    groups = []
    for (i, dec), params in sorted(split.items(), key=lambda kv: kv[0]):
        scale = layer_decay ** (top - i)
        groups.append(dict(params=params, lr=lr * scale, weight_decay=weight_decay if dec else 0.0, lr_scale=scale,
                           name=f"layer_{i}_{'decay' if dec else 'no_decay'}"))
    return groups


class FusedModelEma:
    """Exponential moving average of a model's weights, kept by one HIP launch per step over the two flat parameter stores (docs/ema.md).  It stands where
    timm.utils.ModelEma would (reference main_vl.py:16,295; engine_grid_masking.py:130-131 calls `model_ema.update(model)` after every optimizer step):

        model_ema = FusedModelEma(model, decay=0.9999)
        train_one_epoch_vl(model, ..., model_ema=model_ema)          # engine.py calls model_ema.update(model)
        evaluate_vl(loader, model_ema.ema, device)                   # the averaged model is a model like any other
        torch.save({"model_ema": model_ema.state_dict()}, path)      # what get_state_dict(model_ema) would store (main_vl.py:452)

    `.ema` (alias `.module`, as in timm's ModelEmaV2) is a second model of the same class in eval mode, with a flat store of its own and parameters that take no
    gradient.  `model`: the model or a data-parallel wrapper around it.  `update(model)` computes, for every parameter element and every floating buffer,
    ema = ema * decay + model * (1 - decay) -- the two products and the sum each rounded to fp32, the bits of timm's per-tensor loop -- and writes the bf16
    copy the averaged model computes with in the same pass.  `decay` is a plain attribute (change it between steps); `updates` counts the calls; with
    warmup=True update number t = 1, 2, ... uses min(decay, (1 + t) / (10 + t)).

    Two differences from timm.  (1) Integer buffers -- BatchNorm's num_batches_tracked -- are COPIED from the model: timm's formula, applied to an int64 tensor,
    truncates the average back to an integer and leaves the counter one behind for ever.  (2) The elements of parameters the model holds frozen
    (requires_grad=False at the time of the update, as FusedAdamW reads it) are left alone: they keep the value they were copied with, which is the model's.
    timm averages them too, which moves e * decay + e * (1 - decay) away from e by a rounding now and then.

    The update always happens: after a step the non-finite guard skipped (FusedAdamW(skip_nonfinite=True)) the average still moves towards the unchanged
    parameters, as timm's does behind a GradScaler that skipped -- the engine calls update() unconditionally.

    The source's store is built lazily, so the averaged model's is too: at the first update() on the source's device, or by the averaged model's own first
    forward.  Until then its parameters are ordinary tensors, which is where load_state_dict() before the first forward puts a checkpoint -- nothing is kept
    aside, and the store picks the values up when it is built.  There is no CPU path: update() on host tensors raises MVLTError."""

    def __init__(self, model, decay=0.9999, warmup=False):
        import copy
        src = _unwrap(model)
        S = src.store
        # a deep copy of the module tree (names, shapes, order, values, buffers, tied weights) WITHOUT the source's store -- its flat buffers, gradient buffer,
        # scratch and data-parallel hooks are not the copy's business -- and without what the schedule caches on the model between passes
        memo = {id(S): None}
        for k in ("_plan", "_pool_token", "_mim_fold"):
            if src.__dict__.get(k) is not None:
                memo[id(src.__dict__[k])] = None
        self.ema = copy.deepcopy(src, memo)
        self.ema.__dict__.pop("_mim_fold", None)      # (copied as None when the source had one: MimStep._folded wants a dict of the copy's own, or nothing)
        slots = [k for k, v in vars(src).items() if v is S]
        if not slots:
            raise RuntimeError("FusedModelEma: the model does not hold its FlatStore as an attribute")
        from .params import FlatStore
        for k in slots:
            setattr(self.ema, k, FlatStore(self.ema, S.compute_dtype))
        self.ema.eval()
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self.decay = float(decay)
        self.warmup = bool(warmup)
        self.updates = 0
        self._layout_key = self._mask_key = self._buf_key = None
        self._mask = self._buf_table = None
        self._buf_slots, self._buf_n = [], 0

    @property
    def module(self):
        return self.ema

    def decay_at(self, t):
        """the decay of update number t (counted from 1)"""
        return min(self.decay, (1 + t) / (10 + t)) if self.warmup else self.decay

    def _ensure(self, src):
        S = src.store
        if S.P is None:
            raise RuntimeError("FusedModelEma: run a forward of the model first (its flat parameter store is built lazily)")
        E, dev = self.ema.store, S.P.device
        if E.P is None or E.device != dev or not E.is_current():
            if any(t.device != dev for t in self.ema.parameters()) or any(t.device != dev for t in self.ema.buffers()):
                self.ema.to(dev)
            E.ensure(dev)
        key = (S.P.data_ptr(), E.P.data_ptr())
        if self._layout_key != key:
            if list(S.offsets.items()) != list(E.offsets.items()) or S.total != E.total:
                raise RuntimeError("FusedModelEma: the model's flat store and the averaged model's are laid out differently (not the model this average was built from?)")
            # the two module trees are walked HERE, not per update (0.2 ms of host time for pvlt_tiny), for the SLOTS that hold their buffers -- (the module's
            # `_buffers` dict, name) -- so that each update reads the tensor a slot holds now: a buffer re-registered as a new tensor, or one whose storage moved,
            # changes the key below.  Whatever replaces every tensor of a module (.to(), .cuda(), .float()) re-materialises its store and comes through this branch.
            slots = lambda mod: [(m._buffers, k) for m in mod.modules() for k, b in m._buffers.items() if b is not None]
            self._buf_slots = list(zip(slots(src), slots(self.ema)))
            if any(ks != ke for (_, ks), (_, ke) in self._buf_slots) or len(slots(src)) != len(slots(self.ema)):
                raise RuntimeError("FusedModelEma: the model's buffers and the averaged model's do not pair up by name")
            self._buf_key = None
            self._layout_key = key
        key = (S.P.data_ptr(), E.P.data_ptr(), tuple(p.requires_grad for p in S._plist))
        if self._mask_key != key:                # a store was re-materialised, or a parameter was frozen / un-frozen (as FusedAdamW's mask)
            self._mask = None                    # nothing frozen: no mask, and the alignment gaps (zeros in both stores) average to zeros
            if not all(key[2]):
                mask = torch.zeros(S.total, dtype=torch.uint8)
                for name, p in S.params.items():
                    if not p.requires_grad:
                        off, n, _ = S.offsets[name]
                        mask[off:off + n] = ops.ADAMW_FROZEN
                self._mask = mask.to(dev)
            self._mask_key = key
        pairs = [(ds[ks], de[ke]) for (ds, ks), (de, ke) in self._buf_slots]
        key = tuple(t.data_ptr() for pair in pairs for t in pair)
        if self._buf_key != key:
            rows = []
            for b, e in pairs:
                if b.shape != e.shape or b.dtype != e.dtype or not (b.is_contiguous() and e.is_contiguous()):
                    raise RuntimeError("FusedModelEma: the model's buffers and the averaged model's differ in shape, dtype or layout")
                if b.dtype not in (torch.float32, torch.int64):
                    raise RuntimeError(f"FusedModelEma: a {b.dtype} buffer (fp32 buffers are averaged, int64 ones copied)")
                if b.numel():
                    rows.append([ops.ptr(e), ops.ptr(b), b.numel(), 0 if b.dtype == torch.float32 else 1])
            self._buf_n = len(rows)
            self._buf_table = torch.tensor(rows, dtype=torch.int64).to(dev) if rows else None
            self._buf_key = key
        return S, E

    @torch.no_grad()
    def update(self, model):
        """One launch over the parameters (+ one over the buffers, when the model has any) on the current stream, behind the optimizer step that was
        enqueued before it; no host wait, nothing read from the device."""
        S, E = self._ensure(_unwrap(model))
        d = self.decay_at(self.updates + 1)
        # Is the averaged model's bf16 copy current for its parameters as they stand BEFORE this launch?  Yes when its last refresh() cast (or accepted) it at this
        # version, or when an earlier update declared it fresh at this version; no for a store that has just been materialised (C is uninitialised: refresh()
        # makes the first cast) and after set() / load_state_dict() wrote the parameters.
        c_current = E.c_is_current()
        ops.ema_update(E.P, S.P, E.C, S.total, d, 1.0 - d, self._mask)
        if self._buf_n:
            ops.ema_update_buffers(self._buf_table, self._buf_n, d, 1.0 - d)
        self.updates += 1
        # as after FusedAdamW.step: the W^T / permuted conv copies (and what the MIM decoder folds out of the BatchNorm buffers) are refreshed by the averaged
        # model's next forward.  Its plain bf16 copy is declared current -- the forward then skips its cast -- only when this launch left it so: it wrote every
        # element (no mask), or the elements the mask made it skip were current already.  Otherwise refresh() casts, as for any store (one rule for
        # the optimizers and this update: FlatStore.c_written_by_kernel).
        E.c_written_by_kernel(c_current, wrote_all=self._mask is None)

    @torch.no_grad()
    def set(self, model):
        """the average becomes a copy of `model`: one flat copy for the parameters, one copy per buffer"""
        src = _unwrap(model)
        if src.store.P is None:
            self.ema.load_state_dict(src.state_dict())
            return
        S, E = self._ensure(src)
        E.P.copy_(S.P)                            # (bumps P's version: the next forward re-casts and refreshes)
        for b, e in zip(src.buffers(), self.ema.buffers()):
            e.copy_(b)
        E.force_dirty = True

    def state_dict(self):
        """The averaged model's state_dict -- what timm's get_state_dict(model_ema) stores; plus "_ema_updates", a key that the load hook of pvlt.PyramidVisionLanguageTransformer drops: the checkpoint loads into a plain model of that class, strict (any other
        module wants the key deleted first)."""
        sd = self.ema.state_dict()
        sd["_ema_updates"] = self.updates
        return sd

    def load_state_dict(self, sd):
        """Takes a checkpoint of state_dict() or any state_dict of the model (no "_ema_updates": `updates` stays as it is).  Works before the first
        forward: the values then wait in the averaged model's parameters until its store is built."""
        clean = type(sd)((k, v) for k, v in sd.items() if k != "_ema_updates") if isinstance(sd, dict) else sd
        if hasattr(sd, "_metadata"):
            clean._metadata = sd._metadata
        self.ema.load_state_dict(clean)
        self.ema.store.force_dirty = True
        if "_ema_updates" in sd:
            self.updates = int(sd["_ema_updates"])

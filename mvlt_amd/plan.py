"""The backward plan of a pass: what runs and what is kept for the parameters' current requires_grad flags, and the input-size rule with the
stage grids it leads to.  Pure Python over the model's names, depths and flags: nothing here touches the GPU or the library (it imports with no libmvlt_hip.so built)."""


def check_input_size(model, Himg, Wimg):
    """the reference's input rule: each side a multiple of patch_size * 8 = 32 (its patch embeddings halve the map three times and the MIM decoder's
    x2 upsamples must meet the skip maps again); rectangles are fine (reference libs/pvlt.py:166-172,291-297)"""
    unit = model.patch_size * 8
    assert Himg % unit == 0 and Wimg % unit == 0, \
        f"input size {Himg} x {Wimg} (H x W): each side should be divided by patch_size {unit} (rectangles are fine, as in the reference)"


def stage_grids(model, Himg, Wimg):
    """[(h_i, w_i)] token grids of the four stages for an Himg x Wimg input"""
    return [(Himg // model.patch_size // (2 ** i), Wimg // model.patch_size // (2 ** i)) for i in range(4)]


# =============================================================================================== backward plan (frozen parameters)
class PlanUnit:
    """One unit of the backward pass in the order the schedule visits it.
    launches: {launch group -> does it run}: a parameter-gradient launch runs when ANY parameter it writes is trainable (the optimizer's mask byte
              protects the frozen ones of a mixed launch); group "ln" are LayerNorm weights / biases, whose gradients ride in kernels that run for dx.
    wgrad: some parameter of the unit is trainable.  dgrad: the unit's input gradient is needed (a unit visited later has a trainable parameter).
    save: the forward keeps the unit's activations (= the backward gets as far as this unit)."""
    __slots__ = ("name", "kind", "params", "launches", "wgrad", "dgrad", "save")

    def __init__(self, name, kind, groups, live):
        self.name, self.kind = name, kind
        self.params = {k: tuple(v) for k, v in groups.items()}
        self.launches = {k: any(n in live for n in v) for k, v in groups.items()}
        self.wgrad = any(self.launches.values())
        self.dgrad = self.save = False

    def only(self, *groups):
        """no launch group outside `groups` runs"""
        return not any(on for k, on in self.launches.items() if k not in groups)

    def __repr__(self):
        return f"PlanUnit({self.name}: wgrad={self.wgrad} dgrad={self.dgrad} save={self.save} {self.launches})"


class BackwardPlan:
    """units: [PlanUnit] -- the heads (they run first: autograd orders them among themselves), then block4.<last> .. block4.0, embed4 (patch_embed4,
    text_embed4, pos_embed4, text_pos_embed4), stage 3, 2, 1 likewise, and text_embeddings (the BERT embedding block) last.
    cut: index of the last unit with a trainable parameter (None: nothing is trainable); no unit behind it runs or saves."""

    def __init__(self, units, live):
        self.units, self.live = units, live
        self.by = {u.name: u for u in units}
        on = [k for k, u in enumerate(units) if u.wgrad]
        self.cut = on[-1] if on else None
        trunk_on = any(u.wgrad for u in units if u.kind != "head")
        for k, u in enumerate(units):
            # a head's input gradient feeds the trunk only (the heads do not feed each other)
            u.dgrad = trunk_on if u.kind == "head" else (self.cut is not None and k < self.cut)
            u.save = u.wgrad or u.dgrad
        self.trunk_save = any(u.save for u in units if u.kind != "head")

    @property
    def cut_unit(self):
        return None if self.cut is None else self.units[self.cut]

    def signature(self):
        return [(u.name, u.wgrad, u.dgrad, u.save, tuple(sorted(u.launches.items()))) for u in self.units]


class _EveryLaunch(dict):
    def __missing__(self, k):
        return True


class _EveryUnit(PlanUnit):
    """stand-in for any unit when a pass has no plan: every launch runs, everything is kept"""
    __slots__ = ()

    def __init__(self):
        self.name, self.kind, self.params, self.launches = "*", "all", {}, _EveryLaunch()
        self.wgrad = self.dgrad = self.save = True

    def only(self, *groups):
        return False


_EVERY = _EveryUnit()
WORD_TABLE = "text_embeddings.word_embeddings.weight"


def backward_plan(model):
    """What the backward pass of `model` runs for the parameters' current requires_grad flags.  Pure Python: reads requires_grad, depths, loss_type and
    the parameter names only (no GPU, no flat store).  The schedule asks for it at the start of every grad-enabled forward, so freezing and un-freezing
    between steps takes effect with the next step."""
    names = [n for n, _ in model.named_parameters()]
    live = frozenset(n for n, p in model.named_parameters() if p.requires_grad)
    have = set(names)
    lt = model.loss_type
    units = []

    def wb(prefix):
        return [n for n in (prefix + ".weight", prefix + ".bias") if n in have]

    if lt.get("mlm"):
        units.append(PlanUnit("mlm_head", "head", dict(
            table=[WORD_TABLE], bias=["mlm_head.bias"], dense=wb("mlm_head.transform.dense"), embed=wb("mlm_head_embed.0"),
            ln=wb("mlm_head.transform.LayerNorm") + wb("mlm_head_embed.1")), live))
    for h, on in (("itm", lt.get("itm")), ("sup_cls", lt.get("cls")), ("sub_cls", lt.get("cls"))):
        if on:
            units.append(PlanUnit(h + "_head", "head", dict(
                linear=[h + "_head.linear.weight"], bias=[h + "_head.linear.bias", h + "_head.linear_bias"], embed=wb(h + "_head_embed.0"),
                ln=wb(h + "_head_embed.1")), live))
    if lt.get("t2i"):
        units.append(PlanUnit("t2i_head", "head", dict(all=[n for n in names if n.startswith("t2i_head.")]), live))
    for i in (4, 3, 2, 1):
        for j in reversed(range(model.depths[i - 1])):
            p = f"block{i}.{j}."
            units.append(PlanUnit(f"block{i}.{j}", "block", dict(
                fc1=wb(p + "mlp.fc1"), fc2=wb(p + "mlp.fc2"), proj=wb(p + "attn.proj"), q=wb(p + "attn.q"), kv=wb(p + "attn.kv"), sr=wb(p + "attn.sr"),
                ln=wb(p + "norm1") + wb(p + "norm2") + wb(p + "attn.norm")), live))
        units.append(PlanUnit(f"embed{i}", "embed", dict(
            patch=wb(f"patch_embed{i}.proj"), text=wb(f"text_embed{i}.0"), pos=[f"pos_embed{i}", f"text_pos_embed{i}"],
            ln=wb(f"patch_embed{i}.norm") + wb(f"text_embed{i}.1")), live))
    units.append(PlanUnit("text_embeddings", "bert", dict(embed=[n for n in names if n.startswith("text_embeddings.")]), live))
    return BackwardPlan(units, live)


def _plan_for(model):
    """backward_plan(model), cached on the store under the requires_grad tuple (~230 attribute reads per forward)"""
    S = model.store
    key = (id(S.P), tuple(p.requires_grad for p in S._plist))
    hit = getattr(S, "_plan", None)
    if hit is None or hit[0] != key:
        hit = S._plan = (key, backward_plan(model))
    return hit[1]


def plan_unit(model, name):
    """the unit `name` of the pass's plan (`model._plan`: the model during its forward, or a step that took the plan along); without a plan a stand-in
    whose every launch runs"""
    plan = getattr(model, "_plan", None)
    return plan.by[name] if plan is not None else _EVERY

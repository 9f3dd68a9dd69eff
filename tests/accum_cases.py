"""Gradient accumulation over several backward passes into one flat buffer: the scenarios as data, what stock PyTorch leaves in `.grad` after each, and the
comparison both test files use (docs/accumulation.md).  Imports neither the library nor a GPU.

Two batches, *a* and *b*; the loss of *b* is multiplied by W = 0.5 before its backward, so that the four things a writer of the gradient buffer can do with a
second pass -- add it (g_a + 0.5 g_b), store it (0.5 g_b), drop it (g_a), add it twice (g_a + g_b) -- differ by order one.

A scenario is a script: a list of steps that a driver runs (tests/test_accum_cases_cpu.py drives a plain torch.nn model with autograd alone,
tests/test_accum_gpu.py the real model).  `expected` is the table of what `.grad` holds afterwards; it is written down, not derived from the script, and
pinned to torch by the CPU test."""
import torch

W = 0.5                                # factor on the loss of batch b
ALIGN = 8                              # FlatStore's slice alignment (elements)
WORD_TABLE = "text_embeddings.word_embeddings.weight"
POS_TABLE = "text_embeddings.position_embeddings.weight"
TYPE_TABLE = "text_embeddings.token_type_embeddings.weight"

# steps: ("fwd", tag, batch)  grad-enabled forward of batch "a" / "b", its loss kept under `tag`
#        ("bwd", tag, factor) (factor * loss[tag]).backward(), the graph freed
#        ("zero",)            zero_grad(set_to_none=False)
#        ("none", subset)     p.grad = None for the subset
#        ("foreign", subset)  p.grad = a non-aliasing tensor holding extra["r"][name], for the subset
#        ("clip",)            clip_grad_norm_(parameters, extra["max_norm"])
#        ("freeze", subset)   requires_grad_(False) for the subset
#        ("eval", batch)      eval-mode forward under no_grad, then train mode again
#        ("drop", tag)        the loss kept under `tag` and its graph are dropped without a backward
#        ("die", tag)         loss[tag].backward() raises half way (a host exception)
#        ("check", label)     the driver's own assertions at this point
SCENARIOS = {
    "plain": [("fwd", "a", "a"), ("bwd", "a", 1.0), ("check", "after_pass1"), ("fwd", "b", "b"), ("bwd", "b", W), ("check", "after_pass2")],
    "zero_keep": [("fwd", "a", "a"), ("bwd", "a", 1.0), ("zero",), ("fwd", "b", "b"), ("bwd", "b", W)],
    "mixed_alternate": [("fwd", "a", "a"), ("bwd", "a", 1.0), ("none", "alternate"), ("fwd", "b", "b"), ("bwd", "b", W)],
    "mixed_stage2_word": [("fwd", "a", "a"), ("bwd", "a", 1.0), ("none", "stage2_word"), ("fwd", "b", "b"), ("bwd", "b", W)],
    "foreign": [("fwd", "a", "a"), ("bwd", "a", 1.0), ("foreign", "third"), ("fwd", "b", "b"), ("bwd", "b", W), ("check", "sync")],
    "clip": [("fwd", "a", "a"), ("bwd", "a", 1.0), ("clip",), ("fwd", "b", "b"), ("bwd", "b", W), ("check", "nothing_pending")],
    "inflight_ba": [("fwd", "a", "a"), ("check", "pending1"), ("fwd", "b", "b"), ("check", "pending2"), ("bwd", "b", W), ("check", "pending1"),
                    ("bwd", "a", 1.0), ("check", "pending0")],
    "inflight_ab": [("fwd", "a", "a"), ("check", "pending1"), ("fwd", "b", "b"), ("check", "pending2"), ("bwd", "a", 1.0), ("check", "pending1"),
                    ("bwd", "b", W), ("check", "pending0")],
    "inflight_dropped": [("fwd", "a", "a"), ("eval", "b"), ("fwd", "b", "b"), ("drop", "b"), ("bwd", "a", 1.0), ("check", "pending0")],
    "died": [("fwd", "a", "a"), ("die", "a"), ("none", "all"), ("fwd", "a2", "a"), ("bwd", "a2", 1.0), ("check", "after_dead")],
    "freeze": [("fwd", "a", "a"), ("bwd", "a", 1.0), ("freeze", "stages12"), ("check", "clone_frozen"), ("fwd", "b", "b"), ("bwd", "b", W)],
}

# name -> (subset or None, (coefficient of g_a, of g_b) inside the subset, adds extra["r"], `.grad` aliases the flat buffer inside the subset,
#          (coefficients) outside it).  "c" stands for extra["c"], the clip coefficient max_norm / (|g_a| + 1e-6).
TABLE = {
    "plain": (None, None, False, True, (1.0, W)),
    "zero_keep": (None, None, False, True, (0.0, W)),
    "mixed_alternate": ("alternate", (0.0, W), False, True, (1.0, W)),
    "mixed_stage2_word": ("stage2_word", (0.0, W), False, True, (1.0, W)),
    "foreign": ("third", (0.0, W), True, False, (1.0, W)),
    "clip": (None, None, False, True, ("c", W)),
    "inflight_ba": (None, None, False, True, (1.0, W)),
    "inflight_ab": (None, None, False, True, (1.0, W)),
    "inflight_dropped": (None, None, False, True, (1.0, 0.0)),
    "died": (None, None, False, True, (1.0, 0.0)),
    "freeze": ("stages12", (1.0, 0.0), False, False, (1.0, W)),      # a frozen parameter keeps the `.grad` tensor it had; kernels may still write its slice of G
}

_STAGE12 = tuple(f"{k}{i}" for i in (1, 2) for k in ("patch_embed", "text_embed", "block", "pos_embed", "text_pos_embed"))


def _in_stage(name, stages):
    return any(name == s or name.startswith(s + ".") for s in stages)


def subset(key, names):
    """the parameter names a step of a script means, out of `names` in store order"""
    names = list(names)
    if key == "all":
        return names
    if key == "alternate":
        return names[1::2]
    if key == "third":
        return names[::3]
    if key == "stage2_word":
        return [n for n in names if _in_stage(n, _STAGE12[5:]) or n == WORD_TABLE]
    if key == "stages12":
        return [n for n in names if _in_stage(n, _STAGE12)]
    raise KeyError(key)


def coefficients(scenario, names, extra=None):
    """{name: (coefficient of g_a, coefficient of g_b, adds r, alias)}"""
    sub_key, sub_coef, adds_r, sub_alias, rest = TABLE[scenario]
    sub = set(subset(sub_key, names)) if sub_key else set()
    res = {}
    for n in names:
        ca, cb = sub_coef if n in sub else rest
        if ca == "c":
            ca = float(extra["c"])
        res[n] = (ca, cb, adds_r and n in sub, sub_alias if n in sub else True)
    return res


def expected(scenario, g_a, g_b, names, extra=None):
    """What stock PyTorch leaves in `.grad` of every parameter of `names` after the scenario, from the two single-pass gradients g_a and g_b (dicts by name,
    of tensors, arrays or numbers: the combination is linear), and whether `.grad` must alias its slice of the flat buffer: {name: (value, alias)}.
    extra: {"c": clip coefficient (scenario "clip"), "r": {name: foreign tensor} (scenario "foreign")}."""
    res = {}
    for n, (ca, cb, adds_r, alias) in coefficients(scenario, names, extra).items():
        v = ca * g_a[n] + cb * g_b[n]
        if adds_r:
            v = v + extra["r"][n]
        res[n] = (v, alias)
    return res


def run_script(scenario, driver):
    """run the scenario's steps on `driver` (an object with one method per step kind)"""
    for step in SCENARIOS[scenario]:
        getattr(driver, step[0])(*step[1:])


# ------------------------------------------------------------------ comparison
def row_groups(name, ids, T):
    """The row groups three tensors are compared in, each against its own norm: [(label, row index tensor)] or None for every other parameter.  A lookup-row
    contribution that is lost must not hide inside the dense decoder gradient (40 rows of 30522: 3.6 % of the norm when all rows weigh the same)."""
    if name == WORD_TABLE:
        used = torch.unique(torch.as_tensor(ids).reshape(-1))
        return [("rows looked up in a or b", used), ("other rows", None)]
    if name == POS_TABLE:
        return [("rows < T", torch.arange(T)), ("rows >= T", None)]
    if name == TYPE_TABLE:
        return [("row 0", torch.arange(1)), ("rows >= 1", None)]
    return None


def _split(t, groups):
    if groups is None:
        return [("", t)]
    (la, rows), (lb, _) = groups
    rows = rows.to(t.device)
    rest = torch.ones(t.shape[0], dtype=torch.bool, device=t.device)
    rest[rows] = False
    return [(la, t[rows]), (lb, t[rest])]


def compare(got, want, bar, groups=None, cancel=None, record=None, tag=""):
    """Relative L2 error of got[name] against want[name] per parameter (per row group where groups[name] says so), each against its own expected norm; parameters
    whose expected norm is below 1e-7 are skipped.  A row group whose expected norm is below 1e-7 while its parameter's is not (position rows no caption reaches)
    is measured against the parameter's norm: what is expected there is zero, and anything else is an error of that size.  cancel: {name: c >= 1}, the error of
    these tensors is divided by c (the bf16 ITM tensors whose batch sum cancels, as in test_train_step_parity).  record(quantity, achieved, bound) -> bool is
    the `parity` fixture (None: plain comparison).  -> {(name, group label): achieved error} of everything over the bar."""
    bad = {}
    for name, w in want.items():
        g = got[name]
        w = torch.as_tensor(w).detach().to(device=g.device, dtype=torch.float64)
        g = g.detach().to(torch.float64)
        assert g.shape == w.shape, (name, tuple(g.shape), tuple(w.shape))
        wn_all = w.norm().item()
        if wn_all < 1e-7:
            continue
        for (label, gp), (_, wp) in zip(_split(g, (groups or {}).get(name)), _split(w, (groups or {}).get(name))):
            if wp.numel() == 0:
                continue
            wn = wp.norm().item()
            e = (gp - wp).norm().item() / (wn if wn >= 1e-7 else wn_all) / (cancel or {}).get(name, 1.0)
            q = f"{tag}/{name}" + (f"[{label}]" if label else "")
            ok = record(q, e, bar) if record is not None else e <= bar
            if not ok or e != e:
                bad[(name, label)] = e
    return bad


def cancel_factor(parts):
    """c = sqrt(sum r^2) / |sum r| (>= 1 taken) over the combined per-pair residuals r of the passes that went into a sum: parts = [(factor, residuals a_b of
    that pass)] -- the un-cancelled scale of a batch sum of signed per-pair terms (the ITM biases; tests/test_model_gpu.py, test_train_step_parity)."""
    r = torch.cat([float(f) * torch.as_tensor(a, dtype=torch.float64).reshape(-1) for f, a in parts if f])
    return max(1.0, float(r.pow(2).sum().sqrt() / r.sum().abs().clamp_min(1e-12)))


def gaps(offsets):
    """[(lo, hi)] of the alignment gaps of a flat layout {name: (offset, numel, shape)}: between each parameter's end and its aligned end"""
    res = []
    for off, n, _ in offsets.values():
        hi = off + (n + ALIGN - 1) // ALIGN * ALIGN
        if hi > off + n:
            res.append((off + n, hi))
    return res

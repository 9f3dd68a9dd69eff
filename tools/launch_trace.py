"""Every launch of a pass, argument for argument: one JSON line per call into libmvlt_hip.so, to compare two trees whose host side differs and whose
library does not (the host-side counterpart of tools/isa_kernel_equiv.py).  `mvlt_amd._lib.lib` is replaced by a proxy that records every mvlt_* entry:
integers and floats as they are, argument structs field by field, a pointer into one of the flat store's buffers as [buffer, byte offset] (so the trace
shows which parameter / gradient slice a launch gets), any other pointer as the ordinal of its first appearance (the aliasing pattern between launches);
the stream is dropped.  Imports only what is stable across host-side refactors (pvlt, engine.compute_losses, _lib, the oracle's batch filler and
tests/test_freeze_gpu.py's apply_setting).

    python tools/launch_trace.py --pass a --out traces/new        # a..f, g_<setting>, h: see PASSES; prints launches and SHA-256 of the file
One pass per process: which freed block the caching allocator hands out next (the ordinals) is not stable across the models of one process.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch                                             # noqa: E402
from mvlt_amd import _lib as L, pvlt                     # noqa: E402
from mvlt_amd.engine import compute_losses               # noqa: E402
from oracle import filler, pvlt_oracle as O              # noqa: E402

B, T, SEED, DEV = 2, 8, 7, "cuda:0"
LT_ALL, LT_CLS, LT_MLM = dict(mlm=1, itm=1, t2i=1, cls=0), dict(mlm=0, itm=0, t2i=0, cls=1), dict(mlm=1, itm=0, t2i=0, cls=0)
FROZEN = ("heads", "text", "lower", "one", "patch1", "fc2s3", "pos3")
PASSES = dict(a="bf16 step, mlm (fused) + itm + t2i with target, DropPath 0.1, 64 x 64", b="as a, 96 x 64", c="as a, fp32", d="bf16 step, cls heads only",
              e="bf16 eval under no_grad, full MLM logits, folded-BN decoder", f="bf16 step, full MLM logits",
              h="forward_pyramid_features_vl, grad enabled, everything frozen", **{"g_" + s: "as a, frozen setting " + s for s in FROZEN})


class Recorder:
    """stands where _lib.lib stands: attribute lookup hands out the entry wrapped in a recording closure"""

    def __init__(self, lib):
        self._lib, self.store, self.lines, self._seen = lib, None, [], {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mvlt_"):
            return fn

        def call(*args):
            types = fn.argtypes or [None] * len(args)
            if args and types[-1] is C.c_void_p and (args[-1] or 0) == L.stream_ptr():
                args_rec = args[:-1]
            else:
                args_rec = args
            self.lines.append(json.dumps([name] + [self._value(a, t) for a, t in zip(args_rec, types)]))
            return fn(*args)
        return call

    def _buffers(self):
        S = self.store
        if S is None or S.P is None:
            return []
        named = [("P", S.P), ("C", S.C), ("G", S.G), ("taps", getattr(S, "_tap_arena", None)), ("ln", getattr(S, "_ln_arena", None)),
                 ("tn_partials", getattr(S, "_tn_partials", None))] + [("extra:" + k, v) for k, v in S.extra.items()]
        return [(k, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for k, t in named if t is not None and t.is_cuda]

    def _pointer(self, p):
        if not p:
            return None
        for name, lo, hi in self._buffers():
            if lo <= p < hi:
                return [name, p - lo]
        return "#%d" % self._seen.setdefault(p, len(self._seen))

    def _value(self, a, t):
        if hasattr(a, "_obj"):                           # byref(struct)
            a = a._obj
        if isinstance(a, C.Structure):
            return {f: self._value(getattr(a, f), ft) for f, ft in a._fields_}
        if isinstance(a, C.Array):
            return [self._value(x, a._type_) for x in a]
        if t is C.c_void_p or (a is None and t is not None):
            return self._pointer(a)
        return a.decode() if isinstance(a, bytes) else a


def model_of(lt, dtype=torch.bfloat16, dpr=0.1):
    torch.manual_seed(SEED)
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=lt, pretrained_pth=None, drop_path_rate=dpr,
                       compute_dtype=dtype, img_size=64)
    m.injected_masks = None
    return m.to(DEV).train()


def step(m, h=64, w=64, labels=True, target=True):
    """one forward + backward with every loss the model has"""
    b = {k: v.to(DEV) for k, v in O.to_torch_batch(filler.make_batch(SEED, B, max(h, w), T)).items()}
    img = b["image"][:, :, :h, :w].contiguous()
    kw = dict(mlm_labels=b["mlm_labels"]) if labels and m.loss_type["mlm"] else {}
    if target and m.loss_type["t2i"]:
        kw["t2i_target"] = img
    out = m(img, b["input_ids"], **kw)
    if torch.is_grad_enabled():
        compute_losses(out, img, b["mlm_labels"], b["itm_labels"], b["sup_cls_labels"], b["sub_cls_labels"])[0].backward()
    torch.cuda.synchronize()


def run(name, rec, out_dir, make, go):
    torch.manual_seed(SEED)
    m = make()
    rec.store, rec.lines, rec._seen = m.store, [], {}
    torch.manual_seed(SEED)                              # the Philox (seed, call) pairs of the step's masks are part of the trace
    go(m)
    text = "\n".join(rec.lines) + "\n"
    with open(os.path.join(out_dir, f"trace_{name}.jsonl"), "w") as f:
        f.write(text)
    print(f"{name}: {len(rec.lines)} launches, sha256 {hashlib.sha256(text.encode()).hexdigest()}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pass", dest="which", required=True, choices=sorted(PASSES))
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    rec = L.lib = Recorder(L.lib)
    p = a.which
    if p in ("a", "b", "c"):
        run(p, rec, a.out, lambda: model_of(LT_ALL, torch.float32 if p == "c" else torch.bfloat16), lambda m: step(m, 96 if p == "b" else 64, 64))
    elif p == "d":
        run(p, rec, a.out, lambda: model_of(LT_CLS, dpr=0.0), step)
    elif p == "e":
        def go(m):
            with torch.no_grad():
                step(m.eval(), labels=False, target=False)
        run(p, rec, a.out, lambda: model_of(LT_ALL), go)
    elif p == "f":
        run(p, rec, a.out, lambda: model_of(LT_MLM), lambda m: step(m, labels=False))
    elif p.startswith("g_"):
        from test_freeze_gpu import apply_setting

        def make():
            m = model_of(LT_ALL)
            apply_setting(m, p[2:])
            return m
        run(p, rec, a.out, make, step)
    else:
        def make():
            m = model_of(LT_ALL)
            for q in m.parameters():
                q.requires_grad_(False)
            return m

        def go(m):
            b = O.to_torch_batch(filler.make_batch(SEED, B, 64, T))
            m.forward_pyramid_features_vl(b["image"].to(DEV), b["input_ids"].to(DEV))
            torch.cuda.synchronize()
        run(p, rec, a.out, make, go)


if __name__ == "__main__":
    main()

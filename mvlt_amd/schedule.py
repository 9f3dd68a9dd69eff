"""The entry points of a pass of the MI355X PVLT: the trunk (mvlt_amd/trunk.py), then the heads the loss types ask for (mvlt_amd/heads.py, mvlt_amd/mim.py),
under the backward plan (mvlt_amd/plan.py) read from the parameters' requires_grad flags at the start of the pass."""
import torch

from . import ops
from .heads import _ClsHeadFn, _GradSink, _MLMFullFn, _MLMFusedFn
from .mim import mim_head
from .params import ZeroPool, pool_zeros
from .plan import _plan_for, stage_grids
from .trunk import TrunkStep, _FrozenTrunkFn, _TrunkFn


class _HostCount:
    """A device int32 counter on its way to the host without draining the launch queue: an asynchronous copy into pinned
    memory plus an event recorded right behind it.  `get()` waits for that event only -- the kernels queued after it (the
    whole trunk forward, when the selection is the first launch of the step) keep the GPU busy meanwhile."""
    _pins = {}

    def __init__(self, cnt):
        key = (cnt.device.index, cnt.numel())
        pin = self._pins.get(key)
        if pin is None:
            pin = self._pins[key] = torch.empty(cnt.numel(), dtype=cnt.dtype).pin_memory()
        self.pin = pin
        pin.copy_(cnt, non_blocking=True)
        self.ev = torch.cuda.Event()
        self.ev.record()

    def get(self):
        self.ev.synchronize()
        return int(self.pin[0])


def run_forward(model, images, ids, mlm_labels=None, mlm_positions=None, mlm_count=None, t2i_target=None):
    """mlm_labels: (B, T) int64 with -1 = not selected -> fused masked-row MLM head + loss (`mlm_loss`).
    t2i_target: (B, 3, H, W) fp32 clean image -> the MIM decoder returns its SmoothL1 loss (`t2i_loss`) instead of `t2i_logits`
    (training: the image-sized prediction is never materialised, engine_grid_masking.py:99 is fused behind vl_heads.py:163-165).
    mlm_positions: optional precomputed selection (ascending flat indices, int32, on the device).
    mlm_count: optional number of selected positions as a host int (the engine counts on the host when the loader hands it
    CPU labels; the device prefetcher brings it along) -- without it the count comes back through `_HostCount`."""
    S = model.store
    dev = images.device
    grad_on = _begin_pass(model, dev)
    lt = model.loss_type
    sel = None
    if lt['mlm'] and mlm_labels is not None and mlm_positions is None:
        # masked-index selection (bit-exact vs torch.nonzero): first launch of the step, so that its count is on the host long
        # before the MLM head needs it to size its launches
        flat = mlm_labels.reshape(-1).contiguous()
        idx = torch.empty(flat.numel(), device=dev, dtype=torch.int32)
        cnt = pool_zeros((1,), torch.int32, dev)
        ops.masked_select(flat, idx, cnt)
        sel = (idx, mlm_count if mlm_count is not None else _HostCount(cnt))
    S.refresh(model._transposed, model._conv_perm, model._conv3)
    x1, x2, x3, x4 = _trunk(model, images, ids, grad_on, heads=True)
    sink = _GradSink(S) if grad_on else None            # the heads' common gradient buffer for x4
    B = images.shape[0]
    grids = stage_grids(model, images.shape[2], images.shape[3])
    HW4 = grids[3][0] * grids[3][1]
    out = dict(mlm_logits=None, itm_logits=None, sup_cls_logits=None, sub_cls_logits=None, t2i_logits=None)
    if lt['mlm']:
        if mlm_labels is not None:
            flat = mlm_labels.reshape(-1).contiguous()
            if sel is not None:
                idx, n = sel
                mlm_positions = idx[: (n if isinstance(n, int) else n.get())]
            if mlm_positions.numel() == 0:
                # nothing selected in this batch: CrossEntropyLoss(ignore_index=-1) averages over zero rows -> NaN, and no row
                # sends a gradient back (reference engine_grid_masking.py:84 behaves the same way)
                out["mlm_loss"] = torch.full((), float("nan"), device=dev)
            else:
                labels_sel = flat[mlm_positions.long()].contiguous()
                out["mlm_loss"] = _MLMFusedFn.apply(x4, model, HW4, mlm_positions.contiguous(), labels_sel, sink)
            out["mlm_positions"] = mlm_positions
        else:
            out["mlm_logits"] = _MLMFullFn.apply(x4, model, HW4, sink)
    if lt['itm']:
        out["itm_logits"] = _ClsHeadFn.apply(x4, model, "itm", HW4, sink)
    if lt['cls']:
        out["sup_cls_logits"] = _ClsHeadFn.apply(x4, model, "sup_cls", HW4, sink)
        out["sub_cls_logits"] = _ClsHeadFn.apply(x4, model, "sub_cls", HW4, sink)
    if lt['t2i']:
        if grad_on and not model.training:
            raise NotImplementedError("MIM decoder backward with eval-mode BatchNorm is not scheduled (no reference config needs it)")
        sides = tuple(grids[1:])                      # the (h, w) grids of the three pyramid levels the decoder reads
        fuse_loss = (t2i_target is not None and t2i_target.dtype == torch.float32 and t2i_target.shape == (B, 3, 8 * sides[0][0], 8 * sides[0][1])
                     and ops.upsample_l1_ok(sides[0][1], 8))
        if fuse_loss:
            out["t2i_loss"] = mim_head(model, x2, x3, x4, sides, grad_on, sink, t2i_target.contiguous())
        else:
            out["t2i_logits"] = mim_head(model, x2, x3, x4, sides, grad_on, sink)
    return out


def _begin_pass(model, dev):
    """common head of every forward entry: flat store on the device, one fill for all of this step's zero-initialised scratch"""
    S = model.store
    S.ensure(dev)
    # requires_grad is read HERE, once per forward: the plan of this pass (what its backward runs, what its forward keeps)
    model._plan = plan = _plan_for(model) if torch.is_grad_enabled() else None
    grad_on = plan is not None and plan.cut is not None
    model._pool_token = ZeroPool.of(dev).reset(grad_on)
    if grad_on:
        S.new_pass()                                              # a backward that raised must not poison this pass (FlatStore.new_pass)
    return grad_on


def _trunk(model, images, ids, grad_on, heads):
    """The four stage outputs.  With a trainable parameter in the trunk: one autograd node (_TrunkFn).  With none the trunk runs as it does under
    torch.no_grad() -- nothing kept, no node; `heads`: trainable heads follow, which reach their backward through _FrozenTrunkFn."""
    S = model.store
    params = [p for _, p in S.fn_params]
    if not grad_on or model._plan.trunk_save:
        return _TrunkFn.apply(model, images, ids, grad_on, *params)
    x1, x2, x3, x4 = TrunkStep(model, images, ids, False).forward()
    if not heads:
        model._pool_token = None
        return x1, x2, x3, x4
    return (x1, *_FrozenTrunkFn.apply(model, x2, x3, x4, *params))


def run_trunk(model, images, ids):
    """The trunk alone, behind `forward_pyramid_features_vl` (reference libs/pvlt.py:322-356): the four stage outputs as
    (B, HW_i + T, C_i) token buffers, image tokens first (differentiable: one autograd node, like in `run_forward`)."""
    S = model.store
    grad_on = _begin_pass(model, images.device)
    S.refresh(model._transposed, model._conv_perm, model._conv3)
    return _trunk(model, images, ids, grad_on, heads=False)

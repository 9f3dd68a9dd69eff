"""MIM decoder ("ITGHead", reference libs/vl_heads.py:107-165) as an explicit HIP kernel schedule.

Everything is pixel-major [M = B*H*W, C]: each conv3x3(pad 1) is mvlt_gemm_nt with the 3x3 neighbourhood row map
(im2col never exists in memory), its dgrad is the same gather with flipped/transposed taps, its wgrad is mvlt_gemm_tn with
the gather on the B operand.  BatchNorm uses the batch statistics of the local batch (train mode; the reference does
not convert to SyncBN) or the running statistics (eval), in fp32; the align_corners=True resizes and the three-way
feature products are fp32 kernels of csrc/mim.hip.  torch.cat is replaced by writing into column slices of the
concatenated buffers.  MFMA operands are the only tensors in the compute dtype.
"""
import torch

from . import layers, ops
from .layers import StoreAccess, _empty, linear, linear_bwd, saved
from .params import pool_zeros
from .plan import plan_unit
from ._lib import conv3map, rowmap

BN_EPS, BN_MOM = 1e-5, 0.1
STAT_COPIES = 16           # interleaved batch-statistic accumulators of the conv epilogue (see mvlt_gemm_nt_args.col_copies)
CONVS = ("reduction1", "reduction2", "reduction3", "conv_upsample1", "conv_upsample2", "conv_upsample3", "conv_upsample4",
         "conv_upsample5", "conv_concat2", "conv_concat3", "conv4")
_NO_BN_FOLD = False      # True (set in-process by the eval tests and tools/ubench_eval.py): eval mode keeps the separate BatchNorm pass over an fp32 z


def _z(shape, dev, dtype=torch.float32):
    return pool_zeros(shape, dtype, dev)                          # step-scoped scratch (params.ZeroPool)


class MimStep(StoreAccess):
    def __init__(self, model, x2, x3, x4, sides, training, need_grad):
        self.m, self.S = model, model.store
        self.dt = model.compute_dtype
        self.dev = x2.device
        self.x = (x2, x3, x4)                       # (B, N_i, C_i) stage outputs in the compute dtype, image tokens first
        self.B = x2.shape[0]
        self.s1, self.s2, self.s3 = sides           # (h, w) grids of the three levels: 32 x 32, 16 x 16, 8 x 8 at 256 px
        self.M1, self.M2, self.M3 = (self.B * h * w for h, w in sides)
        self.training = training
        self.need_grad = need_grad
        self.rec = {}                               # per conv: saved tensors for backward
        self.nbt = []                               # num_batches_tracked buffers of the BatchNorms run in train mode

    # ---- one conv3x3 (no bias) + BatchNorm: returns the record; y is produced by `norm`
    def conv_bn(self, name, xin, tokens_in, side, cin, cout, M):
        S, dev = self.S, self.dev
        p = f"t2i_head.{name}"
        amap = conv3map(side[0], side[1], tokens_in, cin)
        bn = getattr(self.m.t2i_head, name)[1]
        if not self.training and not self.need_grad and not _NO_BN_FOLD:
            # inference: BatchNorm on its running statistics is an affine map per output channel -- folded into the conv (`norm` launches it
            # with the destination it is given): no fp32 z, no normalisation pass, eleven launches fewer per forward
            r = dict(name=name, p=p, fold=self._folded(name, p, bn, cin, cout), xin=xin, amap=amap, cin=cin, cout=cout, M=M)
            self.rec[name] = r
            return r
        # z, the conv output BatchNorm normalises: written once, read three times (normalise, the two backward passes) and never an MFMA operand.  On
        # the bf16 path it is kept in fp16 -- the type the reference's autocast gives it -- with the batch statistics taken from the rounded values
        z16 = self.training and self.dt == torch.bfloat16
        z = _empty((M, cout), torch.float16 if z16 else torch.float32, dev)
        st = _z((2, STAT_COPIES, cout), dev) if self.training else (None, None)   # batch statistics ride on the conv's epilogue
        linear(xin, self.wK(p + ".0.weight"), z, M, a_map=amap, col_sum=st[0], col_sumsq=st[1], col_copies=STAT_COPIES)
        fin = None
        if self.training:
            mean, rstd = _empty((cout,), torch.float32, dev), _empty((cout,), torch.float32, dev)
            if z16 and cout % 8 == 0 and cout <= 256:
                # the statistics are finalised in the prologue of the normalisation launch (`norm`): eleven tiny launches fewer per step
                fin = (st[0], st[1], bn.running_mean, bn.running_var)
            else:
                ops.bn_finalize(st[0], st[1], M, cout, BN_EPS, BN_MOM, mean, rstd, bn.running_mean, bn.running_var, copies=STAT_COPIES)
            self.nbt.append(bn.num_batches_tracked)        # all eleven counters are bumped by one launch at the end of forward
        else:
            mean = bn.running_mean
            rstd = torch.rsqrt(bn.running_var + BN_EPS)
        r = dict(name=name, p=p, z=z, mean=mean, rstd=rstd, xin=xin, amap=amap, cin=cin, cout=cout, M=M, side=side,
                 tokens_in=tokens_in, fin=fin)
        self.rec[name] = r
        return r

    def _folded(self, name, p, bn, cin, cout):
        """-> (W', b'): W' = W * gamma * rsqrt(running_var + eps) per output channel, taken from the fp32 masters in the gather's
        [out][kh][kw][cin] order and rounded to the operand dtype ONCE; b' = beta - running_mean * gamma * rsqrt(...).  Cached on the model
        until the parameters' derived copies are refreshed again or the BatchNorm buffers are written."""
        S, m = self.S, self.m
        key = (S.refresh_count, bn.running_mean._version, bn.running_var._version, bn.num_batches_tracked._version, self.dt)
        cache = m.__dict__.setdefault("_mim_fold", {})
        hit = cache.get(name)
        if hit is None or hit[0] != key:
            scale = self.f32(p + ".1.weight") * torch.rsqrt(bn.running_var.float() + BN_EPS)
            shift = (self.f32(p + ".1.bias") - bn.running_mean.float() * scale).contiguous()
            wk = (self.f32(p + ".0.weight").permute(0, 2, 3, 1).reshape(cout, 9 * cin) * scale[:, None]).to(self.dt).contiguous()
            hit = cache[name] = (key, wk, shift)
        return hit[1], hit[2]

    def norm(self, r, y32=None, ld32=0, y16=None, ld16=0):
        if "fold" in r:
            wk, shift = r["fold"]
            for y in (y32, y16):
                if y is not None:
                    linear(r["xin"], wk, y, r["M"], a_map=r["amap"], bias=shift)
            return
        if r.get("fin") is not None:
            s1, s2, rm, rv = r["fin"]
            r["fin"] = None                                # (a second `norm` of the same record must not update the running statistics again)
            ops.bn_finalize_norm(r["z"], r["cout"], s1, s2, STAT_COPIES, BN_EPS, BN_MOM, r["mean"], r["rstd"], rm, rv, self.f32(r["p"] + ".1.weight"),
                                 self.f32(r["p"] + ".1.bias"), r["M"], r["cout"], y32, ld32, y16, ld16)
            return
        ops.bn_norm(r["z"], r["cout"], r["mean"], r["rstd"], self.f32(r["p"] + ".1.weight"), self.f32(r["p"] + ".1.bias"), r["M"], r["cout"],
                    y32, ld32, y16, ld16)

    def up2(self, x32, ldx, side, C, out=None, ldo=None):
        B = self.B
        if out is None:
            out, ldo = _empty((B * 4 * side[0] * side[1], C), self.dt, self.dev), C
        ops.upsample_fwd(x32, ldx, B, side[0], side[1], C, 2, out, ldo)
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, target=None):
        S, dev, dt, B = self.S, self.dev, self.dt, self.B
        x2, x3, x4 = self.x
        s1, s2, s3, M1, M2, M3 = self.s1, self.s2, self.s3, self.M1, self.M2, self.M3
        C2, C3, C4 = x2.shape[2], x3.shape[2], x4.shape[2]
        ch = 64
        f = self.rec
        # reductions of the three pyramid levels to 64 channels
        # the three factors of the full-resolution feature product (low, cu2o, cu3o: written once, read by the product and by its backward, never an
        # MFMA operand) are fp16 beside the fp16 z on the bf16 training path: 0.3 GB less traffic per step
        f16 = torch.float16 if (self.training and dt == torch.bfloat16) else torch.float32
        r = self.conv_bn("reduction1", x2, x2.shape[1], s1, C2, ch, M1); low = _empty((M1, ch), f16, dev); self.norm(r, low, ch)
        r = self.conv_bn("reduction2", x3, x3.shape[1], s2, C3, ch, M2); mid = _empty((M2, ch), torch.float32, dev); self.norm(r, mid, ch)
        r = self.conv_bn("reduction3", x4, x4.shape[1], s3, C4, ch, M3); high = _empty((M3, ch), torch.float32, dev); self.norm(r, high, ch)
        uph = self.up2(high, ch, s3, ch)                                   # (B,16,16,64) operand dtype
        HW1, HW2 = s1[0] * s1[1], s2[0] * s2[1]
        # a = cu1(up(high)) * mid            -> fp32 + operand copy into cat2[:, :64]
        cat2 = _empty((M2, 2 * ch), dt, dev)
        r = self.conv_bn("conv_upsample1", uph, HW2, s2, ch, ch, M2); cu1o = _empty((M2, ch), torch.float32, dev); self.norm(r, cu1o, ch)
        a = _empty((M2, ch), torch.float32, dev)
        ops.ew_mul(a, ch, cu1o, ch, mid, ch, M=M2, Cdim=ch, out16=cat2, ld16=2 * ch)
        r = self.conv_bn("conv_upsample4", uph, HW2, s2, ch, ch, M2); self.norm(r, y16=cat2[:, ch:], ld16=2 * ch)
        r = self.conv_bn("conv_concat2", cat2, HW2, s2, 2 * ch, 2 * ch, M2); c = _empty((M2, 2 * ch), torch.float32, dev); self.norm(r, c, 2 * ch)
        # b = cu2(up(mid)) * cu3(up(a)) * low -> fp32 + operand copy into cat3[:, :64]
        cat3 = _empty((M1, 3 * ch), dt, dev)
        upm = self.up2(mid, ch, s2, ch)
        r = self.conv_bn("conv_upsample2", upm, HW1, s1, ch, ch, M1); cu2o = _empty((M1, ch), f16, dev); self.norm(r, cu2o, ch)
        upa = self.up2(a, ch, s2, ch)
        r = self.conv_bn("conv_upsample3", upa, HW1, s1, ch, ch, M1); cu3o = _empty((M1, ch), f16, dev); self.norm(r, cu3o, ch)
        ops.ew_mul(None, 0, cu2o, ch, cu3o, ch, low, ch, M=M1, Cdim=ch, out16=cat3, ld16=3 * ch)
        upc = self.up2(c, 2 * ch, s2, 2 * ch)
        r = self.conv_bn("conv_upsample5", upc, HW1, s1, 2 * ch, 2 * ch, M1); self.norm(r, y16=cat3[:, ch:], ld16=3 * ch)
        d16 = _empty((M1, 3 * ch), dt, dev)
        r = self.conv_bn("conv_concat3", cat3, HW1, s1, 3 * ch, 3 * ch, M1); self.norm(r, y16=d16, ld16=3 * ch)
        e16 = _empty((M1, 3 * ch), dt, dev)
        r = self.conv_bn("conv4", d16, HW1, s1, 3 * ch, 3 * ch, M1); self.norm(r, y16=e16, ld16=3 * ch)
        # score: conv1x1 (192 -> 3) + bias, then x8 bilinear to the image, written as NCHW fp32
        sc = _empty((M1, 3), torch.float32, dev)
        linear(e16, S.extra["t2i_head.score.0.weight::W"], sc, bias=self.f32("t2i_head.score.0.bias"))
        if target is not None:
            # training with the loss fused behind the decoder: SmoothL1 against the target image while interpolating, the (B, 3, H, W)
            # prediction is never written (and the backward recomputes it from the score map)
            acc = pool_zeros((1,), torch.float32, dev)
            ops.upsample_l1_fwd(sc, 3, B, s1[0], s1[1], 3, 8, target, acc)
            out = (acc / target.numel()).reshape(())
            self.sc, self.target = sc, target
        else:
            out = _empty((B, 3, 8 * s1[0], 8 * s1[1]), torch.float32, dev)
            ops.upsample_fwd(sc, 3, B, s1[0], s1[1], 3, 8, out, 0, nchw=True)
        if self.nbt:
            torch._foreach_add_(self.nbt, 1)
            self.nbt = []
        if self.need_grad:
            self.keep = dict(low=low, mid=mid, cu1o=cu1o, cu2o=cu2o, cu3o=cu3o, e16=e16)
        else:
            self.rec = {}
        return out

    # ------------------------------------------------------------------ backward
    def bn_conv_bwd(self, name, dy, lddy, dx=None, accumulate=False, dx_map=None, dx_dtype=torch.float32, need_dx=True):
        """dy: fp32 gradient w.r.t. the BN output [M, cout] (row stride lddy).  Accumulates the BN / conv parameter gradients
        into the flat buffer and returns (or accumulates into) the gradient w.r.t. the conv input (need_dx=False: parameter gradients only)."""
        S, dev, dt = self.S, self.dev, self.dt
        r = self.rec[name]
        p, M, cin, cout = r["p"], r["M"], r["cin"], r["cout"]
        red = _z((2, cout), dev)
        ops.bn_bwd_reduce(dy, lddy, r["z"], cout, r["mean"], r["rstd"], M, cout, red[0], red[1])
        dz = _empty((M, cout), dt, dev)
        ops.bn_bwd_apply(dy, lddy, r["z"], cout, r["mean"], r["rstd"], self.f32(p + ".1.weight"), red[0], red[1], M, cout, dz, cout,
                         g_beta=self.g(p + ".1.bias"), g_gamma=self.g(p + ".1.weight"))
        # wgrad computed in the gather's [out][dy][dx][cin] order, accumulated at nn.Conv2d's [out][cin][3][3] place
        layers.conv_wgrad(S, p + ".0.weight", dz, r["xin"], r["amap"])
        if not need_dx:
            return None
        # dgrad: gather dz over the same grid with flipped taps
        gmap = conv3map(r["side"][0], r["side"][1], r["side"][0] * r["side"][1], cout)
        if dx is None:
            dx = _empty((M, cin), dx_dtype, dev)
        linear(dz, S.extra[p + ".0.weight::F"], dx, M, a_map=gmap, c_map=dx_map, R=dx if accumulate else None)
        return dx

    def backward(self, dout, sink=None, dgrad=True):
        """dgrad=False (nothing in the trunk is trainable): the three reductions give parameter gradients only, no gradient for x2 / x3 / x4"""
        S, dev, dt, B = self.S, self.dev, self.dt, self.B
        s1, s2, s3, M1, M2, M3 = self.s1, self.s2, self.s3, self.M1, self.M2, self.M3
        ch = 64
        k = self.keep
        # score head
        dsc_p = _z((M1, 8), dev, dt)                     # [pixels][3 -> 8] in the compute dtype: the operand of the two GEMMs below
        if getattr(self, "target", None) is not None:    # fused loss: dout is the scalar gradient of the loss
            ops.upsample_l1_bwd(self.sc, 3, B, s1[0], s1[1], 3, 8, self.target, dout.reshape(1).float().contiguous(), dsc_p, 8)
            self.sc = self.target = None
        else:
            dout = dout.contiguous().float()
            ops.upsample_bwd(dout, 0, True, B, s1[0], s1[1], 3, 8, dsc_p, 8)
        # the three 192-channel gradient maps at full resolution travel in the operand dtype (each is written once and read twice by the
        # BatchNorm backward behind it: 0.9 GB less traffic per step at batch 256); the maps further down stay fp32 (they are accumulated into)
        gd = dt if dt == torch.bfloat16 else torch.float32
        de = _empty((M1, 3 * ch), gd, dev)
        # weight gradient and, as the GEMM's column sum, the bias gradient (a torch sum over a [262144, 3] matrix took 92 us)
        linear_bwd(True, dsc_p, k["e16"], self.g("t2i_head.score.0.weight"), self.g("t2i_head.score.0.bias"), self.wT("t2i_head.score.0.weight"), de)
        dd = self.bn_conv_bwd("conv4", de, 3 * ch, dx_dtype=gd)
        dcat3 = self.bn_conv_bwd("conv_concat3", dd, 3 * ch, dx_dtype=gd)          # [:, :64] = db, [:, 64:] = d(cu5 out)
        dupc = self.bn_conv_bwd("conv_upsample5", dcat3[:, ch:], 3 * ch, dx_dtype=gd)
        dc = _empty((M2, 2 * ch), torch.float32, dev)
        ops.upsample_bwd(dupc, 2 * ch, False, B, s2[0], s2[1], 2 * ch, 2, dc, 2 * ch)
        # b = cu2o * cu3o * low
        db = dcat3                                                                  # columns [0, 64), row stride 192
        dcu2o, dcu3o, dlow = _empty((M1, ch), gd, dev), _empty((M1, ch), gd, dev), _empty((M1, ch), gd, dev)
        ops.ew_mul3_bwd(db, 3 * ch, k["cu2o"], k["cu3o"], k["low"], ch, dcu2o, dcu3o, dlow, M1, ch)
        # gradient of cat2 = [a | cu4 out]: starts with the path a -> up -> cu3
        dcat2 = _z((M2, 2 * ch), dev)
        dupa = self.bn_conv_bwd("conv_upsample3", dcu3o, ch, dx_dtype=gd)
        ops.upsample_bwd(dupa, ch, False, B, s2[0], s2[1], ch, 2, dcat2, 2 * ch, accumulate=True)
        dupm = self.bn_conv_bwd("conv_upsample2", dcu2o, ch, dx_dtype=gd)
        dmid = _empty((M2, ch), torch.float32, dev)
        ops.upsample_bwd(dupm, ch, False, B, s2[0], s2[1], ch, 2, dmid, ch)
        self.bn_conv_bwd("conv_concat2", dc, 2 * ch, dx=dcat2, accumulate=True)
        duph = self.bn_conv_bwd("conv_upsample4", dcat2[:, ch:], 2 * ch)
        # a = cu1o * mid
        dcu1o = _empty((M2, ch), torch.float32, dev)
        ops.ew_mul(dcu1o, ch, dcat2, 2 * ch, k["mid"], ch, M=M2, Cdim=ch)
        ops.ew_mul(dmid, ch, dcat2, 2 * ch, k["cu1o"], ch, M=M2, Cdim=ch, accumulate=True)
        self.bn_conv_bwd("conv_upsample1", dcu1o, ch, dx=duph, accumulate=True)
        dhigh = _empty((M3, ch), torch.float32, dev)
        ops.upsample_bwd(duph, ch, False, B, s3[0], s3[1], ch, 2, dhigh, ch)
        # reductions: gradients w.r.t. the image tokens of the stage outputs (text rows stay zero)
        grads = []
        for name, dy, x, side in (("reduction1", dlow, self.x[0], s1), ("reduction2", dmid, self.x[1], s2), ("reduction3", dhigh, self.x[2], s3)):
            if not dgrad:
                self.bn_conv_bwd(name, dy, ch, need_dx=False)
                grads.append(None)
                continue
            if name == "reduction3" and sink is not None:
                dxs, ret = sink.take(x.shape, x.dtype, x.device)      # the heads' common buffer: image rows are this decoder's
            else:
                dxs = ret = S.own(torch.empty_like(x))     # image rows are all written by the conv dgrad below;
                dxs[:, side[0] * side[1]:].zero_()         # only the text rows need the explicit zeros
            self.bn_conv_bwd(name, dy, ch, dx=dxs, dx_map=rowmap(side[0] * side[1], x.shape[1], 0))
            grads.append(ret)
        self.rec, self.keep = {}, {}
        return grads


class _MimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, x3, x4, model, sides, need_grad, sink=None, target=None):
        step = MimStep(model, x2, x3, x4, sides, model.training, need_grad)
        out = step.forward(target)
        ctx.step, ctx.sink = step, sink
        ctx.dgrad = plan_unit(model, "t2i_head").dgrad
        return out

    @staticmethod
    def backward(ctx, dout):
        step = saved(ctx.step)
        step.S.queue_finalize()
        g2, g3, g4 = step.backward(dout, ctx.sink, ctx.dgrad)
        ctx.step = ctx.sink = None
        step.S.fold_copies(early=True)                # the conv weight gradients leave the tap arena for G (with a data-parallel wrapper: now)
        step.S.announce_prefix("t2i_head.")          # the decoder's gradients are final: reduce them under the trunk backward
        return g2, g3, g4, None, None, None, None, None


def mim_head(model, x2, x3, x4, sides, need_grad, sink=None, target=None):
    """sides: the (h, w) token grids of stages 2-4.  -> t2i_logits (B, 3, 8 h_2, 8 w_2), or with `target` (fp32 NCHW image) the mean SmoothL1 loss against it as a 0-dim tensor"""
    return _MimFn.apply(x2, x3, x4, model, sides, need_grad, sink, target)

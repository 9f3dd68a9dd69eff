"""The trunk's forward / backward kernel schedule (the work that reference libs/pvlt.py:322-356 and its autograd graph do with dozens of
ATen kernels per block), and the autograd nodes that carry it.

Data layout: one token-major activation buffer (B, HW+T, C) per stage in the compute dtype; image tokens first.
  * PatchEmbed / Attention.sr (kernel==stride convs) read it through a patch row-map inside the GEMM loader
  * text tokens are the row range [HW, HW+T) (row-map), so there is no torch.cat / torch.split / NCHW permute
  * LN(+pos-embed) epilogues write straight into the concatenated buffer
Backward is scheduled by hand: every weight gradient is accumulated by the wgrad GEMM directly into the flat fp32
gradient buffer (no autograd accumulate pass), input gradients reuse buffers in place.
"""
import torch

from . import layers, ops
from ._lib import patchmap, rowmap
from .layers import StoreAccess, _empty, linear, linear_bwd, saved
from .params import pool_zeros
from .plan import check_input_size, plan_unit, stage_grids
from .pvlt import BERT_DROP, EPS_BERT, EPS_BLOCK, EPS_DEFAULT


def _step_rng(model):
    """(seed, call) of the next draw of the step's own train-mode masks (BERT dropout, DropPath): the seed is torch's
    (torch.manual_seed(args.seed + rank), reference main_vl.py:207-209, so ranks draw different masks), the counter runs per model"""
    model._rng_calls = getattr(model, "_rng_calls", 0) + 1
    return torch.initial_seed(), model._rng_calls


# =============================================================================================== trunk
class TrunkStep(StoreAccess):
    """One forward (and optionally backward) of the 4-stage trunk."""

    def __init__(self, model, images, ids, need_grad, plan=None):
        self.m = model
        self.S = model.store
        self._plan = plan if need_grad else None     # BackwardPlan of this pass (None: every unit runs, as if all parameters were trainable)
        self.dev = images.device
        self.dt = model.compute_dtype       # GEMM / attention operand dtype
        self.rt = torch.float32             # residual-stream dtype: adds and LayerNorm inputs stay fp32 (what the
        #                                     reference's autocast region does too); only MFMA operands are bf16
        self.need_grad = need_grad
        self.images = images.contiguous().float()
        self.ids = ids.contiguous()
        self.B = images.shape[0]
        assert images.shape[1] == model.in_chans
        Himg, Wimg = images.shape[2], images.shape[3]
        check_input_size(model, Himg, Wimg)
        self.Himg, self.Wimg = Himg, Wimg
        self.T = ids.shape[1]
        assert self.T == model.T_num, "input_ids length must equal num_text_tokens"
        self.grid = stage_grids(model, Himg, Wimg)       # (h_i, w_i) token grid of every stage
        self.saved = []          # per stage dict
        self.training = model.training

    def _mark(self):
        """bench.py: HIP events around the Block kernels of a stage (SRAttention + MLP incl. their LayerNorms), in pairs, on the
        launch stream -- the blocks-only GPU time behind north_star's MFMA-utilisation figure.  Off unless model._block_events
        is a list."""
        ev = getattr(self.m, "_block_events", None)
        if ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

    def keeps(self, name):
        """does the forward keep the activations of unit `name`"""
        return self.need_grad and plan_unit(self, name).save

    # ---- pos embed: learned for the constructor grid, bilinearly resized (align_corners=False) to this input's grid
    def _pos(self, i, param):
        m = self.m
        (h, w), C = self.grid[i], m.dims[i]
        HW = h * w
        pe = (param[:, 1:] if i == 3 else param)[0]                 # (grid*grid, C) rows of the flat buffer; stage 4 skips the cls slot
        if HW == m.grids[0] ** 2:          # reference libs/pvlt.py:292 compares the patch COUNT with stage-1's constructor grid
            if HW != m.grids[i] ** 2:
                # a later stage whose grid has stage 1's constructor patch count (448 px at the default 224: stage 2 is 56 x 56) gets its
                # embedding unresized there, and the reference's `x + pos_embed` fails on the shapes; refuse the same way instead of reading
                # h * w rows of a grids[i]^2-row parameter
                raise RuntimeError(f"stage {i + 1}: a {h}x{w} token grid gets the {m.grids[i]}x{m.grids[i]} position embedding unresized "
                                   f"(reference libs/pvlt.py:292 compares every stage with stage 1's {m.grids[0] ** 2} patches): the reference "
                                   f"model cannot run this input size either")
            return pe          # (a non-square stage-1 grid of that count -- 392 x 8 at the default 224 -- adds the square embedding row for row, like the reference)
        return self._pos_pre[i]                # resized by the one launch at the start of the forward pass (`_pos_prefetch`)

    def _pos_prefetch(self):
        """the resized position embeddings of all four stages in ONE launch (they depend on parameters only)"""
        m = self.m
        jobs, self._pos_pre = [], {}
        for i in range(4):
            (h, w), C = self.grid[i], m.dims[i]
            if h * w == m.grids[0] ** 2:
                continue
            param = self.f32(f"pos_embed{i+1}")
            pe = (param[:, 1:] if i == 3 else param)[0]
            out = _empty((h * w, C), torch.float32, self.dev)
            jobs.append((pe, out, m.grids[i], m.grids[i], h, w, C))
            self._pos_pre[i] = out
        if jobs:
            ops.resize_bilinear_tokens_multi(jobs)

    def _droppath_scales(self, blk_index):
        m = self.m
        rate = m.dpr[blk_index]
        if not self.training or rate == 0.0:
            return None, None
        inj = m.injected_masks
        if inj is not None:
            k1 = inj["droppath"][blk_index].to(self.dev, torch.float32)
            k2 = inj["droppath2"][blk_index].to(self.dev, torch.float32)
        else:
            if getattr(self, "_dp_all", None) is None:
                # every block's two keep masks in one draw (4 small launches per step instead of 8 per block)
                rates = getattr(m, "_dpr_dev", None)
                if rates is None or rates.device != self.dev:
                    rates = m._dpr_dev = torch.tensor(list(m.dpr), device=self.dev, dtype=torch.float32)
                self._dp_all = ops.droppath_scales(_empty((len(m.dpr), 2, self.B), torch.float32, self.dev), rates, *_step_rng(m))
            return self._dp_all[blk_index, 0], self._dp_all[blk_index, 1]
        return (k1 / (1.0 - rate)).contiguous(), (k2 / (1.0 - rate)).contiguous()

    # ------------------------------------------------------------------ forward
    def forward(self):
        m, S, B, T, dt, dev = self.m, self.S, self.B, self.T, self.dt, self.dev
        te = "text_embeddings."
        self._pos_prefetch()
        # BERT embeddings (+LN eps 1e-12, +dropout in train mode)
        rows = B * T
        self.emb = _empty((rows, m.hidden), dt, dev)
        self.emb_mean = _empty((rows,), torch.float32, dev)
        self.emb_rstd = _empty((rows,), torch.float32, dev)
        self.keep = None
        if self.training:
            inj = m.injected_masks
            if inj is not None:
                self.keep = inj["bert"].to(dev).reshape(rows, m.hidden).to(torch.uint8).contiguous()
            else:
                self.keep = ops.keep_mask(_empty((rows, m.hidden), torch.uint8, dev), BERT_DROP, *_step_rng(m))
        ops.bert_embed_fwd(self.ids, self.f32(te + "word_embeddings.weight"), self.f32(te + "position_embeddings.weight"),
                           self.f32(te + "token_type_embeddings.weight"), self.f32(te + "LayerNorm.weight"),
                           self.f32(te + "LayerNorm.bias"), self.keep, BERT_DROP, self.emb, self.emb_mean, self.emb_rstd,
                           rows, T, EPS_BERT)
        xp = None
        blk_index = 0
        outs = []
        for i in range(4):
            xp, blk_index = self._stage_forward(i, xp, blk_index)
            outs.append(xp)
            if i == 0 and not self.keeps("embed1"):
                self.emb = self.keep = None        # read again only by stage 1's text-embedding weight gradient and the BERT block's backward
        return outs

    def _stage_forward(self, i, xp, blk_index):
        m, B, T, dt, dev = self.m, self.B, self.T, self.dt, self.dev
        C = m.dims[i]
        h, w = self.grid[i]
        HW = h * w
        N = HW + T
        sv = dict(i=i, C=C, HW=HW, N=N)
        pe, ten = f"patch_embed{i+1}.", f"text_embed{i+1}."
        # ---- patch embed: kernel==stride conv as GEMM, then LN(1e-5) + pos-embed written into x[:, :HW]
        pe_pre = _empty((B * HW, C), dt, dev)
        if i == 0:
            K = m.in_chans * m.patch_size ** 2
            P1 = _empty((B * HW, K), dt, dev)
            ops.patchify(self.images, P1, B, m.in_chans, self.Himg, self.Wimg, m.patch_size)
            linear(P1, self.w(pe + "proj.weight"), pe_pre, bias=self.f32(pe + "proj.bias"))
            sv["P1"] = P1
        else:
            Cp, Np, wp = m.dims[i - 1], self.saved[i - 1]["N"], self.grid[i - 1][1]
            pm = patchmap(2, wp, Np, HW, w, Cp)
            linear(xp, self.wK(pe + "proj.weight"), pe_pre, B * HW, a_map=pm, bias=self.f32(pe + "proj.bias"))
            sv["pm_in"] = pm
        x = _empty((B, N, C), self.rt, dev)
        pos = self._pos(i, self.f32(f"pos_embed{i+1}"))
        sv["pe_pre"], sv["pe_mean"], sv["pe_rstd"] = pe_pre, _empty((B * HW,), torch.float32, dev), _empty((B * HW,), torch.float32, dev)
        # the first block's norm1 is chained onto the two embedding LayerNorms below (their output rows are in registers): that block
        # launches no LayerNorm of its own and the fp32 rows are not read back
        chain = None
        if dt == torch.bfloat16 and C in ops.LN_CHAIN_WIDTHS:
            p0 = f"block{i+1}.0."
            self._pre_ln1 = (_empty((B, N, C), dt, dev), _empty((B * N,), torch.float32, dev), _empty((B * N,), torch.float32, dev))
            chain = (self.f32(p0 + "norm1.weight"), self.f32(p0 + "norm1.bias"), EPS_BLOCK, *self._pre_ln1)
        ops.layernorm_fwd(pe_pre, x, self.f32(pe + "norm.weight"), self.f32(pe + "norm.bias"), B * HW, C, C, C, EPS_DEFAULT,
                          mean=sv["pe_mean"], rstd=sv["pe_rstd"], add=pos, add_rows=HW, y_map=rowmap(HW, N, 0), chain=chain)
        # ---- text embed: Linear + LN(1e-5) + text pos-embed written into x[:, HW:]
        te_pre = _empty((B * T, C), dt, dev)
        if i == 0:
            linear(self.emb, self.w(ten + "0.weight"), te_pre, bias=self.f32(ten + "0.bias"))
        else:
            Cp, Np, HWp = m.dims[i - 1], self.saved[i - 1]["N"], self.saved[i - 1]["HW"]
            linear(xp, self.w(ten + "0.weight"), te_pre, B * T, a_map=rowmap(T, Np, HWp), bias=self.f32(ten + "0.bias"))
        sv["te_pre"], sv["te_mean"], sv["te_rstd"] = te_pre, _empty((B * T,), torch.float32, dev), _empty((B * T,), torch.float32, dev)
        ops.layernorm_fwd(te_pre, x, self.f32(ten + "1.weight"), self.f32(ten + "1.bias"), B * T, C, C, C, EPS_DEFAULT,
                          mean=sv["te_mean"], rstd=sv["te_rstd"], add=self.f32(f"text_pos_embed{i+1}")[0], add_rows=T,
                          y_map=rowmap(T, N, HW), chain=chain)
        sv["x_in_prev"] = xp
        sv["blocks"] = []
        self._mark()
        for j in range(m.depths[i]):
            x, bsv = self._block_forward(i, j, x, blk_index)
            sv["blocks"].append(bsv)
            blk_index += 1
        self._mark()
        if x.dtype != dt:                    # MFMA-operand copy of the stage output (next stage's convs, the heads)
            xb = _empty((B, N, C), dt, dev)
            ops.cast_bf16(x, xb, x.numel())
            x = xb
        sv["x_out"] = x
        taps = getattr(m, "_taps", None)
        if taps is not None:            # tests: stage outputs in the reference's (img_feat NCHW, text_feat) form
            taps[f"img_feat{i+1}"] = x[:, :HW].float().reshape(B, h, w, C).permute(0, 3, 1, 2)
            taps[f"text_feat{i+1}"] = x[:, HW:].float()
        if not self.keeps(f"embed{i+1}"):       # the backward stops above this stage's embeddings (or there is none): only the shapes stay
            for k in ("P1", "pm_in", "pe_pre", "pe_mean", "pe_rstd", "te_pre", "te_mean", "te_rstd", "x_in_prev"):
                sv.pop(k, None)
        self.saved.append(sv)
        return x, blk_index

    def _block_forward(self, i, j, x, blk_index):
        m, B, T, dt, dev = self.m, self.B, self.T, self.dt, self.dev
        C, h, r, hid = m.dims[i], m.heads[i], m.sr[i], m.hid[i]
        gh, gw = self.grid[i]
        HW = gh * gw
        N = HW + T
        M = B * N
        p = f"block{i+1}.{j}."
        f32 = torch.float32
        keep = self.keeps(f"block{i+1}.{j}")       # (a block behind the backward plan's cut keeps nothing)
        bs = dict(x=x)
        s1, s2 = self._droppath_scales(blk_index)
        bs["s1"], bs["s2"] = s1, s2
        # LN1 (already done by the previous block's fused MLP epilogue where there is one)
        pre = getattr(self, "_pre_ln1", None)
        self._pre_ln1 = None
        if pre is not None:
            xn1, bs["m1"], bs["r1"] = pre
        else:
            xn1 = _empty((B, N, C), dt, dev)
            bs["m1"], bs["r1"] = _empty((M,), f32, dev), _empty((M,), f32, dev)
            ops.layernorm_fwd(x, xn1, self.f32(p + "norm1.weight"), self.f32(p + "norm1.bias"), M, C, C, C, EPS_BLOCK, mean=bs["m1"], rstd=bs["r1"])
        bs["xn1"] = xn1
        # q
        q = _empty((B, N, C), dt, dev)
        linear(xn1, self.w(p + "attn.q.weight"), q, bias=self.f32(p + "attn.q.bias"))
        bs["q"] = q
        # k, v source: spatially reduced image tokens (conv r x r stride r + LN 1e-5) followed by the text tokens
        if r > 1:
            HWr = (gh // r) * (gw // r)
            Mk = HWr + T
            pm = patchmap(r, gw, N, HWr, gw // r, C)
            sr_pre = _empty((B * HWr, C), dt, dev)
            linear(xn1, self.wK(p + "attn.sr.weight"), sr_pre, B * HWr, a_map=pm, bias=self.f32(p + "attn.sr.bias"))
            kvin = _empty((B * HWr, C), dt, dev)
            bs["msr"], bs["rsr"] = _empty((B * HWr,), f32, dev), _empty((B * HWr,), f32, dev)
            ops.layernorm_fwd(sr_pre, kvin, self.f32(p + "attn.norm.weight"), self.f32(p + "attn.norm.bias"), B * HWr, C, C, C,
                              EPS_DEFAULT, mean=bs["msr"], rstd=bs["rsr"])
            kv = _empty((B, Mk, 2 * C), dt, dev)
            wkv, bkv = self.w(p + "attn.kv.weight"), self.f32(p + "attn.kv.bias")
            linear(kvin, wkv, kv, c_map=rowmap(HWr, Mk, 0), bias=bkv)
            linear(xn1, wkv, kv, B * T, a_map=rowmap(T, N, HW), c_map=rowmap(T, Mk, HWr), bias=bkv)
            bs.update(sr_pre=sr_pre, kvin=kvin, pm=pm, HWr=HWr)
        else:
            Mk = N
            kv = _empty((B, Mk, 2 * C), dt, dev)
            linear(xn1, self.w(p + "attn.kv.weight"), kv, bias=self.f32(p + "attn.kv.bias"))
        bs["kv"], bs["Mk"] = kv, Mk
        # attention core
        ao = _empty((B, N, C), dt, dev)
        lse = _empty((B, h, N), f32, dev)
        ops.sr_attention_fwd(q, kv, ao, lse, B, h, N, Mk, C, 2 * C, C, 0, C, 64 ** -0.5)
        bs["ao"], bs["lse"] = ao, lse
        # proj + DropPath + residual
        xm = _empty((B, N, C), self.rt, dev)
        xn2 = _empty((B, N, C), dt, dev)
        bs["m2"], bs["r2"] = _empty((M,), f32, dev), _empty((M,), f32, dev)
        bs["xn2"] = xn2
        bs["fused_mlp"] = fused = (dt == torch.bfloat16 and C in (64, 128))
        # stages 1-2 (one tile of the projection holds whole rows): Block.norm2 rides on the projection's epilogue -- the fused MLP then reads
        # its operand in bf16 and the fp32 mid stream only once (as the residual), instead of normalising the fp32 rows itself
        proj_ln = fused and M < (1 << 24)      # (the lean GEMM epilogues index rows in 24 bits)
        linear(ao, self.w(p + "attn.proj.weight"), xm, bias=self.f32(p + "attn.proj.bias"),
               row_scale=s1, rows_per_scale=N, R=x,
               post_ln=(self.f32(p + "norm2.weight"), self.f32(p + "norm2.bias"), EPS_BLOCK, xn2.view(M, C), bs["m2"], bs["r2"]) if proj_ln else None)
        bs["xm"] = xm
        # LN2 + MLP (fc1 + exact GELU, fc2) + DropPath + residual
        # the last block of a stage has no fp32 consumer (its output feeds the next stage's patch embedding and the heads, which read
        # the MFMA-operand copy): the fused MLP then writes that copy itself and no fp32 stream -- no separate cast pass
        last_op = fused and j == m.depths[i] - 1 and self.dt != self.rt
        # stages 3-4: the same through fc2's residual epilogue (bf16 C beside the fp32 residual, mvlt_gemm_nt_args.r_fp32)
        # (r_fp32 exists in the lean residual epilogue only: rows indexed in 24 bits, 16-byte row pieces -- otherwise the fp32 output + cast pass below)
        last_gemm = ((not fused) and j == m.depths[i] - 1 and dt == torch.bfloat16 and self.rt == torch.float32 and
                     M < (1 << 24) and C % 8 == 0)
        xo = _empty((B, N, C), dt if (last_op or last_gemm) else self.rt, dev)
        if fused:
            # stages 1-2: LN2 -> fc1 -> GELU -> fc2 -> DropPath -> +residual in ONE kernel.  The (tokens x hidden) activation stays on
            # chip and is recomputed by the fused backward kernels; LN2 is folded into the operand load (the kernel reads the fp32
            # mid stream once for both the normalisation and the residual, and stores LN2's output + statistics for the backward)
            ln = None if proj_ln else (self.f32(p + "norm2.weight"), self.f32(p + "norm2.bias"), EPS_BLOCK, xn2, bs["m2"], bs["r2"])
            post = None
            if j + 1 < m.depths[i]:
                # the next block's norm1 rides on this kernel's epilogue (the output row is in registers there)
                pn = f"block{i+1}.{j+1}."
                self._pre_ln1 = (_empty((B, N, C), dt, dev), _empty((M,), f32, dev), _empty((M,), f32, dev))
                post = (self.f32(pn + "norm1.weight"), self.f32(pn + "norm1.bias"), EPS_BLOCK, *self._pre_ln1)
            ops.mlp_fwd(None if ln else xn2, self.w(p + "mlp.fc1.weight"), self.f32(p + "mlp.fc1.bias"), self.w(p + "mlp.fc2.weight"),
                        self.f32(p + "mlp.fc2.bias"), xm, None if last_op else xo, M, C, hid, row_scale=s2, rows_per_scale=N, ln=ln,
                        out_op=xo if last_op else None, post_ln=post)
        else:
            ops.layernorm_fwd(xm, xn2, self.f32(p + "norm2.weight"), self.f32(p + "norm2.bias"), M, C, C, C, EPS_BLOCK, mean=bs["m2"], rstd=bs["r2"])
            hpre = _empty((M, hid), dt, dev) if keep else None
            gact = _empty((M, hid), dt, dev)
            linear(xn2, self.w(p + "mlp.fc1.weight"), gact, bias=self.f32(p + "mlp.fc1.bias"), act=1, H=hpre)
            bs["hpre"], bs["gact"] = hpre, gact
            linear(gact, self.w(p + "mlp.fc2.weight"), xo, bias=self.f32(p + "mlp.fc2.bias"), row_scale=s2, rows_per_scale=N, R=xm)
        if not keep:
            bs.clear()
        return xo, bs

    # ------------------------------------------------------------------ backward
    def _scaled(self, dy, scale, N):
        """dy * scale[b] per sample (DropPath); identity when scale is None."""
        if scale is None:
            return dy
        out = torch.empty_like(dy)
        ops.row_scale(dy, scale, N, self.B * N, dy.shape[-1], out)
        return out

    def backward(self, dxs):
        """dxs: gradients w.r.t. the four stage outputs (None allowed).  Fills the flat gradient buffer."""
        m, B, T, dt, dev, S = self.m, self.B, self.T, self.dt, self.dev, self.S
        self._pos_adj = []
        # gradient tensors the head nodes of this pass created themselves (the heads' shared buffer, the MIM decoder's outputs) may be
        # written in place; anything else autograd hands us is copied first
        own = [d is not None and d.dtype == dt and d.is_contiguous() and S.owns(d) for d in dxs]
        dx, merged = None, False
        for i in (3, 2, 1, 0):
            if not plan_unit(self, f"block{i+1}.{m.depths[i] - 1}").save:
                break                      # the plan's cut lies above this stage: nothing from here on has a trainable parameter
            sv = self.saved[i]
            d_out = dxs[i]
            if d_out is not None and not merged:
                d_out = d_out.to(dt)
                if dx is None:
                    dx = d_out if own[i] else d_out.contiguous().clone()
                else:
                    dx.add_(d_out)
            if dx is None:
                continue
            # the stage's input gradient is accumulated straight into the previous stage's own head gradient where there is one
            into = dxs[i - 1] if i > 0 and own[i - 1] else None
            dx = self._stage_backward(i, sv, dx.view(B, sv["N"], sv["C"]), into)
            merged = into is not None and dx is not None
            if plan_unit(self, f"embed{i+1}").save:      # (a stage the cut ends half-way travels with the leftovers at the end of the pass)
                self.S.announce_stage(i)
        # the learned position embeddings (root parameters: they sit in front of the stage blocks in the flat layout) got their last
        # contribution from stage 1's backward: final now, so that only the BERT embedding block is left for the end of the pass
        if self._pos_adj:
            ops.resize_bilinear_tokens_multi(self._pos_adj, adjoint=True)
            self._pos_adj = []
        self.S.announce_prefix("pos_embed", "text_pos_embed")
        self.S.fold_copies()
        self.saved = []

    def _stage_backward(self, i, sv, dx, into=None):
        m, B, T, dt, dev = self.m, self.B, self.T, self.dt, self.dev
        C, HW, N = sv["C"], sv["HW"], sv["N"]
        self._mark()
        for j in reversed(range(m.depths[i])):
            if not plan_unit(self, f"block{i+1}.{j}").save:        # behind the cut
                self._mark()
                return None
            dx = self._block_backward(i, j, sv["blocks"][j], dx)
        self._mark()
        u = plan_unit(self, f"embed{i+1}")
        if not u.save:
            return None
        on = u.launches
        pe, ten = f"patch_embed{i+1}.", f"text_embed{i+1}."
        f32 = torch.float32
        # pos-embed / text-pos-embed gradients: sum over the batch of d(x0)
        if on["pos"]:
            dpos_all = _empty((N, C), f32, dev)
            ops.batch_sum(dx, dpos_all, B, N, C, N, C, acc2=self.g(f"text_pos_embed{i+1}")[0], split=HW)        # text rows straight into G
            self._pos_backward(i, dpos_all[:HW])
        if not u.dgrad and u.only("pos"):            # the cut, with the two position embeddings the only trainable tensors: the rest of the unit is dropped
            return None
        # patch-embed LN backward -> d(pe_pre)
        d_pe = _empty((B * HW, C), dt, dev)
        ops.layernorm_bwd(dx, sv["pe_pre"], d_pe, self.f32(pe + "norm.weight"), sv["pe_mean"], sv["pe_rstd"], B * HW, C, C, C, C,
                          dgamma=self.gl(pe + "norm.weight"), dbeta=self.gl(pe + "norm.bias"), **self.lnk(), dy_map=rowmap(HW, N, 0))
        d_te = _empty((B * T, C), dt, dev)
        ops.layernorm_bwd(dx, sv["te_pre"], d_te, self.f32(ten + "1.weight"), sv["te_mean"], sv["te_rstd"], B * T, C, C, C, C,
                          dgamma=self.gl(ten + "1.weight"), dbeta=self.gl(ten + "1.bias"), **self.lnk(), dy_map=rowmap(T, N, HW))
        if i == 0:
            linear_bwd(on["patch"], d_pe, sv["P1"], self.g(pe + "proj.weight"), self.g(pe + "proj.bias"))
            # (round 6: the text-embedding weight gradients leave as partial tiles too -- 64 x 768 over 32768 rows: 64 splits' atomics on 1536 cache lines were 56 us)
            d_emb = _empty((B * T, m.hidden), dt, dev) if u.dgrad else None      # (= some tensor of the BERT embedding block is trainable: it is the only unit below)
            linear_bwd(on["text"], d_te, self.emb, self.g(ten + "0.weight"), self.g(ten + "0.bias"), self.wT(ten + "0.weight"), d_emb, tn=self.S)
            if u.dgrad:
                self._bert_backward(d_emb)
            return None
        Cp, Np, HWp = m.dims[i - 1], self.saved[i - 1]["N"], self.saved[i - 1]["HW"]
        xp = sv["x_in_prev"]
        pm = sv["pm_in"]
        # conv weight gradient: computed in the gather's [out][kh][kw][cin] order, accumulated at its [out][cin][kh][kw] place
        if on["patch"]:
            layers.conv_wgrad(self.S, pe + "proj.weight", d_pe, xp, pm, colsum=self.g(pe + "proj.bias"))
        linear_bwd(on["text"], d_te, xp, self.g(ten + "0.weight"), self.g(ten + "0.bias"), x_map=rowmap(T, Np, HWp), tn=self.S)
        if not u.dgrad:
            return None
        dxp = into.view(B, Np, Cp) if into is not None else _empty((B, Np, Cp), dt, dev)
        linear(d_pe, self.wKT(pe + "proj.weight"), dxp, c_map=pm, R=into)                       # image rows (each once)
        linear(d_te, self.wT(ten + "0.weight"), dxp, c_map=rowmap(T, Np, HWp), R=into)          # text rows
        return dxp

    def _pos_backward(self, i, dpos):
        m = self.m
        h, w = self.grid[i]
        HW = h * w
        gv = self.g(f"pos_embed{i+1}")
        gv = (gv[:, 1:] if i == 3 else gv)[0]
        if HW == m.grids[0] ** 2:
            gv.add_(dpos)
            return
        # the adjoints of all stages leave in one launch at the end of the trunk's backward (`backward`): dpos stays alive in the list until then
        self._pos_adj.append((dpos, gv, m.grids[i], m.grids[i], h, w, dpos.shape[1]))

    def _bert_backward(self, d_emb):
        m, B, T = self.m, self.B, self.T
        te = "text_embeddings."
        ops.bert_embed_bwd(d_emb, self.ids, self.f32(te + "word_embeddings.weight"), self.f32(te + "position_embeddings.weight"),
                           self.f32(te + "token_type_embeddings.weight"), self.f32(te + "LayerNorm.weight"), self.keep, BERT_DROP,
                           self.emb_mean, self.emb_rstd, self.g(te + "word_embeddings.weight"), self.g(te + "position_embeddings.weight"),
                           self.g(te + "token_type_embeddings.weight"), self.g(te + "LayerNorm.weight"), self.g(te + "LayerNorm.bias"),
                           B * T, T)

    def _block_backward(self, i, j, bs, dx):
        """dx: gradient w.r.t. the block output (B,N,C), overwritten in place with the gradient w.r.t. its input."""
        m, B, T, dt, dev = self.m, self.B, self.T, self.dt, self.dev
        C, h, r, hid = m.dims[i], m.heads[i], m.sr[i], m.hid[i]
        HW = self.grid[i][0] * self.grid[i][1]
        N = HW + T
        M = B * N
        p = f"block{i+1}.{j}."
        f32 = torch.float32
        u = plan_unit(self, f"block{i+1}.{j}")
        on = u.launches
        # the plan's cut with only MLP weights / biases trainable in this block: their gradients need d(block output) alone -- the pass ends here
        mlp_only = not u.dgrad and u.only("fc1", "fc2")
        # ---- MLP branch: x_out = x_mid + s2 * (fc2(gelu(fc1(LN2(x_mid)))))
        dxn2 = _empty((M, C), dt, dev)
        # the DropPath-scaled copy of d(x_mid), the gradient of the attention branch x_mid = x + s1 * proj(attn(LN1(x))), comes out of norm2's backward
        fuse = bs["s1"] is not None
        if bs["fused_mlp"]:
            w1, w2t = self.w(p + "mlp.fc1.weight"), self.wT(p + "mlp.fc2.weight")
            if on["fc1"] or on["fc2"]:
                ops.mlp_bwd_dw(bs["xn2"], dx, w1, w2t, self.f32(p + "mlp.fc1.bias"), self.g(p + "mlp.fc1.weight"), self.g(p + "mlp.fc1.bias"),
                               self.g(p + "mlp.fc2.weight"), self.g(p + "mlp.fc2.bias"), M, C, hid, row_scale=bs["s2"], rows_per_scale=N,
                               partials=self.S.tn_partials(), defer_fold=True)
            if mlp_only:
                bs.clear()
                return dx
            # ... and norm2's backward rides on the dx kernel's epilogue (the row of d(LN output) is in registers there): dx is
            # updated in place, the DropPath-scaled copy for the attention branch comes out of the same pass, no dxn2 round trip
            dy1 = _empty((M, C), dx.dtype, dev) if fuse else dx
            ops.mlp_bwd_dx(bs["xn2"], dx, w1, self.wT(p + "mlp.fc1.weight"), w2t, self.f32(p + "mlp.fc1.bias"), None, M, C, hid,
                           row_scale=bs["s2"], rows_per_scale=N,
                           ln_bwd=dict(x=bs["xm"], mean=bs["m2"], rstd=bs["r2"], gamma=self.f32(p + "norm2.weight"), dx=dx,
                                       dgamma=self.gl(p + "norm2.weight"), dbeta=self.gl(p + "norm2.bias"),
                                       dx2=dy1 if fuse else None, dx2_scale=bs["s1"], dx2_rows_per_scale=N))
        else:
            dy2 = getattr(self, "_dy2_pre", None)                # written by the block above's norm1 backward when there is one
            self._dy2_pre = None
            if dy2 is None:
                dy2 = self._scaled(dx, bs["s2"], N)
            fc2_only = mlp_only and not on["fc1"]
            dh = None if fc2_only else _empty((M, hid), dt, dev)
            linear_bwd(on["fc2"], dy2, bs["gact"], self.g(p + "mlp.fc2.weight"), self.g(p + "mlp.fc2.bias"), self.wT(p + "mlp.fc2.weight"), dh, tn=self.S, act=2, H=bs["hpre"])
            if fc2_only:
                bs.clear()
                return dx
            bs["gact"] = bs["hpre"] = None
            linear_bwd(on["fc1"], dh, bs["xn2"], self.g(p + "mlp.fc1.weight"), self.g(p + "mlp.fc1.bias"), self.wT(p + "mlp.fc1.weight"),
                       None if mlp_only else dxn2, tn=self.S)
            if mlp_only:
                bs.clear()
                return dx
            del dh
            # dx += LN2 backward = d(x_mid); the same kernel writes its DropPath-scaled copy
            dy1 = _empty((M, C), dx.dtype, dev) if fuse else dx
            ops.layernorm_bwd(dxn2, bs["xm"], dx, self.f32(p + "norm2.weight"), bs["m2"], bs["r2"], M, C, C, C, C,
                              dgamma=self.gl(p + "norm2.weight"), dbeta=self.gl(p + "norm2.bias"), **self.lnk(), accumulate=True,
                              dx2=dy1 if fuse else None, dx2_scale=bs["s1"], dx2_rows_per_scale=N, lddx2=C)
        # stages 1-2 (C = 64 / 128, HBM-bound): the weight gradient and the input gradient of a C x C Linear come out of ONE pass over dY
        lin_fuse = dt == torch.bfloat16 and C in (64, 128)
        dao = dxn2          # reuse
        # (a frozen weight + bias: no weight gradient, and the fused launch gives way to the plain input-gradient GEMM of stages 3-4)
        # (stages 3-4: 9-16 output tiles x 32-56 m-splits -- reduced through bf16 partial tiles + a fold instead of atomics: mvlt_gemm_tn_args.partials)
        linear_bwd(on["proj"], dy1, bs["ao"], self.g(p + "attn.proj.weight"), self.g(p + "attn.proj.bias"), self.wT(p + "attn.proj.weight"), dao, fuse=lin_fuse, tn=self.S)
        Mk = bs["Mk"]
        dq = _empty((B, N, C), dt, dev)
        # dK/dV: one query chunk per (batch, head) from B*heads >= 512 on (mvlt_sr_attention_bwd then stores plainly, every
        # element once); only the split case accumulates with atomics and needs the zero fill
        if dt == torch.bfloat16 and ops.sr_attention_bwd_chunks(B, h, N, Mk, dt) == 1:      # (every 256-px stage with B * heads >= 512; round 6: pvlt_medium's stage 3 at batch 64)
            dkv = _empty((B, Mk, 2 * C), dt, dev)              # written once, in the operand dtype
            ops.sr_attention_bwd(bs["q"], bs["kv"], bs["ao"], dao, bs["lse"], dq, dkv, B, h, N, Mk, C, 2 * C, C, 2 * C, 0, C, 64 ** -0.5)
        else:
            dkv32 = pool_zeros((B, Mk, 2 * C), f32, dev)
            ops.sr_attention_bwd(bs["q"], bs["kv"], bs["ao"], dao, bs["lse"], dq, dkv32, B, h, N, Mk, C, 2 * C, C, 2 * C, 0, C, 64 ** -0.5)
            dkv = dkv32.to(dt)
            del dkv32
        # q projection
        dxn1 = dao          # reuse again: d(LN1 output), every row written by the q dgrad
        linear_bwd(on["q"], dq, bs["xn1"], self.g(p + "attn.q.weight"), self.g(p + "attn.q.bias"), self.wT(p + "attn.q.weight"), dxn1, fuse=lin_fuse, tn=self.S)
        gkvw, gkvb = self.g(p + "attn.kv.weight"), self.g(p + "attn.kv.bias")
        wkvT = self.wT(p + "attn.kv.weight")
        if r > 1:
            HWr, pm = bs["HWr"], bs["pm"]
            # text keys come straight from LN1(x)[text rows]
            linear_bwd(on["kv"], dkv, bs["xn1"], gkvw, gkvb, wkvT, dxn1, B * T, tn=self.S, dy_map=rowmap(T, Mk, HWr), x_map=rowmap(T, N, HW),
                       dx_map=rowmap(T, N, HW), R=dxn1)
            # image keys: kv <- LN(sr conv(LN1(x)[image rows]))
            dkvin = _empty((B * HWr, C), dt, dev)
            linear_bwd(on["kv"], dkv, bs["kvin"], gkvw, gkvb, wkvT, dkvin, B * HWr, tn=self.S, dy_map=rowmap(HWr, Mk, 0))
            dsr = _empty((B * HWr, C), dt, dev)
            ops.layernorm_bwd(dkvin, bs["sr_pre"], dsr, self.f32(p + "attn.norm.weight"), bs["msr"], bs["rsr"], B * HWr, C, C, C, C,
                              dgamma=self.gl(p + "attn.norm.weight"), dbeta=self.gl(p + "attn.norm.bias"), **self.lnk())
            if on["sr"]:
                layers.conv_wgrad(self.S, p + "attn.sr.weight", dsr, bs["xn1"], pm, colsum=self.g(p + "attn.sr.bias"))
            linear(dsr, self.wKT(p + "attn.sr.weight"), dxn1, c_map=pm, R=dxn1)
        else:
            linear_bwd(on["kv"], dkv, bs["xn1"], gkvw, gkvb, wkvT, dxn1, tn=self.S, R=dxn1)
        # the block below (processed next) scales this gradient by its own MLP-branch DropPath factor first thing when its MLP is not the
        # fused kernel (stages 3-4): norm1's backward writes that scaled copy in the same pass
        prev = self.saved[i]["blocks"][j - 1] if j > 0 else None
        pre = prev is not None and not prev.get("fused_mlp", True) and prev.get("s2") is not None
        self._dy2_pre = _empty((M, C), dx.dtype, dev) if pre else None
        ops.layernorm_bwd(dxn1, bs["x"], dx, self.f32(p + "norm1.weight"), bs["m1"], bs["r1"], M, C, C, C, C,
                          dgamma=self.gl(p + "norm1.weight"), dbeta=self.gl(p + "norm1.bias"), **self.lnk(), accumulate=True,
                          dx2=self._dy2_pre, dx2_scale=prev["s2"] if pre else None, dx2_rows_per_scale=N if pre else 0, lddx2=C if pre else 0)
        bs.clear()
        return dx


class _TrunkFn(torch.autograd.Function):
    """The trunk as ONE autograd node.  Every parameter of the HIP-scheduled part of the model (trunk AND heads) is an
    input of this node: its backward runs after all head nodes, so it can hand autograd the finished slices of the flat
    gradient buffer.  That keeps stock torch machinery working unchanged on top of the side-effect gradient writes:
    AccumulateGrad (and therefore torch DistributedDataParallel's reducer hooks, reference main_vl.py:301), GradScaler,
    clip_grad_norm_ and torch.optim all see ordinary .grad tensors -- which alias the flat buffer, no copies."""

    @staticmethod
    def forward(ctx, model, images, ids, need_grad, *params):
        step = TrunkStep(model, images, ids, need_grad, getattr(model, "_plan", None))
        # the node's outputs are tensor objects of their own (same storage): the step keeps the stage buffers it wrote, and an output that the node's own context
        # holds closes a reference cycle through its grad_fn -- a forward whose graph is dropped without a backward (or whose backward raised) then keeps its
        # activations and its ZeroPool token alive, and every later step finds a forward "pending" (docs/accumulation.md)
        outs = [o.detach() for o in step.forward()]
        ctx.step = step
        ctx.pool_token, model._pool_token = model._pool_token, None      # this node's life = the time the step's pooled scratch is owned
        ctx.set_materialize_grads(False)          # unused stage outputs send None, not a zero tensor of their size (138 MB at stage 1)
        ctx.mark_non_differentiable(outs[0])
        return tuple(outs)

    @staticmethod
    def backward(ctx, d1, d2, d3, d4):
        step = saved(ctx.step)
        S = step.S
        S.queue_finalize()
        step.backward([None, d2, d3, d4])
        ctx.step = None
        ctx.pool_token = None
        return (None, None, None, None, *_grad_slices(S, ctx, 4))


def _grad_slices(S, ctx, first):
    """what a parameter-carrying node returns to autograd: the finished slices of the flat gradient buffer (see _TrunkFn)"""
    grads = []
    for k, (name, p) in enumerate(S.fn_params):
        gv = S.grad(name)
        if not ctx.needs_input_grad[first + k]:
            grads.append(None)          # frozen: .grad stays None
        elif p.grad is not None and p.grad.data_ptr() == gv.data_ptr():
            grads.append(None)          # .grad already aliases the flat buffer (accumulation without zero_grad)
        else:
            grads.append(gv)
    return grads


class _FrozenTrunkFn(torch.autograd.Function):
    """Stands where _TrunkFn stands when no trunk unit has a trainable parameter (a linear probe: only heads train).  The trunk has then run outside
    autograd, exactly as under torch.no_grad() -- nothing saved, no trunk node; this node only ties the stage outputs the heads read to the parameters,
    so that the head nodes get their backward and, after all of them, the trainable parameters get their slices of the flat gradient buffer."""

    @staticmethod
    def forward(ctx, model, x2, x3, x4, *params):
        ctx.S = model.store
        ctx.pool_token, model._pool_token = model._pool_token, None
        ctx.set_materialize_grads(False)
        return x2.detach(), x3.detach(), x4.detach()

    @staticmethod
    def backward(ctx, d2, d3, d4):
        S = ctx.S
        S.queue_finalize()
        ctx.pool_token = None
        S.fold_copies()
        return (None, None, None, None, *_grad_slices(S, ctx, 4))


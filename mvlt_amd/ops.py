"""Thin Python calls over the C ABI (include/mvlt_hip.h and the additions beside it).  Every function launches HIP kernels asynchronously on
torch's current stream; tensors are only used as device buffers.  No fallbacks: a missing library or a CPU tensor
raises (mvlt_amd/_lib.py)."""
import ctypes as C

import torch

from . import _lib as L
from ._lib import DT, check, patchmap, ptr, rowmap, stream_ptr

_ID = rowmap()


def _gemm_nt_args(A, B, C_out, M, N, K, lda, ldb, ldc, *, a_map=None, c_map=None, bias=None, act=0, H=None,
                  row_scale=None, rows_per_scale=0, R=None, col_sum=None, col_sumsq=None, col_copies=0, split_k=0, post_ln=None):
    """the mvlt_gemm_nt_args of a gemm_nt / gemm_nt_plan call"""
    assert A.dtype == B.dtype and A.dtype in DT and (C_out.dtype in DT or (C_out.dtype == torch.float16 and col_sum is not None))
    if bias is not None:
        assert bias.dtype == torch.float32
    if row_scale is not None:
        assert row_scale.dtype == torch.float32
    if R is not None:
        assert R.dtype == C_out.dtype or (R.dtype == torch.float32 and C_out.dtype == torch.bfloat16)       # (the second: mvlt_gemm_nt_args.r_fp32)
    if H is not None:
        assert H.dtype == C_out.dtype
    if col_sum is not None:
        assert col_sum.dtype == torch.float32 and col_sumsq is not None and col_sumsq.dtype == torch.float32
    a = L.GemmNTArgs(A=ptr(A), B=ptr(B), C=ptr(C_out), M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc,
                     dtype=DT[A.dtype], out_dtype=2 if C_out.dtype == torch.float16 else DT[C_out.dtype], a_map=a_map or _ID, c_map=c_map or _ID,
                     bias=ptr(bias), act=act, H=ptr(H), row_scale=ptr(row_scale), rows_per_scale=rows_per_scale, R=ptr(R),
                     col_sum=ptr(col_sum), col_sumsq=ptr(col_sumsq), col_copies=col_copies, split_k=split_k)
    if R is not None and R.dtype != C_out.dtype:
        a.r_fp32 = 1
    if post_ln is not None:
        g, b, eps, y, mean, rstd = post_ln
        assert g.dtype == b.dtype == mean.dtype == rstd.dtype == torch.float32 and y.dtype == torch.bfloat16 and y.is_contiguous()
        a.post_y, a.post_ld, a.post_gamma, a.post_beta, a.post_eps, a.post_mean, a.post_rstd = ptr(y), y.shape[-1], ptr(g), ptr(b), eps, ptr(mean), ptr(rstd)
    return a


def gemm_nt(A, B, C_out, *dims, **kw):
    """gemm_nt(A, B, C_out, M, N, K, lda, ldb, ldc, *, a_map, c_map, bias, act, H, row_scale, rows_per_scale, R, col_sum, col_sumsq, col_copies, split_k, post_ln):
    C[M,N] = epi(A[M,K] @ B[N,K]^T); see mvlt_gemm_nt in include/mvlt_hip.h.  post_ln = (gamma, beta, eps, y, mean, rstd): LayerNorm of the
    finished output rows rides on the epilogue (N == 64 / 128, bf16 operands, R given)."""
    check(L.lib.mvlt_gemm_nt(C.byref(_gemm_nt_args(A, B, C_out, *dims, **kw)), stream_ptr()), "mvlt_gemm_nt")
    return C_out


class Plan:
    """what a GEMM, attention or fused-MLP call would launch (mvlt_gemm_plan / mvlt_attn_plan / mvlt_mlp_plan of include/mvlt_hip_plan.h): .name is the kernel as _lib.last_kernel() prints it, .p the struct"""

    def __init__(self, plan_fn, args, cls=None, name_fn=None):
        p, buf = (cls or L.GemmPlan)(), C.create_string_buffer(256)
        check(plan_fn(C.byref(args), C.byref(p)), "plan")
        check(min((name_fn or L.lib.mvlt_gemm_plan_name)(C.byref(p), buf, len(buf)), 0), "plan name")
        self.p, self.name = p, buf.value.decode()

    def __getattr__(self, field):
        v = getattr(self.p, field)
        return v if isinstance(v, int) else list(v)


def gemm_nt_plan(*args, **kw):
    """same arguments as gemm_nt; nothing is launched and no device is touched"""
    return Plan(L.lib.mvlt_gemm_nt_plan, _gemm_nt_args(*args, **kw))


def gemm_tn_plan(*args, **kw):
    """same arguments as gemm_tn; nothing is launched and no device is touched"""
    return Plan(L.lib.mvlt_gemm_tn_plan, _gemm_tn_args(*args, **kw))


def tn_fold_flush(partials=None):
    """fold the partial-tile reductions that gemm_tn(partials=..., defer_fold=True) left pending in that scratch (None: in every scratch): one launch per scratch on the
    producers' stream, which the current stream waits for if it is another one; none pending: none"""
    check(L.lib.mvlt_tn_fold_flush(ptr(partials), stream_ptr()), "mvlt_tn_fold_flush")


def tn_fold_discard(partials=None):
    """drop the pending deferred folds of that scratch (None: all) without running them (the start of a backward pass: whatever its store has pending then belongs to a
    pass that was abandoned)"""
    check(L.lib.mvlt_tn_fold_discard(ptr(partials)), "mvlt_tn_fold_discard")


def weight_prep(desc_dev, blk_dev, ndesc, total_blocks, dtype, blk_desc=None):
    """desc_dev: uint8 device tensor holding ndesc packed mvlt_prep_desc; blk_dev: int32 device tensor [ndesc + 1]."""
    check(L.lib.mvlt_weight_prep(ptr(desc_dev), ptr(blk_dev), ndesc, total_blocks, ptr(blk_desc), DT[dtype], stream_ptr()), "mvlt_weight_prep")


def gemm_tn(A, B, C_out, *dims, **kw):
    """gemm_tn(A, B, C_out, M, N1, N2, lda, ldb, ldc, *, a_map, b_map, colsum, splits, taps, seg, dgrad, partials, defer_fold, overwrite):
    C[N1,N2] += A[M,N1]^T @ B[M,N2] (fp32 atomics); colsum[N1] += A.sum(0).  taps > 1: logical column tap*seg + c is
    accumulated at column c*taps + tap (conv weight gradients straight into the [out][cin][kh][kw] layout).
    dgrad = (W^T [N2][N1] bf16, out [M, N2] bf16): the Linear's input gradient out = A @ W from the same pass over A (N1 == N2 in {64, 128}).
    partials = a scratch tensor (the largest single launch of the model needs 37 MiB; deferring launches share it region by region: FlatStore holds 256 MiB): split reductions leave as bf16 partial tiles + an ordered fold instead of fp32 atomics where the
    library has that mode (mvlt_gemm_tn_args.partials in include/mvlt_hip.h: whole 256 x 256 tiles, >= 8 m-splits on the 128-wide kernel, conv3x3 weight gradients); deterministic."""
    check(L.lib.mvlt_gemm_tn(C.byref(_gemm_tn_args(A, B, C_out, *dims, **kw)), stream_ptr()), "mvlt_gemm_tn")
    return C_out


def _gemm_tn_args(A, B, C_out, M, N1, N2, lda, ldb, ldc, *, a_map=None, b_map=None, colsum=None, splits=0, taps=0, seg=0, dgrad=None, partials=None, defer_fold=False, overwrite=False):
    """the mvlt_gemm_tn_args of a gemm_tn / gemm_tn_plan call"""
    assert A.dtype == B.dtype and A.dtype in DT and C_out.dtype == torch.float32
    if colsum is not None:
        assert colsum.dtype == torch.float32
    a_map, b_map = a_map or _ID, b_map or _ID
    # the kernel's tile is 128 (N1 side) x 64/128 (N2 side): a narrow N1 gets the 64-wide side by computing C^T = B^T A and storing it transposed; the bias
    # gradient becomes the column sum of the (now) B operand.  (With a partial-tile scratch the 64 x 128 tile of the LDS-DMA kernel takes the shape as it is.)
    swap = dgrad is None and N1 <= 64 < N2 and b_map.mode == 0 and taps <= 1 and partials is None
    if swap:
        A, B, N1, N2, lda, ldb, a_map, b_map = B, A, N2, N1, ldb, lda, b_map, a_map
    a = L.GemmTNArgs(A=ptr(A), B=ptr(B), C=ptr(C_out), M=M, N1=N1, N2=N2, lda=lda, ldb=ldb, ldc=ldc, dtype=DT[A.dtype], a_map=a_map, b_map=b_map, splits=splits)
    if swap:
        a.colsum_b, a.trans_c = ptr(colsum), 1
    elif dgrad is not None:
        wt, dx = dgrad
        assert A.dtype == torch.bfloat16 and wt.dtype == dx.dtype == torch.bfloat16 and N1 == N2 and N1 in (64, 128) and taps <= 1
        assert wt.is_contiguous() and tuple(wt.shape) == (N2, N1) and dx.stride(-1) == 1
        # dx may be a row-strided view (a column slice of a wider buffer): its own row pitch goes to the kernel (N2 was passed);
        # the fused kernel walks plain rows on both operands
        dgrad_ld = dx.stride(-2) if dx.dim() >= 2 else N2
        assert dgrad_ld % 8 == 0 and dgrad_ld >= N2, dgrad_ld
        assert a_map.mode == 0 and a_map.rows_per_batch == 0 and b_map.mode == 0 and b_map.rows_per_batch == 0, "gemm_tn(dgrad=...): plain row maps only"
        a.colsum_a, a.dgrad_wt, a.dgrad_out, a.dgrad_ld = ptr(colsum), ptr(wt), ptr(dx), dgrad_ld
    else:
        a.colsum_a, a.c_taps, a.c_seg = ptr(colsum), taps, seg
        if partials is not None:       # scratch for the atomic-free reduction of whole 256 x 256 output tiles (mvlt_gemm_tn_args.partials); ignored for other shapes
            a.partials, a.partials_bytes = ptr(partials), partials.numel() * partials.element_size()
            a.defer_fold = 1 if defer_fold else 0       # the caller promises tn_fold_flush() before anything reads C_out
    if overwrite and dgrad is None:
        assert not a.trans_c and taps <= 1 and N2 % 4 == 0 and ldc % 4 == 0 and A.dtype == torch.bfloat16, "gemm_tn(overwrite=True): bf16, plain output layout, N2 and ldc multiples of 4"
        a.c_overwrite = 1                               # C_out holds zeros (the caller's word): one m-split, plain stores instead of atomics
    return a


LN_CHAIN_WIDTHS = (64, 128, 320, 512, 768)     # widths with a fixed-geometry forward kernel: these can chain a second LayerNorm


def layernorm_fwd(x, y, gamma, beta, rows, Cdim, ldx, ldy, eps, *, mean=None, rstd=None, add=None, add_rows=0,
                  x_map=None, y_map=None, chain=None):
    """chain = (gamma2, beta2, eps2, y2, mean2, rstd2): y2 (bf16, rows laid out like y) = LayerNorm(y) with the second parameter set,
    from the same pass; mean2 / rstd2 are indexed by y's physical row.  Only for Cdim in LN_CHAIN_WIDTHS."""
    assert x.dtype in DT and y.dtype in DT and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    a = L.LayerNormArgs(x=ptr(x), y=ptr(y), gamma=ptr(gamma), beta=ptr(beta), mean=ptr(mean), rstd=ptr(rstd), add=ptr(add), add_rows=add_rows,
                        rows=rows, C=Cdim, ldx=ldx, ldy=ldy, x_map=x_map or _ID, y_map=y_map or _ID, eps=eps, dtype=DT[x.dtype], y_dtype=DT[y.dtype])
    if chain is not None:
        g2, b2, eps2, y2, m2, r2 = chain
        assert Cdim in LN_CHAIN_WIDTHS and y2.dtype == torch.bfloat16 and g2.dtype == b2.dtype == m2.dtype == r2.dtype == torch.float32
        a.y2, a.gamma2, a.beta2, a.eps2, a.mean2, a.rstd2 = ptr(y2), ptr(g2), ptr(b2), eps2, ptr(m2), ptr(r2)
    check(L.lib.mvlt_layernorm_fwd(C.byref(a), stream_ptr()), "mvlt_layernorm_fwd")
    return y


def layernorm_bwd(dy, x, dx, gamma, mean, rstd, rows, Cdim, lddy, ldx, lddx, *, dgamma=None, dbeta=None,
                  dy_map=None, x_map=None, dx_map=None, accumulate=False, dx2=None, dx2_scale=None, dx2_rows_per_scale=0, lddx2=0,
                  copies=1, copy_stride=0):
    assert dy.dtype in DT and x.dtype in DT and dx.dtype in DT
    assert dx2 is None or (dx2.dtype == dy.dtype and dx2_scale is not None and dx2_scale.dtype == torch.float32 and dx2_rows_per_scale > 0)
    a = L.LayerNormBwdArgs(dy=ptr(dy), x=ptr(x), dx=ptr(dx), gamma=ptr(gamma), mean=ptr(mean), rstd=ptr(rstd), dgamma=ptr(dgamma), dbeta=ptr(dbeta),
                           rows=rows, C=Cdim, lddy=lddy, ldx=ldx, lddx=lddx, dy_map=dy_map or _ID, x_map=x_map or _ID, dx_map=dx_map or _ID,
                           dx_accumulate=1 if accumulate else 0, dtype=DT[dy.dtype], x_dtype=DT[x.dtype], dx_dtype=DT[dx.dtype],
                           dx2=ptr(dx2), dx2_scale=ptr(dx2_scale), dx2_rows_per_scale=dx2_rows_per_scale, lddx2=lddx2, dg_copies=copies, dg_copy_stride=copy_stride)
    check(L.lib.mvlt_layernorm_bwd(C.byref(a), stream_ptr()), "mvlt_layernorm_bwd")
    return dx


def fold_copies(arena, copies, stride, dst_index, j0, j1, dst):
    assert arena.dtype == torch.float32 and dst.dtype == torch.float32 and dst_index.dtype == torch.int32
    check(L.lib.mvlt_fold_copies(ptr(arena), copies, stride, ptr(dst_index), j0, j1, ptr(dst), stream_ptr()), "mvlt_fold_copies")


def batch_sum(x, out, B, R, Cdim, batch_stride_rows, ld, acc2=None, split=0):
    """out[r] = sum over the batch of x[b, r]; with acc2, rows r >= split are added to acc2[r - split] instead"""
    assert out.dtype == torch.float32 and (acc2 is None or (acc2.dtype == torch.float32 and acc2.is_contiguous()))
    check(L.lib.mvlt_batch_sum(ptr(x), ptr(out), B, R, Cdim, batch_stride_rows, ld, DT[x.dtype], ptr(acc2), split, stream_ptr()), "mvlt_batch_sum")
    return out


def _attention_fwd_args(Q, KV, O, lse, B, H, N, M, ldq, ldkv, ldo, k_off, v_off, scale):
    assert Q.dtype == KV.dtype == O.dtype and Q.dtype in DT
    return L.AttnArgs(Q=ptr(Q), KV=ptr(KV), O=ptr(O), lse=ptr(lse), B=B, H=H, N=N, M=M, ldq=ldq, ldkv=ldkv, ldo=ldo, k_off=k_off, v_off=v_off,
                      scale=scale, dtype=DT[Q.dtype])


def _attention_bwd_args(Q, KV, O, dO, lse, dQ, dKV, B, H, N, M, ldq, ldkv, ldo, lddkv, k_off, v_off, scale):
    assert dKV.dtype == torch.float32 or (dKV.dtype == torch.bfloat16 and Q.dtype == torch.bfloat16)
    return L.AttnBwdArgs(Q=ptr(Q), KV=ptr(KV), O=ptr(O), dO=ptr(dO), lse=ptr(lse), dQ=ptr(dQ), dKV=ptr(dKV), B=B, H=H, N=N, M=M,
                         ldq=ldq, ldkv=ldkv, ldo=ldo, lddkv=lddkv, k_off=k_off, v_off=v_off, scale=scale, dtype=DT[Q.dtype], dkv_dtype=DT[dKV.dtype])


def _attention_fwd(entry, *args):
    check(getattr(L.lib, entry)(C.byref(_attention_fwd_args(*args)), stream_ptr()), entry)
    return args[2]


def _attention_bwd(entry, *args):
    check(getattr(L.lib, entry)(C.byref(_attention_bwd_args(*args)), stream_ptr()), entry)
    return args[5], args[6]


def attention_plan(*args, streamed=False):
    """what sr_attention_fwd (14 arguments) / sr_attention_bwd (18 arguments) or, with streamed=True, their *_streamed forms would launch for the same arguments
    (mvlt_attn_plan of include/mvlt_hip_plan.h, .name as _lib.last_kernel() prints it); nothing is launched"""
    fwd = len(args) == 14
    a = (_attention_fwd_args if fwd else _attention_bwd_args)(*args)
    plan_fn = L.lib.mvlt_sr_attention_fwd_plan if fwd else L.lib.mvlt_sr_attention_bwd_plan
    return Plan(lambda args_ref, plan_ref: plan_fn(args_ref, int(streamed), plan_ref), a, L.AttnPlan, L.lib.mvlt_attn_plan_name)


def sr_attention_fwd(Q, KV, O, lse, B, H, N, M, ldq, ldkv, ldo, k_off, v_off, scale):
    return _attention_fwd("mvlt_sr_attention_fwd", Q, KV, O, lse, B, H, N, M, ldq, ldkv, ldo, k_off, v_off, scale)


def sr_attention_bwd_chunks(B, H, N, M, dtype):
    """query chunks per (batch, head) the backward would use with an fp32 dKV; 1: hand it a bf16 dKV instead (every element stored once: no zero fill, no cast)"""
    return int(L.lib.mvlt_sr_attention_bwd_chunks(B, H, N, M, DT[dtype]))


def sr_attention_bwd(Q, KV, O, dO, lse, dQ, dKV, B, H, N, M, ldq, ldkv, ldo, lddkv, k_off, v_off, scale):
    return _attention_bwd("mvlt_sr_attention_bwd", Q, KV, O, dO, lse, dQ, dKV, B, H, N, M, ldq, ldkv, ldo, lddkv, k_off, v_off, scale)


def sr_attention_fwd_streamed(Q, KV, O, lse, B, H, N, M, ldq, ldkv, ldo, k_off, v_off, scale):
    """sr_attention_fwd on the key-streamed kernel at any M (sr_attention_fwd takes it only past the LDS-resident range)"""
    return _attention_fwd("mvlt_sr_attention_fwd_streamed", Q, KV, O, lse, B, H, N, M, ldq, ldkv, ldo, k_off, v_off, scale)


def sr_attention_bwd_streamed(Q, KV, O, dO, lse, dQ, dKV, B, H, N, M, ldq, ldkv, ldo, lddkv, k_off, v_off, scale):
    """sr_attention_bwd on the key-streamed kernel at any M: chunks of 128 queries, fp32 atomics into a zeroed fp32 dKV when there are
    several; a bf16 dKV needs N <= 128"""
    return _attention_bwd("mvlt_sr_attention_bwd_streamed", Q, KV, O, dO, lse, dQ, dKV, B, H, N, M, ldq, ldkv, ldo, lddkv, k_off, v_off, scale)


# ------------------------------------------------------------------ helpers of csrc/elementwise.hip
def bert_embed_fwd(ids, word, pos, type0, gamma, beta, keep, drop_p, y, mean, rstd, rows, T, eps):
    assert ids.dtype == torch.int64 and (keep is None or keep.dtype == torch.uint8)
    check(L.lib.mvlt_bert_embed_fwd(ptr(ids), ptr(word), ptr(pos), ptr(type0), ptr(gamma), ptr(beta), ptr(keep), drop_p,
                                    ptr(y), ptr(mean), ptr(rstd), rows, T, word.shape[1], eps, DT[y.dtype], stream_ptr()),
          "mvlt_bert_embed_fwd")
    return y


def bert_embed_bwd(dy, ids, word, pos, type0, gamma, keep, drop_p, mean, rstd, dword, dpos, dtype0, dgamma, dbeta, rows, T):
    check(L.lib.mvlt_bert_embed_bwd(ptr(dy), ptr(ids), ptr(word), ptr(pos), ptr(type0), ptr(gamma), ptr(keep), drop_p,
                                    ptr(mean), ptr(rstd), ptr(dword), ptr(dpos), ptr(dtype0), ptr(dgamma), ptr(dbeta),
                                    rows, T, word.shape[1], DT[dy.dtype], stream_ptr()), "mvlt_bert_embed_bwd")


def head_grad_prep(dlogits, dl, db1, db2=None):
    """dl[B, n_pad] = dlogits[B, n] (zero padded, dl's dtype); db1 (and db2) += dlogits.sum(0)"""
    assert dlogits.dtype == torch.float32 and dlogits.is_contiguous() and dl.is_contiguous() and dl.dtype in DT and db1.dtype == torch.float32
    B, n = dlogits.shape
    check(L.lib.mvlt_head_grad_prep(ptr(dlogits), B, n, dl.shape[1], ptr(dl), ptr(db1), ptr(db2), DT[dl.dtype], stream_ptr()), "mvlt_head_grad_prep")


def patchify(img, out, B, Cin, H, W, k):
    assert img.dtype == torch.float32 and img.is_contiguous()
    check(L.lib.mvlt_patchify(ptr(img), ptr(out), B, Cin, H, W, k, DT[out.dtype], stream_ptr()), "mvlt_patchify")
    return out


def masked_select(labels, idx, count, ignore_index=-1):
    assert labels.dtype == torch.int64 and idx.dtype == torch.int32 and count.dtype == torch.int32 and labels.is_contiguous()
    check(L.lib.mvlt_masked_select(ptr(labels), labels.numel(), ignore_index, ptr(idx), ptr(count), stream_ptr()), "mvlt_masked_select")


def gather_rows(src, idx, dst, rows, Cdim, ld_src, src_map=None):
    assert idx.dtype == torch.int32 and src.dtype == dst.dtype
    m = C.byref(src_map) if src_map is not None else None
    check(L.lib.mvlt_gather_rows(ptr(src), ptr(idx), ptr(dst), rows, Cdim, ld_src, m, DT[src.dtype], stream_ptr()), "mvlt_gather_rows")
    return dst


def scatter_rows(src, idx, dst, rows, Cdim, ld_dst, dst_map=None, accumulate=False):
    assert idx.dtype == torch.int32 and src.dtype == dst.dtype
    m = C.byref(dst_map) if dst_map is not None else None
    check(L.lib.mvlt_scatter_rows(ptr(src), ptr(idx), ptr(dst), rows, Cdim, ld_dst, m, 1 if accumulate else 0, DT[src.dtype], stream_ptr()),
          "mvlt_scatter_rows")
    return dst


def cross_entropy_fwd(logits, labels, lse, loss_sum, count, rows, V, ld, ignore_index=-1):
    assert labels.dtype == torch.int64
    check(L.lib.mvlt_cross_entropy_fwd(ptr(logits), ptr(labels), ignore_index, ptr(lse), ptr(loss_sum), ptr(count), rows, V, ld,
                                       DT[logits.dtype], stream_ptr()), "mvlt_cross_entropy_fwd")


def cross_entropy_bwd(logits, labels, lse, gscale, count, dlogits, rows, V, ld, ldd, ignore_index=-1):
    check(L.lib.mvlt_cross_entropy_bwd(ptr(logits), ptr(labels), ignore_index, ptr(lse), ptr(gscale), ptr(count), ptr(dlogits), rows, V, ld, ldd,
                                       DT[logits.dtype], DT[dlogits.dtype], stream_ptr()), "mvlt_cross_entropy_bwd")


def _ce_smooth_ok(logits, labels, weight, rows, V, ld, label_smoothing):
    assert logits.dtype in DT and logits.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous()       # (a dtype but fp32: the entry point refuses it)
    assert labels.numel() >= rows and (rows <= 0 or logits.numel() >= (rows - 1) * ld + V)
    assert weight is None or (weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() >= V)
    return float(label_smoothing)


def ce_smooth_fwd(logits, labels, lse, smooth, acc, rows, V, ld, *, ignore_index=-1, label_smoothing=0.0, weight=None):
    """F.cross_entropy(logits, labels, weight=weight, ignore_index=..., label_smoothing=...) over the rows of an fp32 matrix (include/mvlt_hip_loss.h): lse[r],
    smooth[r] = W lse_r - sum_c w_c x[r, c] (written for label_smoothing > 0 only) and acc = [numerator, den, W] by plain stores -- the mean is acc[0] / acc[1].
    weight: fp32 [V] or None."""
    e = _ce_smooth_ok(logits, labels, weight, rows, V, ld, label_smoothing)
    for t, n in ((lse, rows), (smooth, rows), (acc, 3)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n
    check(L.lib.mvlt_ce_smooth_fwd(ptr(logits), ptr(labels), ignore_index, e, ptr(weight), ptr(lse), ptr(smooth), ptr(acc), rows, V, ld, DT[logits.dtype],
                                   stream_ptr()), "mvlt_ce_smooth_fwd")


def ce_smooth_bwd(logits, labels, lse, gscale, acc, dlogits, rows, V, ld, ldd, *, ignore_index=-1, label_smoothing=0.0, weight=None):
    """the gradient of `ce_smooth_fwd`'s mean times the device scalar gscale, from the lse and acc it left; dlogits fp32 or bf16 [rows, ldd], its padding
    columns [V, ldd) zeroed.  1 / den is taken as 0 when den is not positive (every row ignored); it is never clamped to 1."""
    e = _ce_smooth_ok(logits, labels, weight, rows, V, ld, label_smoothing)
    for t, n in ((lse, rows), (gscale, 1), (acc, 3)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n
    assert dlogits.dtype in DT and dlogits.is_contiguous() and (rows <= 0 or dlogits.numel() >= rows * ldd)
    check(L.lib.mvlt_ce_smooth_bwd(ptr(logits), ptr(labels), ignore_index, e, ptr(weight), ptr(lse), ptr(gscale), ptr(acc), ptr(dlogits), rows, V, ld, ldd,
                                   DT[logits.dtype], DT[dlogits.dtype], stream_ptr()), "mvlt_ce_smooth_bwd")


ADAMW_FROZEN = 2          # decay_mask byte of a frozen element (MVLT_ADAMW_FROZEN in include/mvlt_hip.h); 0 = step, 1 = step with weight decay


def adamw_step(p, g, m, v, p16, n, hp, decay_mask=None, *, gscale_dev=None):
    """decay_mask: one uint8 per element -- 0 step, 1 step with weight decay, ADAMW_FROZEN leave p / m / v / p16 alone.
    gscale_dev: fp32 device scalar multiplied into hp[7] inside the kernel (the clip coefficient of `clip_coef`); None = no extra factor"""
    assert decay_mask is None or decay_mask.dtype == torch.uint8
    if gscale_dev is not None:
        assert gscale_dev.dtype == torch.float32
    check(L.lib.mvlt_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), n, ptr(hp), ptr(decay_mask), ptr(gscale_dev), stream_ptr()), "mvlt_adamw_step")


def grad_sumsq(g, n, mask, partials):
    """partials[b] = sum of g[i]^2 over workgroup b's fixed share of g[0:n] (only where mask == 1 when a uint8 mask is given): no atomics, every entry stored"""
    assert g.dtype == torch.float32 and partials.dtype == torch.float32 and g.is_contiguous() and partials.is_contiguous()
    assert g.numel() >= n and (mask is None or (mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.numel() >= n))
    check(L.lib.mvlt_grad_sumsq(ptr(g), n, ptr(mask), ptr(partials), partials.numel(), stream_ptr()), "mvlt_grad_sumsq")


def clip_coef(partials, grad_scale, max_norm, out):
    """out[0] = grad_scale * sqrt(sum(partials)), out[1] = min(1, max_norm / (out[0] + 1e-6)) (torch.nn.utils.clip_grad_norm_'s coefficient)"""
    assert partials.dtype == torch.float32 and out.dtype == torch.float32 and out.numel() >= 2 and out.is_contiguous() and partials.is_contiguous()
    check(L.lib.mvlt_clip_coef(ptr(partials), partials.numel(), float(grad_scale), float(max_norm), ptr(out), stream_ptr()), "mvlt_clip_coef")


def step_gate(partials, grad_scale, max_norm, out, counters):
    """out[0:4] = [norm, coefficient, ok, 0] from the partials of `grad_sumsq`: norm = grad_scale * sqrt(sum(partials)) in `clip_coef`'s bits, ok = 1.0 when
    it is finite else 0.0, coefficient = 0 when it is not finite, min(1, max_norm / (norm + 1e-6)) when max_norm > 0, else 1.  counters (int32[2], device,
    kept by the caller from step to step): [0] += ok, [1] += not ok.  The gate `adamw_step_gated` obeys (include/mvlt_hip_ext.h)."""
    assert partials.dtype == torch.float32 and out.dtype == torch.float32 and out.numel() >= 4 and out.is_contiguous() and partials.is_contiguous()
    assert counters.dtype == torch.int32 and counters.numel() >= 2 and counters.is_contiguous()
    check(L.lib.mvlt_step_gate(ptr(partials), partials.numel(), float(grad_scale), float(max_norm), ptr(out), ptr(counters), stream_ptr()), "mvlt_step_gate")


def adamw_step_gated(p, g, m, v, p16, n, hp, decay_mask, gate):
    """`adamw_step` under the gate of `step_gate`: gate[2] == 0 -> no load or store of p / g / m / v / p16 / decay_mask at all (the step is skipped on the
    device); gate[2] == 1 -> adamw_step(..., gscale_dev=gate[1:2]) bit for bit"""
    assert decay_mask is None or decay_mask.dtype == torch.uint8
    assert gate.dtype == torch.float32 and gate.numel() >= 4 and gate.is_contiguous()
    check(L.lib.mvlt_adamw_step_gated(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), n, ptr(hp), ptr(decay_mask), ptr(gate), stream_ptr()), "mvlt_adamw_step_gated")


OPT_FROZEN = 255          # group byte of an element no launch steps (MVLT_OPT_FROZEN in include/mvlt_hip_opt.h): a frozen parameter or an alignment gap
OPT_MAX_GROUPS = 254      # MVLT_OPT_MAX_GROUPS


def adamw_step_groups(p, g, m, v, p16, n, hp, group_of, table, n_groups, *, gscale_dev=None, gate=None):
    """`adamw_step` with a learning rate and a weight decay per parameter group (include/mvlt_hip_opt.h).  hp: the fp32[8] row of `adamw_step`, its slots 0
    (lr) and 4 (weight_decay) ignored; table: fp32 [n_groups, 2] = {lr, weight_decay} on the device; group_of: one uint8 per element -- the element's group, or
    OPT_FROZEN (as any byte >= n_groups): p / m / v / p16 are left alone.  gscale_dev as for `adamw_step`, gate as for `adamw_step_gated`; at most one."""
    for t in (p, g, m, v, hp, table):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert min(p.numel(), g.numel(), m.numel(), v.numel(), group_of.numel()) >= n and hp.numel() >= 8 and table.numel() >= 2 * n_groups
    assert p16 is None or (p16.dtype == torch.bfloat16 and p16.is_contiguous() and p16.numel() >= n)
    assert group_of.dtype == torch.uint8 and group_of.is_contiguous()
    assert gscale_dev is None or gscale_dev.dtype == torch.float32
    assert gate is None or (gate.dtype == torch.float32 and gate.numel() >= 4 and gate.is_contiguous())
    check(L.lib.mvlt_adamw_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), n, ptr(hp), ptr(group_of), ptr(table), n_groups, ptr(gscale_dev), ptr(gate),
                                       stream_ptr()), "mvlt_adamw_step_groups")


LAMB_CHUNK = 16384        # elements one workgroup of lamb_moments / lamb_apply works on (MVLT_LAMB_CHUNK in include/mvlt_hip_lamb.h)
LAMB_ROW = 6              # int64 per tensor row: offset, length, group, frozen, first_chunk, n_chunks (MVLT_LAMB_ROW)
LAMB_ALWAYS_ADAPT = 1     # flags of lamb_fold (MVLT_LAMB_ALWAYS_ADAPT, MVLT_LAMB_TRUST_CLIP)
LAMB_TRUST_CLIP = 2


def lamb_check_tables(tensors, chunks, n, n_groups):
    """The two tables of the LAMB launches as HOST tensors (int64 [n_tensors, LAMB_ROW], int32 [n_chunks, 2]) against buffers of n elements and n_groups
    groups: raises MVLTError naming the first row that points outside them, overlaps, or does not tile the chunk table.  No device, no launch."""
    assert tensors.dtype == torch.int64 and chunks.dtype == torch.int32 and not tensors.is_cuda and not chunks.is_cuda
    assert tensors.is_contiguous() and chunks.is_contiguous() and tensors.numel() % LAMB_ROW == 0 and chunks.numel() % 2 == 0
    check(L.lib.mvlt_lamb_check_tables(tensors.data_ptr() or None, tensors.numel() // LAMB_ROW, chunks.data_ptr() or None, chunks.numel() // 2, n, n_groups),
          "mvlt_lamb_check_tables")


def _lamb_tables_ok(tensors, chunks):
    assert tensors.dtype == torch.int64 and tensors.is_contiguous() and tensors.numel() % LAMB_ROW == 0
    assert chunks.dtype == torch.int32 and chunks.is_contiguous() and chunks.numel() % 2 == 0
    return tensors.numel() // LAMB_ROW, chunks.numel() // 2


def lamb_moments(p, g, m, v, n, hp, tensors, chunks, table, n_groups, partials, *, gscale_dev=None, gate=None):
    """LAMB launch 1 (include/mvlt_hip_lamb.h): per chunk of one tensor, m and v stepped in `adamw_step`'s bits and partials[c] = {sum p^2, sum u^2}.  hp: the
    fp32[8] row of `adamw_step`, slots 0 and 4 ignored; table: fp32 [n_groups, 2] = {lr, weight_decay}; tensors / chunks: the device copies of tables that
    `lamb_check_tables` accepted for n.  gscale_dev as for `adamw_step`, gate as for `adamw_step_gated`; at most one."""
    nt, nc = _lamb_tables_ok(tensors, chunks)
    for t in (p, g, m, v, hp, table, partials):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert min(p.numel(), g.numel(), m.numel(), v.numel()) >= n and hp.numel() >= 8 and table.numel() >= 2 * n_groups and partials.numel() >= 2 * nc
    assert gscale_dev is None or gscale_dev.dtype == torch.float32
    assert gate is None or (gate.dtype == torch.float32 and gate.numel() >= 4 and gate.is_contiguous())
    check(L.lib.mvlt_lamb_moments(ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(hp), ptr(tensors), nt, ptr(chunks), nc, ptr(table), n_groups, ptr(partials),
                                  ptr(gscale_dev), ptr(gate), stream_ptr()), "mvlt_lamb_moments")


def lamb_fold(partials, tensors, n_chunks, table, n_groups, flags, ratios, *, gate=None):
    """LAMB launch 2: ratios[T] = ||p|| / ||u|| of every tensor that trains (1 where its weight decay is 0 unless LAMB_ALWAYS_ADAPT, and where a norm is 0;
    min(., 1) under LAMB_TRUST_CLIP) from the partials of `lamb_moments`, summed in a fixed order; frozen tensors keep what ratios held"""
    nt = tensors.numel() // LAMB_ROW
    for t in (partials, table, ratios):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert tensors.dtype == torch.int64 and tensors.is_contiguous() and partials.numel() >= 2 * n_chunks and ratios.numel() >= nt and table.numel() >= 2 * n_groups
    assert gate is None or (gate.dtype == torch.float32 and gate.numel() >= 4 and gate.is_contiguous())
    check(L.lib.mvlt_lamb_fold(ptr(partials), n_chunks, ptr(tensors), nt, ptr(table), n_groups, int(flags), ptr(ratios), ptr(gate), stream_ptr()), "mvlt_lamb_fold")


def lamb_apply(p, m, v, p16, n, hp, tensors, chunks, table, n_groups, ratios, *, gate=None):
    """LAMB launch 3: p -= lr * ratios[T] * u with u recomputed from the m, v, p that `lamb_moments` left; p16 (bf16, optional) receives the new values in
    the same pass"""
    nt, nc = _lamb_tables_ok(tensors, chunks)
    for t in (p, m, v, hp, table, ratios):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert min(p.numel(), m.numel(), v.numel()) >= n and hp.numel() >= 8 and table.numel() >= 2 * n_groups and ratios.numel() >= nt
    assert p16 is None or (p16.dtype == torch.bfloat16 and p16.is_contiguous() and p16.numel() >= n)
    assert gate is None or (gate.dtype == torch.float32 and gate.numel() >= 4 and gate.is_contiguous())
    check(L.lib.mvlt_lamb_apply(ptr(p), ptr(m), ptr(v), ptr(p16), n, ptr(hp), ptr(tensors), nt, ptr(chunks), nc, ptr(table), n_groups, ptr(ratios), ptr(gate),
                                stream_ptr()), "mvlt_lamb_apply")


def ema_update(ema, p, ema16, n, decay, one_minus_decay, mask=None):
    """ema[0:n] = ema * decay + p * one_minus_decay, the two products and the sum each rounded to fp32 on its own (timm's ModelEma formula in torch's
    bits); ema16 (bf16, optional) receives the bf16 of the new values in the same pass; mask (uint8, optional): elements whose byte is ADAMW_FROZEN are
    left alone in ema and ema16.  Both factors go by value (include/mvlt_hip_ema.h)."""
    assert ema.dtype == torch.float32 and p.dtype == torch.float32 and ema.is_contiguous() and p.is_contiguous() and ema.numel() >= n and p.numel() >= n
    assert ema16 is None or (ema16.dtype == torch.bfloat16 and ema16.is_contiguous() and ema16.numel() >= n)
    assert mask is None or (mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() >= n)
    check(L.lib.mvlt_ema_update(ptr(ema), ptr(p), ptr(ema16), n, float(decay), float(one_minus_decay), ptr(mask), stream_ptr()), "mvlt_ema_update")


def ema_update_buffers(table, n_tensors, decay, one_minus_decay):
    """one launch over a device table int64[n_tensors][4] = {dst address, src address, numel, kind}: kind 0 = fp32, averaged like `ema_update`; kind 1 =
    int64, copied (include/mvlt_hip_ema.h)"""
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= 4 * n_tensors
    check(L.lib.mvlt_ema_update_buffers(ptr(table), n_tensors, float(decay), float(one_minus_decay), stream_ptr()), "mvlt_ema_update_buffers")


def scale_by_dev(x, n, factor_dev):
    """x[0:n] *= factor_dev[0] (an fp32 device scalar; exactly 1 skips the pass on the device)"""
    assert x.dtype == torch.float32 and factor_dev.dtype == torch.float32 and x.is_contiguous() and x.numel() >= n
    check(L.lib.mvlt_scale_by_dev(ptr(x), n, ptr(factor_dev), stream_ptr()), "mvlt_scale_by_dev")


def smooth_l1_fwd(pred, target, loss_sum):
    assert pred.dtype == torch.float32 and target.dtype == torch.float32 and pred.is_contiguous() and target.is_contiguous()
    check(L.lib.mvlt_smooth_l1_fwd(ptr(pred), ptr(target), pred.numel(), ptr(loss_sum), stream_ptr()), "mvlt_smooth_l1_fwd")


def smooth_l1_bwd(pred, target, gscale, grad):
    check(L.lib.mvlt_smooth_l1_bwd(ptr(pred), ptr(target), pred.numel(), ptr(gscale), ptr(grad), stream_ptr()), "mvlt_smooth_l1_bwd")


def cast_bf16(src, dst, n):
    check(L.lib.mvlt_cast_bf16(ptr(src), ptr(dst), n, stream_ptr()), "mvlt_cast_bf16")


def row_scale(x, scale, rows_per_scale, M, Cdim, out):
    assert x.is_contiguous() and out.is_contiguous() and scale.dtype == torch.float32 and x.dtype == out.dtype
    check(L.lib.mvlt_row_scale(ptr(x), ptr(scale), rows_per_scale, M, Cdim, ptr(out), DT[x.dtype], stream_ptr()), "mvlt_row_scale")


def transpose_cast(w, out, R, Ccols, ld_out):
    assert w.dtype == torch.float32 and w.is_contiguous()
    check(L.lib.mvlt_transpose_cast(ptr(w), ptr(out), R, Ccols, ld_out, DT[out.dtype], stream_ptr()), "mvlt_transpose_cast")


# ------------------------------------------------------------------ MIM decoder helpers (csrc/mim.hip)
ZDT = {torch.float32: 1, torch.float16: 2}       # the pre-BatchNorm conv output z: fp32, or fp16 on the bf16 path (mvlt_gemm_nt out_dtype 2)


def col_stats(z, ldz, M, Cdim, s, ss):
    check(L.lib.mvlt_col_stats(ptr(z), ldz, M, Cdim, ptr(s), ptr(ss), stream_ptr()), "mvlt_col_stats")


def bn_finalize(s, ss, M, Cdim, eps, momentum, mean, rstd, running_mean=None, running_var=None, copies=1):
    check(L.lib.mvlt_bn_finalize(ptr(s), ptr(ss), copies, M, Cdim, eps, momentum, ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var), stream_ptr()),
          "mvlt_bn_finalize")


def bn_norm(z, ldz, mean, rstd, gamma, beta, M, Cdim, y32=None, ld32=0, y16=None, ld16=0):
    check(L.lib.mvlt_bn_norm(ptr(z), ldz, ZDT[z.dtype], ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), M, Cdim, ptr(y32), ld32, ZDT[y32.dtype] if y32 is not None else 1, ptr(y16), ld16,
                             DT[y16.dtype] if y16 is not None else 0, stream_ptr()), "mvlt_bn_norm")


def bn_finalize_norm(z, ldz, s, ss, copies, eps, momentum, mean, rstd, running_mean, running_var, gamma, beta, M, Cdim, y32=None, ld32=0, y16=None, ld16=0):
    assert z.dtype == torch.float16 and (y16 is None or y16.dtype == torch.bfloat16)
    check(L.lib.mvlt_bn_finalize_norm(ptr(z), ldz, ptr(s), ptr(ss), copies, eps, momentum, ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var), ptr(gamma), ptr(beta), M, Cdim,
                                      ptr(y32), ld32, ZDT[y32.dtype] if y32 is not None else 1, ptr(y16), ld16, stream_ptr()), "mvlt_bn_finalize_norm")


def bn_bwd_reduce(dy, lddy, z, ldz, mean, rstd, M, Cdim, s1, s2):
    assert dy.dtype in DT and z.dtype in ZDT
    check(L.lib.mvlt_bn_bwd_reduce(ptr(dy), lddy, ptr(z), ldz, ZDT[z.dtype], ptr(mean), ptr(rstd), M, Cdim, ptr(s1), ptr(s2), DT[dy.dtype], stream_ptr()), "mvlt_bn_bwd_reduce")


def bn_bwd_apply(dy, lddy, z, ldz, mean, rstd, gamma, s1, s2, M, Cdim, dz16, lddz, g_beta=None, g_gamma=None):
    assert dy.dtype in DT and z.dtype in ZDT
    check(L.lib.mvlt_bn_bwd_apply(ptr(dy), lddy, ptr(z), ldz, ZDT[z.dtype], ptr(mean), ptr(rstd), ptr(gamma), ptr(s1), ptr(s2), M, Cdim, ptr(dz16), lddz,
                                  ptr(g_beta), ptr(g_gamma), DT[dz16.dtype], DT[dy.dtype], stream_ptr()), "mvlt_bn_bwd_apply")


def ew_mul3_bwd(dy, lddy, a, b, c, ld, da, db, dc, M, Cdim):
    assert dy.dtype in DT and da.dtype == db.dtype == dc.dtype == dy.dtype and a.dtype == b.dtype == c.dtype and a.dtype in ZDT
    check(L.lib.mvlt_ew_mul3_bwd(ptr(dy), lddy, ptr(a), ptr(b), ptr(c), ld, ZDT[a.dtype], ptr(da), ptr(db), ptr(dc), M, Cdim, DT[dy.dtype], stream_ptr()), "mvlt_ew_mul3_bwd")


def ew_mul(out, ldo, a, lda, b, ldb, c=None, ldc=0, *, M, Cdim, accumulate=False, out16=None, ld16=0):
    assert a.dtype == b.dtype and (c is None or c.dtype == a.dtype) and a.dtype in ZDT
    check(L.lib.mvlt_ew_mul(ptr(out), ldo, ptr(a), lda, ptr(b), ldb, ptr(c), ldc, ZDT[a.dtype], M, Cdim, 1 if accumulate else 0, ptr(out16), ld16,
                            DT[out16.dtype] if out16 is not None else 0, stream_ptr()), "mvlt_ew_mul")


def upsample_fwd(x, ldx, B, H, W, Cdim, scale, out, ldo, nchw=False):
    check(L.lib.mvlt_upsample_fwd(ptr(x), ldx, B, H, W, Cdim, scale, ptr(out), ldo, DT[out.dtype], 1 if nchw else 0, stream_ptr()), "mvlt_upsample_fwd")


def upsample_bwd(dy, lddy, nchw, B, H, W, Cdim, scale, dx, lddx, accumulate=False):
    assert dy.dtype in DT and dx.dtype in DT
    check(L.lib.mvlt_upsample_bwd(ptr(dy), lddy, 1 if nchw else 0, B, H, W, Cdim, scale, ptr(dx), lddx, 1 if accumulate else 0, DT[dx.dtype],
                                  DT[dy.dtype], stream_ptr()), "mvlt_upsample_bwd")


def upsample_l1_ok(W, scale):
    """geometry the fused upsample + SmoothL1 kernels take (the final x8 upsample of the MIM decoder)"""
    return W <= 64 and (W * scale) % 4 == 0 and W * scale <= 256


def upsample_l1_fwd(x, ldx, B, H, W, Cdim, scale, target, loss_sum):
    """loss_sum[0] += sum SmoothL1(upsample(x) - target); x: fp32 [B*H*W, ldx] pixel-major, target: fp32 NCHW [B, C, H*scale, W*scale]"""
    assert x.dtype == target.dtype == loss_sum.dtype == torch.float32 and target.is_contiguous()
    check(L.lib.mvlt_upsample_l1_fwd(ptr(x), ldx, B, H, W, Cdim, scale, ptr(target), ptr(loss_sum), stream_ptr()), "mvlt_upsample_l1_fwd")


def upsample_l1_bwd(x, ldx, B, H, W, Cdim, scale, target, gscale, dx, lddx):
    """dx[:, :C] = d(mean SmoothL1) / d(x) * gscale[0] (dx bf16 or fp32, row stride lddx)"""
    assert x.dtype == target.dtype == gscale.dtype == torch.float32 and dx.dtype in DT and target.is_contiguous()
    check(L.lib.mvlt_upsample_l1_bwd(ptr(x), ldx, B, H, W, Cdim, scale, ptr(target), ptr(gscale), ptr(dx), lddx, DT[dx.dtype], stream_ptr()),
          "mvlt_upsample_l1_bwd")


# ------------------------------------------------------------------ fused MLP (csrc/mlp.hip, kernels in csrc/mlp_<family>.hip), bf16, C in {64, 128}
def _mlp_fwd_args(x, w1, b1, w2, b2, residual, out, M, Cdim, hid, *, row_scale=None, rows_per_scale=0, h_out=None, ln=None, out_op=None, post_ln=None):
    """the mvlt_mlp_args of a mlp_fwd / mlp_plan("fwd", ...) call"""
    assert w1.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16
    assert residual.dtype == torch.float32 and residual.is_contiguous() and (out is not None or out_op is not None)
    assert out is None or out.dtype == torch.float32
    assert out_op is None or (out_op.dtype == torch.bfloat16 and out_op.is_contiguous())
    a = L.MlpArgs(x=ptr(x), w1=ptr(w1), wb=ptr(w2), b1=ptr(b1), b2=ptr(b2), residual=ptr(residual), row_scale=ptr(row_scale), rows_per_scale=rows_per_scale,
                  out=ptr(out), h_out=ptr(h_out), M=M, C=Cdim, hid=hid, out_op=ptr(out_op))
    if ln is None:
        assert x.dtype == torch.bfloat16
    else:
        g, b, eps, y, mean, rstd = ln
        assert g.dtype == b.dtype == mean.dtype == rstd.dtype == torch.float32 and y.dtype == torch.bfloat16 and y.is_contiguous()
        a.ln_x, a.ln_gamma, a.ln_beta, a.ln_eps, a.ln_y, a.ln_mean, a.ln_rstd = ptr(residual), ptr(g), ptr(b), eps, ptr(y), ptr(mean), ptr(rstd)
    if post_ln is not None:
        pg, pb, peps, py, pm, pr = post_ln
        assert pg.dtype == pb.dtype == pm.dtype == pr.dtype == torch.float32 and py.dtype == torch.bfloat16 and py.is_contiguous()
        a.post_gamma, a.post_beta, a.post_eps, a.post_y, a.post_mean, a.post_rstd = ptr(pg), ptr(pb), peps, ptr(py), ptr(pm), ptr(pr)
    return a


def mlp_fwd(x, w1, b1, w2, b2, residual, out, *dims, out_op=None, **kw):
    """mlp_fwd(x, w1, b1, w2, b2, residual, out, M, Cdim, hid, *, row_scale, rows_per_scale, h_out, ln, out_op, post_ln)
    ln = (gamma, beta, eps, y, mean, rstd): LayerNorm(residual) folded into the operand load -- `x` is then not read (may be None);
    y (bf16 [M, C]) receives the normalised rows, mean / rstd (fp32 [M]) the row statistics.
    out_op: optional bf16 [M, C] copy of the output; `out` (fp32) may be None when only the copy is wanted.
    post_ln = (gamma, beta, eps, y, mean, rstd): LayerNorm of the OUTPUT rows (the next block's norm1) from the epilogue."""
    check(L.lib.mvlt_mlp_fwd(C.byref(_mlp_fwd_args(x, w1, b1, w2, b2, residual, out, *dims, out_op=out_op, **kw)), stream_ptr()), "mvlt_mlp_fwd")
    return out if out is not None else out_op


def _mlp_bwd_dx_args(x, dy, w1, w1t, w2t, b1, out, M, Cdim, hid, *, row_scale=None, rows_per_scale=0, ln_bwd=None, lnb_partials=None):
    """the mvlt_mlp_args of a mlp_bwd_dx / mlp_plan("bwd_dx", ...) call; lnb_partials: the per-workgroup column sums of ln_bwd (fp32 [ceil(M / 128), 2 C])"""
    assert x.dtype == dy.dtype == torch.bfloat16 and (out is None or out.dtype == torch.bfloat16)
    a = L.MlpArgs(x=ptr(x), dy=ptr(dy), w1=ptr(w1), wb=ptr(w1t), wc=ptr(w2t), b1=ptr(b1), row_scale=ptr(row_scale), rows_per_scale=rows_per_scale, M=M, C=Cdim, hid=hid)
    if ln_bwd is None:
        a.out = ptr(out)
        return a
    k = ln_bwd
    assert k["x"].dtype == torch.float32 and k["dx"].dtype == torch.bfloat16 and k["dx"].is_contiguous() and k["x"].is_contiguous()
    assert k["mean"].dtype == k["rstd"].dtype == k["gamma"].dtype == k["dgamma"].dtype == k["dbeta"].dtype == torch.float32
    dx2 = k.get("dx2")
    assert dx2 is None or (dx2.dtype == torch.bfloat16 and dx2.is_contiguous() and k["dx2_scale"].dtype == torch.float32)
    a.lnb_x, a.lnb_mean, a.lnb_rstd, a.lnb_gamma, a.lnb_dx = ptr(k["x"]), ptr(k["mean"]), ptr(k["rstd"]), ptr(k["gamma"]), ptr(k["dx"])
    a.lnb_dx2, a.lnb_dx2_scale, a.lnb_dx2_rows_per_scale, a.lnb_partials = ptr(dx2), ptr(k.get("dx2_scale")), int(k.get("dx2_rows_per_scale", 0)), ptr(lnb_partials)
    return a


def mlp_bwd_dx(x, dy, w1, w1t, w2t, b1, out, M, Cdim, hid, *, ln_bwd=None, **kw):
    """mlp_bwd_dx(x, dy, w1, w1t, w2t, b1, out, M, Cdim, hid, *, row_scale, rows_per_scale, ln_bwd)
    ln_bwd = dict(x, mean, rstd, gamma, dx, dgamma, dbeta[, dx2, dx2_scale, dx2_rows_per_scale]): the backward of the LayerNorm in
    front of the MLP from this kernel's epilogue -- dx (bf16 [M, C], may be `dy`) += LN backward in place, dx2 = its scaled copy,
    dgamma / dbeta += the column sums (through per-workgroup partials and one mvlt_add_column_sums launch); `out` is not written."""
    if ln_bwd is None:
        check(L.lib.mvlt_mlp_bwd_dx(C.byref(_mlp_bwd_dx_args(x, dy, w1, w1t, w2t, b1, out, M, Cdim, hid, **kw)), stream_ptr()), "mvlt_mlp_bwd_dx")
        return out
    partials = torch.empty((M + 127) // 128, 2 * Cdim, device=x.device, dtype=torch.float32)
    a = _mlp_bwd_dx_args(x, dy, w1, w1t, w2t, b1, out, M, Cdim, hid, ln_bwd=ln_bwd, lnb_partials=partials, **kw)
    check(L.lib.mvlt_mlp_bwd_dx(C.byref(a), stream_ptr()), "mvlt_mlp_bwd_dx")
    add_column_sums(partials, ln_bwd["dgamma"], ln_bwd["dbeta"])
    return ln_bwd["dx"]


def add_column_sums(partials, dst0, dst1):
    """dst0 += column sums of partials[:, :n0], dst1 += those of partials[:, n0:] (fp32)"""
    rows, cols = partials.shape
    assert partials.dtype == dst0.dtype == dst1.dtype == torch.float32 and partials.is_contiguous() and dst0.numel() + dst1.numel() == cols
    check(L.lib.mvlt_add_column_sums(ptr(partials), rows, cols, cols, ptr(dst0), dst0.numel(), ptr(dst1), stream_ptr()), "mvlt_add_column_sums")


def _mlp_bwd_dw_args(x, dy, w1, w2t, b1, dw1, db1, dw2, db2, M, Cdim, hid, *, row_scale=None, rows_per_scale=0, partials=None, defer_fold=False):
    """the mvlt_mlp_args of a mlp_bwd_dw / mlp_plan("bwd_dw", ...) call"""
    assert x.dtype == dy.dtype == torch.bfloat16 and dw1.dtype == torch.float32
    a = L.MlpArgs(x=ptr(x), dy=ptr(dy), w1=ptr(w1), wc=ptr(w2t), b1=ptr(b1), row_scale=ptr(row_scale), rows_per_scale=rows_per_scale,
                  dw1=ptr(dw1), db1=ptr(db1), dw2=ptr(dw2), db2=ptr(db2), M=M, C=Cdim, hid=hid)
    if partials is not None:
        a.partials, a.partials_bytes, a.defer_fold = ptr(partials), partials.numel() * partials.element_size(), 1 if defer_fold else 0
    return a


def mlp_bwd_dw(*args, **kw):
    """mlp_bwd_dw(x, dy, w1, w2t, b1, dw1, db1, dw2, db2, M, Cdim, hid, *, row_scale, rows_per_scale, partials, defer_fold)
    partials = the weight-gradient scratch of gemm_tn (FlatStore.tn_partials()): the token splits leave as bf16 partial tiles + the ordered fold instead of fp32 atomics;
    defer_fold: folded with the other pending ones (tn_fold_flush before anything reads dw1 / dw2)"""
    check(L.lib.mvlt_mlp_bwd_dw(C.byref(_mlp_bwd_dw_args(*args, **kw)), stream_ptr()), "mvlt_mlp_bwd_dw")


_MLP_PLANS = {"fwd": (_mlp_fwd_args, "mvlt_mlp_fwd_plan"), "bwd_dx": (_mlp_bwd_dx_args, "mvlt_mlp_bwd_dx_plan"), "bwd_dw": (_mlp_bwd_dw_args, "mvlt_mlp_bwd_dw_plan")}


def mlp_plan(which, *args, **kw):
    """what mlp_fwd / mlp_bwd_dx / mlp_bwd_dw (which = "fwd" / "bwd_dx" / "bwd_dw") would launch for the same arguments (mvlt_mlp_plan of include/mvlt_hip_plan.h,
    .name as _lib.last_kernel() prints it); nothing is launched and no device is touched.  A single _lib.MlpArgs stands for the arguments as well (the plan looks at
    pointers, it never follows them).  With ln_bwd the per-workgroup partials mlp_bwd_dx allocates are stood in for by ln_bwd["dx"]."""
    make, entry = _MLP_PLANS[which]
    if len(args) == 1 and isinstance(args[0], L.MlpArgs):
        a = args[0]
    else:
        if which == "bwd_dx" and kw.get("ln_bwd") is not None:
            kw.setdefault("lnb_partials", kw["ln_bwd"]["dx"])
        a = make(*args, **kw)
    return Plan(getattr(L.lib, entry), a, L.MlpPlan, L.lib.mvlt_mlp_plan_name)


# ------------------------------------------------------------------ device-side batch preparation (csrc/batchprep.hip)
def grid_mask_flags(flags, B, gh, gw, num_mask, mode, seed, sample0):
    assert flags.dtype == torch.uint8 and flags.is_contiguous() and flags.numel() == B * gh * gw
    check(L.lib.mvlt_grid_mask_flags(ptr(flags), B, gh, gw, num_mask, mode, seed, sample0, stream_ptr()), "mvlt_grid_mask_flags")
    return flags


def grid_mask_apply(image, flags, masked, patch=16, fill=1e-6):
    assert image.dtype == torch.float32 and masked.dtype == torch.float32 and image.is_contiguous() and masked.is_contiguous()
    B, Cc, H, W = image.shape
    check(L.lib.mvlt_grid_mask_apply(ptr(image), ptr(flags), ptr(masked), B, Cc, H, W, patch, fill, stream_ptr()), "mvlt_grid_mask_apply")
    return masked


def token_mask(ori_ids, input_ids, labels, seed, sample0, vocab=30522):
    assert ori_ids.dtype == input_ids.dtype == labels.dtype == torch.int64 and ori_ids.is_contiguous()
    B, T = ori_ids.shape
    check(L.lib.mvlt_token_mask(ptr(ori_ids), ptr(input_ids), ptr(labels), B, T, seed, sample0, vocab, stream_ptr()), "mvlt_token_mask")


def keep_mask(keep, drop_p, seed, call):
    """keep (uint8, any shape, contiguous) <- Bernoulli(1 - drop_p) from Philox(seed; call)"""
    assert keep.dtype == torch.uint8 and keep.is_contiguous()
    check(L.lib.mvlt_keep_mask(ptr(keep), keep.numel(), drop_p, seed & (2 ** 64 - 1), call, stream_ptr()), "mvlt_keep_mask")
    return keep


def droppath_scales(out, rates, seed, call):
    """out (fp32 [nrate, ...]) <- Bernoulli(1 - rates[r]) / (1 - rates[r]) per element of row r"""
    assert out.dtype == rates.dtype == torch.float32 and out.is_contiguous() and rates.is_contiguous() and out.shape[0] == rates.numel()
    check(L.lib.mvlt_droppath_scales(ptr(out), ptr(rates), rates.numel(), out.numel() // max(1, rates.numel()), seed & (2 ** 64 - 1), call, stream_ptr()),
          "mvlt_droppath_scales")
    return out


# ------------------------------------------------------------------ image ingest: uint8 pixels -> fp32 image + grid-masked copy (csrc/ingest.hip, include/mvlt_hip_ingest.h)
def ingest_table(mean=None, std=None):
    """the fp32 (3, 256) value table of `image_ingest`, on the CPU, computed the way torchvision's ToTensor (`byte.float().div(255)`) and Normalize
    (`.sub(mean).div(std)` with fp32 mean / std) compute a pixel, so the kernel's output equals that transform bit for bit by construction"""
    assert (mean is None) == (std is None)
    t = torch.arange(256).float().div(255).repeat(3, 1)
    if mean is not None:
        m, s = torch.as_tensor(mean, dtype=torch.float32).view(3, 1), torch.as_tensor(std, dtype=torch.float32).view(3, 1)
        assert bool((s != 0).all())
        t = t.sub(m).div(s)
    return t.contiguous()


def ingest_norm(mean, std):
    """the fp32 [6] = {mean[3], std[3]} argument of `image_ingest_resize`, on the CPU"""
    t = torch.cat([torch.as_tensor(mean, dtype=torch.float32).view(3), torch.as_tensor(std, dtype=torch.float32).view(3)])
    assert bool((t[3:] != 0).all())
    return t.contiguous()


def _ingest_out_ok(image, masked, flags, B, H, W, patch):
    assert image.dtype == torch.float32 and image.is_contiguous() and tuple(image.shape) == (B, 3, H, W)
    assert (masked is None) == (flags is None)
    if masked is not None:
        assert masked.dtype == torch.float32 and masked.is_contiguous() and masked.shape == image.shape
        assert flags.dtype == torch.uint8 and flags.is_contiguous() and patch > 0 and flags.numel() == B * (H // patch) * (W // patch)


def image_ingest(src, table, image, masked=None, flags=None, layout=0, patch=16, fill=1e-6):
    """image (B,3,H,W) fp32 <- table[c][src] for uint8 src (B,H,W,3) (layout 0) or (B,3,H,W) (layout 1); table: `ingest_table(...)` on the device.  With masked / flags
    (uint8, B * H/patch * W/patch) the same pass writes masked = flags ? fill : image -- `grid_mask_apply`'s result without its launch."""
    assert src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 4 and layout in (0, 1)
    B, H, W = (src.shape[0], src.shape[1], src.shape[2]) if layout == 0 else (src.shape[0], src.shape[2], src.shape[3])
    assert src.shape[3 if layout == 0 else 1] == 3
    assert table.dtype == torch.float32 and table.is_contiguous() and table.numel() == 768
    _ingest_out_ok(image, masked, flags, B, H, W, patch)
    check(L.lib.mvlt_image_ingest(ptr(src), layout, ptr(table), ptr(image), ptr(masked), ptr(flags), B, H, W, patch, fill, stream_ptr()), "mvlt_image_ingest")
    return image


def image_ingest_resize(src, rects, rects_host, image, masked=None, flags=None, flip=None, norm=None, patch=16, fill=1e-6):
    """image (B,3,H,W) fp32 <- each sample's rectangle rects[b] = (y0, x0, h, w) of the uint8 slab src (B,Hmax,Wmax,3), resampled to (H, W) by the antialiased
    triangle filter (Pillow's resize(BILINEAR) geometry, fp32 intermediate), mirrored where flip[b] is set, / 255, then (. - mean) / std with norm =
    `ingest_norm(mean, std)` on the device.  rects: int32 (B,4) on the device; rects_host: the same values in a CPU tensor -- the entry point checks THEM (inside
    the slab, downscale factor at most 8) before it launches, so no sync is needed.  masked / flags as in `image_ingest`."""
    assert src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 4 and src.shape[3] == 3
    B, Hmax, Wmax = src.shape[0], src.shape[1], src.shape[2]
    assert rects.dtype == torch.int32 and rects.is_contiguous() and tuple(rects.shape) == (B, 4)
    assert not rects_host.is_cuda and rects_host.dtype == torch.int32 and rects_host.is_contiguous() and tuple(rects_host.shape) == (B, 4)
    assert image.dim() == 4
    H, W = image.shape[2], image.shape[3]
    _ingest_out_ok(image, masked, flags, B, H, W, patch)
    assert flip is None or (flip.dtype == torch.uint8 and flip.is_contiguous() and flip.numel() == B)
    assert norm is None or (norm.dtype == torch.float32 and norm.is_contiguous() and norm.numel() == 6)
    check(L.lib.mvlt_image_ingest_resize(ptr(src), Hmax, Wmax, ptr(rects), rects_host.data_ptr(), ptr(flip), ptr(norm), ptr(image), ptr(masked), ptr(flags),
                                         B, H, W, patch, fill, stream_ptr()), "mvlt_image_ingest_resize")
    return image


def flip_flags(flip, p, seed, sample0):
    """flip (uint8 [B]) <- Bernoulli(p) per sample from Philox(seed; sample0 + b, element 0, stream 6): (draw >> 8) < round(p * 2^24)"""
    assert flip.dtype == torch.uint8 and flip.is_contiguous() and flip.dim() == 1
    check(L.lib.mvlt_flip_flags(ptr(flip), flip.numel(), p, seed & (2 ** 64 - 1), sample0, stream_ptr()), "mvlt_flip_flags")
    return flip


# ------------------------------------------------------------------ position-embedding resize, GELU backward (csrc/elementwise.hip)
def loss_compose(losses, weights, out, total):
    """out[0] = total[0] = sum_i weights[i] * losses[i], out[1 + i] = weights[i] * losses[i]; losses: five fp32 device scalars or None"""
    assert len(losses) == len(weights) == 5 and out.dtype == total.dtype == torch.float32 and out.numel() >= 6 and out.is_contiguous()
    for t in losses:
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1)
    ptrs = (C.c_void_p * 5)(*[ptr(t) for t in losses])
    ws = (C.c_float * 5)(*[float(w) for w in weights])
    check(L.lib.mvlt_loss_compose(ptrs, ws, ptr(out), ptr(total), stream_ptr()), "mvlt_loss_compose")
    return out


def resize_bilinear_tokens_multi(jobs, adjoint=False):
    """jobs: up to four (src, dst, hin, win, hout, wout, Cdim) like resize_bilinear_tokens, one launch"""
    n = len(jobs)
    assert 1 <= n <= 4
    for src, dst, *_ in jobs:
        assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.stride(-1) == 1 and dst.stride(-1) == 1
    P, I = C.c_void_p * n, C.c_int * n
    arr = lambda f: I(*[f(j) for j in jobs])
    check(L.lib.mvlt_resize_bilinear_tokens_multi(P(*[ptr(j[0]) for j in jobs]), arr(lambda j: j[0].stride(0)), P(*[ptr(j[1]) for j in jobs]),
                                                  arr(lambda j: j[1].stride(0)), arr(lambda j: j[2]), arr(lambda j: j[3]), arr(lambda j: j[4]), arr(lambda j: j[5]),
                                                  arr(lambda j: j[6]), n, 1 if adjoint else 0, stream_ptr()), "mvlt_resize_bilinear_tokens_multi")


def resize_bilinear_tokens(src, dst, hin, win, hout, wout, Cdim, adjoint=False):
    """src [hin*win, C] -> dst [hout*wout, C] (fp32, rows Cdim floats apart); adjoint: src is d(dst-shaped), accumulated into dst = d(source map)"""
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.stride(-1) == 1 and dst.stride(-1) == 1
    check(L.lib.mvlt_resize_bilinear_tokens(ptr(src), src.stride(0), ptr(dst), dst.stride(0), hin, win, hout, wout, Cdim, 1 if adjoint else 0, stream_ptr()),
          "mvlt_resize_bilinear_tokens")
    return dst


def gelu_bwd(dy, h, out):
    assert dy.dtype == h.dtype == out.dtype and dy.is_contiguous() and h.is_contiguous() and out.is_contiguous()
    check(L.lib.mvlt_gelu_bwd(ptr(dy), ptr(h), ptr(out), dy.numel(), DT[dy.dtype], stream_ptr()), "mvlt_gelu_bwd")
    return out

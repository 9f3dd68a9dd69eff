"""ctypes binding of libmvlt_hip.so (the C ABI declared in include/mvlt_hip.h, and the additions of include/mvlt_hip_ext.h, include/mvlt_hip_ema.h, include/mvlt_hip_plan.h, include/mvlt_hip_opt.h, include/mvlt_hip_lamb.h, include/mvlt_hip_loss.h and include/mvlt_hip_ingest.h).

The product path has NO fallback: importing this module without the built library, or calling an op without a
GPU, raises.  torch is used only for device memory and streams.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVLT_HIP_LIB") or os.path.join(_HERE, "libmvlt_hip.so")      # override: A/B runs of two builds


class MVLTError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is missing: build it with `python -m mvlt_amd.build` (hipcc, gfx950). "
                      "mvlt_amd has no CPU or eager fallback.")
lib = C.CDLL(LIB_PATH)

c_int, c_float, c_void_p, c_long = C.c_int, C.c_float, C.c_void_p, C.c_long


class RowMap(C.Structure):
    _fields_ = [(n, c_int) for n in ("mode", "rows_per_batch", "batch_stride", "offset",
                                     "r", "w_in", "tokens_in", "hw_out", "w_out", "c_seg", "h_in")]


class GemmNTArgs(C.Structure):
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p),
                ("M", c_int), ("N", c_int), ("K", c_int), ("lda", c_int), ("ldb", c_int), ("ldc", c_int),
                ("dtype", c_int), ("out_dtype", c_int),
                ("a_map", RowMap), ("c_map", RowMap),
                ("bias", c_void_p), ("act", c_int), ("H", c_void_p),
                ("row_scale", c_void_p), ("rows_per_scale", c_int), ("R", c_void_p),
                ("col_sum", c_void_p), ("col_sumsq", c_void_p), ("col_copies", c_int), ("split_k", c_int),
                ("post_y", c_void_p), ("post_ld", c_int), ("post_gamma", c_void_p), ("post_beta", c_void_p), ("post_eps", c_float),
                ("post_mean", c_void_p), ("post_rstd", c_void_p), ("r_fp32", c_int)]


class PrepDesc(C.Structure):
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("kind", c_int), ("R", c_int), ("C", c_int), ("ld_out", c_int),
                ("d0", c_int), ("d1", c_int), ("d2", c_int), ("src_off", c_int), ("ss0", c_int), ("ss1", c_int), ("ss2", c_int),
                ("ds0", c_int), ("ds1", c_int), ("ds2", c_int)]


class GemmTNArgs(C.Structure):
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p),
                ("M", c_int), ("N1", c_int), ("N2", c_int), ("lda", c_int), ("ldb", c_int), ("ldc", c_int),
                ("dtype", c_int), ("a_map", RowMap), ("b_map", RowMap),
                ("colsum_a", c_void_p), ("splits", c_int), ("colsum_b", c_void_p), ("trans_c", c_int),
                ("c_taps", c_int), ("c_seg", c_int), ("dgrad_wt", c_void_p), ("dgrad_out", c_void_p), ("dgrad_ld", c_int),
                ("partials", c_void_p), ("partials_bytes", c_long), ("defer_fold", c_int), ("c_overwrite", c_int)]


class LayerNormArgs(C.Structure):
    _fields_ = [("x", c_void_p), ("y", c_void_p), ("gamma", c_void_p), ("beta", c_void_p),
                ("mean", c_void_p), ("rstd", c_void_p), ("add", c_void_p), ("add_rows", c_int),
                ("rows", c_int), ("C", c_int), ("ldx", c_int), ("ldy", c_int),
                ("x_map", RowMap), ("y_map", RowMap), ("eps", c_float), ("dtype", c_int), ("y_dtype", c_int),
                ("y2", c_void_p), ("gamma2", c_void_p), ("beta2", c_void_p), ("eps2", c_float), ("mean2", c_void_p), ("rstd2", c_void_p)]


class LayerNormBwdArgs(C.Structure):
    _fields_ = [("dy", c_void_p), ("x", c_void_p), ("dx", c_void_p),
                ("gamma", c_void_p), ("mean", c_void_p), ("rstd", c_void_p),
                ("dgamma", c_void_p), ("dbeta", c_void_p),
                ("rows", c_int), ("C", c_int), ("lddy", c_int), ("ldx", c_int), ("lddx", c_int),
                ("dy_map", RowMap), ("x_map", RowMap), ("dx_map", RowMap),
                ("dx_accumulate", c_int), ("dtype", c_int), ("x_dtype", c_int), ("dx_dtype", c_int),
                ("dx2", c_void_p), ("dx2_scale", c_void_p), ("dx2_rows_per_scale", c_int), ("lddx2", c_int),
                ("dg_copies", c_int), ("dg_copy_stride", c_long)]


class AttnArgs(C.Structure):
    _fields_ = [("Q", c_void_p), ("KV", c_void_p), ("O", c_void_p), ("lse", c_void_p),
                ("B", c_int), ("H", c_int), ("N", c_int), ("M", c_int),
                ("ldq", c_int), ("ldkv", c_int), ("ldo", c_int), ("k_off", c_int), ("v_off", c_int),
                ("scale", c_float), ("dtype", c_int)]


class AttnBwdArgs(C.Structure):
    _fields_ = [("Q", c_void_p), ("KV", c_void_p), ("O", c_void_p), ("dO", c_void_p), ("lse", c_void_p),
                ("dQ", c_void_p), ("dKV", c_void_p),
                ("B", c_int), ("H", c_int), ("N", c_int), ("M", c_int),
                ("ldq", c_int), ("ldkv", c_int), ("ldo", c_int), ("lddkv", c_int),
                ("k_off", c_int), ("v_off", c_int), ("scale", c_float), ("dtype", c_int), ("dkv_dtype", c_int)]


class MlpArgs(C.Structure):
    _fields_ = [("x", c_void_p), ("dy", c_void_p), ("w1", c_void_p), ("wb", c_void_p), ("wc", c_void_p),
                ("b1", c_void_p), ("b2", c_void_p), ("residual", c_void_p), ("row_scale", c_void_p), ("rows_per_scale", c_int),
                ("out", c_void_p), ("h_out", c_void_p), ("dw1", c_void_p), ("db1", c_void_p), ("dw2", c_void_p), ("db2", c_void_p),
                ("M", c_int), ("C", c_int), ("hid", c_int),
                ("ln_x", c_void_p), ("ln_gamma", c_void_p), ("ln_beta", c_void_p), ("ln_eps", c_float),
                ("ln_y", c_void_p), ("ln_mean", c_void_p), ("ln_rstd", c_void_p), ("out_op", c_void_p),
                ("post_gamma", c_void_p), ("post_beta", c_void_p), ("post_eps", c_float),
                ("post_y", c_void_p), ("post_mean", c_void_p), ("post_rstd", c_void_p),
                ("lnb_x", c_void_p), ("lnb_mean", c_void_p), ("lnb_rstd", c_void_p), ("lnb_gamma", c_void_p),
                ("lnb_dx", c_void_p), ("lnb_dx2", c_void_p), ("lnb_dx2_scale", c_void_p), ("lnb_dx2_rows_per_scale", c_int),
                ("lnb_partials", c_void_p), ("partials", c_void_p), ("partials_bytes", c_long), ("defer_fold", c_int)]


# header name -> class of every argument struct: the import-time size check below and the header-against-binding test walk it
STRUCTS = (("mvlt_rowmap", RowMap), ("mvlt_prep_desc", PrepDesc), ("mvlt_gemm_nt_args", GemmNTArgs), ("mvlt_gemm_tn_args", GemmTNArgs),
           ("mvlt_layernorm_args", LayerNormArgs), ("mvlt_layernorm_bwd_args", LayerNormBwdArgs),
           ("mvlt_attn_args", AttnArgs), ("mvlt_attn_bwd_args", AttnBwdArgs), ("mvlt_mlp_args", MlpArgs))

# entry point -> (restype, argtypes), parameter by parameter as include/mvlt_hip.h declares them (tests/test_host_cpu.py compares the two).  Every pointer a
# tensor goes into is c_void_p, so ptr() hands over plain ints; struct arguments are POINTER(class) and take C.byref(args).
_vp, _i, _l, _f, _u64, _str = c_void_p, c_int, c_long, c_float, C.c_uint64, C.c_char_p
_by_args = lambda cls: (_i, [C.POINTER(cls), _vp])          # int f(const <struct>* args, void* stream)
PROTOTYPES = {
    "mvlt_last_error": (_str, []),
    "mvlt_abi_version": (_i, []),
    "mvlt_last_kernel": (_str, []),
    "mvlt_sizeof": (_i, [_str]),
    "mvlt_gemm_nt": _by_args(GemmNTArgs),
    "mvlt_gemm_tn": _by_args(GemmTNArgs),
    "mvlt_tn_fold_flush": (_i, [_vp, _vp]),
    "mvlt_tn_fold_discard": (_i, [_vp]),
    "mvlt_layernorm_fwd": _by_args(LayerNormArgs),
    "mvlt_layernorm_bwd": _by_args(LayerNormBwdArgs),
    "mvlt_fold_copies": (_i, [_vp, _i, _l, _vp, _i, _i, _vp, _vp]),
    "mvlt_batch_sum": (_i, [_vp, _vp, _i, _i, _i, _l, _i, _i, _vp, _i, _vp]),
    "mvlt_sr_attention_fwd": _by_args(AttnArgs),
    "mvlt_sr_attention_bwd": _by_args(AttnBwdArgs),
    "mvlt_sr_attention_bwd_chunks": (_i, [_i] * 5),
    "mvlt_sr_attention_fwd_streamed": _by_args(AttnArgs),
    "mvlt_sr_attention_bwd_streamed": _by_args(AttnBwdArgs),
    # csrc/elementwise.hip
    "mvlt_bert_embed_fwd": (_i, [_vp] * 7 + [_f, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "mvlt_bert_embed_bwd": (_i, [_vp] * 7 + [_f] + [_vp] * 7 + [_i, _i, _i, _i, _vp]),
    "mvlt_patchify": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mvlt_masked_select": (_i, [_vp, _i, _l, _vp, _vp, _vp]),
    "mvlt_resize_bilinear_tokens": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "mvlt_resize_bilinear_tokens_multi": (_i, [_vp] * 9 + [_i, _i, _vp]),
    "mvlt_gelu_bwd": (_i, [_vp, _vp, _vp, _l, _i, _vp]),
    "mvlt_loss_compose": (_i, [C.POINTER(c_void_p), C.POINTER(c_float), _vp, _vp, _vp]),
    # csrc/batchprep.hip
    "mvlt_grid_mask_flags": (_i, [_vp, _i, _i, _i, _i, _i, _u64, _u64, _vp]),
    "mvlt_grid_mask_apply": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "mvlt_token_mask": (_i, [_vp, _vp, _vp, _i, _i, _u64, _u64, _i, _vp]),
    "mvlt_keep_mask": (_i, [_vp, _l, _f, _u64, _u64, _vp]),
    "mvlt_droppath_scales": (_i, [_vp, _vp, _i, _i, _u64, _u64, _vp]),
    "mvlt_gather_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(RowMap), _i, _vp]),
    "mvlt_scatter_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(RowMap), _i, _i, _vp]),
    "mvlt_cross_entropy_fwd": (_i, [_vp, _vp, _l, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlt_cross_entropy_bwd": (_i, [_vp, _vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mvlt_smooth_l1_fwd": (_i, [_vp, _vp, _l, _vp, _vp]),
    "mvlt_smooth_l1_bwd": (_i, [_vp, _vp, _l, _vp, _vp, _vp]),
    "mvlt_adamw_step": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _vp]),
    "mvlt_grad_sumsq": (_i, [_vp, _l, _vp, _vp, _i, _vp]),
    "mvlt_clip_coef": (_i, [_vp, _i, _f, _f, _vp, _vp]),
    "mvlt_scale_by_dev": (_i, [_vp, _l, _vp, _vp]),
    "mvlt_cast_bf16": (_i, [_vp, _vp, _l, _vp]),
    "mvlt_row_scale": (_i, [_vp, _vp, _i, _l, _i, _vp, _i, _vp]),
    "mvlt_head_grad_prep": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "mvlt_transpose_cast": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlt_weight_prep": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp]),          # descs: a DEVICE table of PrepDesc, hence no POINTER(PrepDesc)
    # csrc/mlp.hip (kernels: csrc/mlp_<family>.hip)
    "mvlt_mlp_fwd": _by_args(MlpArgs),
    "mvlt_mlp_bwd_dx": _by_args(MlpArgs),
    "mvlt_mlp_bwd_dw": _by_args(MlpArgs),
    "mvlt_add_column_sums": (_i, [_vp, _l, _i, _i, _vp, _i, _vp, _vp]),
    # csrc/mim.hip
    "mvlt_col_stats": (_i, [_vp, _i, _l, _i, _vp, _vp, _vp]),
    "mvlt_bn_finalize": (_i, [_vp, _vp, _i, _l, _i, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "mvlt_bn_norm": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _l, _i, _vp, _i, _i, _vp, _i, _i, _vp]),
    "mvlt_bn_finalize_norm": (_i, [_vp, _i, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _l, _i, _vp, _i, _i, _vp, _i, _vp]),
    "mvlt_bn_bwd_reduce": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _l, _i, _vp, _vp, _i, _vp]),
    "mvlt_bn_bwd_apply": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _l, _i, _vp, _i, _vp, _vp, _i, _i, _vp]),
    "mvlt_ew_mul": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _l, _i, _i, _vp, _i, _i, _vp]),
    "mvlt_ew_mul3_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _l, _i, _i, _vp]),
    "mvlt_upsample_fwd": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "mvlt_upsample_bwd": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    "mvlt_upsample_l1_fwd": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mvlt_upsample_l1_bwd": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp]),
}
EXPORTS = list(PROTOTYPES)
for _name, (_res, _args) in PROTOTYPES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

ABI_VERSION = 8          # include/mvlt_hip.h MVLT_ABI_VERSION this binding was written against
if lib.mvlt_abi_version() != ABI_VERSION:
    raise ImportError(f"ABI mismatch: {LIB_PATH} is version {lib.mvlt_abi_version()}, the binding is version {ABI_VERSION} (stale build? run python -m mvlt_amd.build)")
for _name, _cls in STRUCTS:
    _n = lib.mvlt_sizeof(_name.encode())
    if _n != C.sizeof(_cls):
        raise ImportError(f"ABI mismatch for {_name}: library says {_n} bytes, binding has {C.sizeof(_cls)}")

# The entry points of include/mvlt_hip_ext.h: additions beside the ABI above (whose table and version stay as they are), bound the same way and checked
# against their own version number (tests/test_guard_cpu.py compares this table with that header).
EXT_PROTOTYPES = {
    "mvlt_ext_version": (_i, []),
    "mvlt_step_gate": (_i, [_vp, _i, _f, _f, _vp, _vp, _vp]),
    "mvlt_adamw_step_gated": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _vp]),
}
for _name, (_res, _args) in EXT_PROTOTYPES.items():
    if not hasattr(lib, _name):
        raise ImportError(f"{LIB_PATH} does not export {_name} (include/mvlt_hip_ext.h): stale build? run python -m mvlt_amd.build")
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

EXT_VERSION = 1          # include/mvlt_hip_ext.h MVLT_EXT_VERSION this binding was written against
if lib.mvlt_ext_version() != EXT_VERSION:
    raise ImportError(f"extension mismatch: {LIB_PATH} is version {lib.mvlt_ext_version()}, the binding is version {EXT_VERSION} (stale build? run python -m mvlt_amd.build)")

# The entry points of include/mvlt_hip_ema.h (the fused weight EMA, docs/ema.md): a third table, bound and version-checked like the one above
# (tests/test_ema_cpu.py compares it with that header).
EMA_PROTOTYPES = {
    "mvlt_ema_version": (_i, []),
    "mvlt_ema_update": (_i, [_vp, _vp, _vp, _l, _f, _f, _vp, _vp]),
    "mvlt_ema_update_buffers": (_i, [_vp, _i, _f, _f, _vp]),             # table: a DEVICE array of int64[n][4]
}
for _name, (_res, _args) in EMA_PROTOTYPES.items():
    if not hasattr(lib, _name):
        raise ImportError(f"{LIB_PATH} does not export {_name} (include/mvlt_hip_ema.h): stale build? run python -m mvlt_amd.build")
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

EMA_VERSION = 1          # include/mvlt_hip_ema.h MVLT_EMA_VERSION this binding was written against
if lib.mvlt_ema_version() != EMA_VERSION:
    raise ImportError(f"EMA entry points mismatch: {LIB_PATH} is version {lib.mvlt_ema_version()}, the binding is version {EMA_VERSION} (stale build? run python -m mvlt_amd.build)")

# The entry points of include/mvlt_hip_plan.h (what the GEMM, the SR-attention and the fused-MLP entry points would launch, without a device): a fourth table with its own structs,
# bound and version-checked like the ones above (tests/test_gemm_plan_cpu.py compares both with that header).
class GemmPlan(C.Structure):
    _fields_ = [("family", c_int), ("tp", c_int * 6), ("grid", c_int * 3), ("block", c_int), ("lds", c_int),
                ("ns_flags", c_int), ("nbuf", c_int), ("per_split", c_int), ("t1", c_int), ("t2", c_int), ("splits", c_int),
                ("swap_operands", c_int), ("fold", c_int), ("fold_grid", c_int), ("partials_need", c_long)]


class AttnPlan(C.Structure):
    _fields_ = [("family", c_int), ("tp", c_int * 4), ("grid", c_int), ("block", c_int), ("lds", c_int), ("nq_chunks", c_int), ("q_per_wg", c_int)]


class MlpPlan(C.Structure):
    _fields_ = [("family", c_int), ("tp", c_int * 2), ("grid", c_int), ("block", c_int), ("lds", c_int), ("m_per_split", c_int), ("splits", c_int), ("ny", c_int),
                ("fold", c_int), ("fold_grid", c_int * 2), ("partials_need", c_long)]


PLAN_STRUCTS = (("mvlt_gemm_plan", GemmPlan), ("mvlt_attn_plan", AttnPlan), ("mvlt_mlp_plan", MlpPlan))
PLAN_PROTOTYPES = {
    "mvlt_plan_version": (_i, []),
    "mvlt_gemm_nt_plan": (_i, [C.POINTER(GemmNTArgs), C.POINTER(GemmPlan)]),
    "mvlt_gemm_tn_plan": (_i, [C.POINTER(GemmTNArgs), C.POINTER(GemmPlan)]),
    "mvlt_gemm_plan_name": (_i, [C.POINTER(GemmPlan), _str, C.c_size_t]),
    "mvlt_gemm_plan_sizeof": (_i, []),
    "mvlt_sr_attention_fwd_plan": (_i, [C.POINTER(AttnArgs), _i, C.POINTER(AttnPlan)]),
    "mvlt_sr_attention_bwd_plan": (_i, [C.POINTER(AttnBwdArgs), _i, C.POINTER(AttnPlan)]),
    "mvlt_attn_plan_name": (_i, [C.POINTER(AttnPlan), _str, C.c_size_t]),
    "mvlt_attn_plan_sizeof": (_i, []),
    "mvlt_mlp_fwd_plan": (_i, [C.POINTER(MlpArgs), C.POINTER(MlpPlan)]),
    "mvlt_mlp_bwd_dx_plan": (_i, [C.POINTER(MlpArgs), C.POINTER(MlpPlan)]),
    "mvlt_mlp_bwd_dw_plan": (_i, [C.POINTER(MlpArgs), C.POINTER(MlpPlan)]),
    "mvlt_mlp_plan_name": (_i, [C.POINTER(MlpPlan), _str, C.c_size_t]),
    "mvlt_mlp_plan_sizeof": (_i, []),
}
for _name, (_res, _args) in PLAN_PROTOTYPES.items():
    if not hasattr(lib, _name):
        raise ImportError(f"{LIB_PATH} does not export {_name} (include/mvlt_hip_plan.h): stale build? run python -m mvlt_amd.build")
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

PLAN_VERSION = 3         # include/mvlt_hip_plan.h MVLT_PLAN_VERSION this binding was written against
_plan_sizes = [(n, getattr(lib, n + "_sizeof")(), C.sizeof(c)) for n, c in PLAN_STRUCTS]
if lib.mvlt_plan_version() != PLAN_VERSION or any(have != want for _, have, want in _plan_sizes):
    raise ImportError(f"plan entry points mismatch: {LIB_PATH} is version {lib.mvlt_plan_version()}, the binding is version {PLAN_VERSION}; (struct, bytes in the library, "
                      f"bytes in the binding): {_plan_sizes} (stale build? run python -m mvlt_amd.build)")

# The entry points of include/mvlt_hip_opt.h (AdamW with a learning rate and a weight decay per parameter group, docs/param_groups.md): a table of their own,
# bound and version-checked like the EMA one (tests/test_param_groups_cpu.py compares it with that header).
OPT_PROTOTYPES = {
    "mvlt_opt_version": (_i, []),
    "mvlt_adamw_step_groups": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _i, _vp, _vp, _vp]),      # table: a DEVICE array of float[n_groups][2]
}
for _name, (_res, _args) in OPT_PROTOTYPES.items():
    if not hasattr(lib, _name):
        raise ImportError(f"{LIB_PATH} does not export {_name} (include/mvlt_hip_opt.h): stale build? run python -m mvlt_amd.build")
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

OPT_VERSION = 1          # include/mvlt_hip_opt.h MVLT_OPT_VERSION this binding was written against
if lib.mvlt_opt_version() != OPT_VERSION:
    raise ImportError(f"optimizer entry points mismatch: {LIB_PATH} is version {lib.mvlt_opt_version()}, the binding is version {OPT_VERSION} (stale build? run python -m mvlt_amd.build)")

# The entry points of include/mvlt_hip_lamb.h (LAMB: layer-wise trust ratios over the flat store in three launches, docs/lamb.md): a table of their own,
# bound and version-checked like the one above (tests/test_lamb_cpu.py compares it with that header).
LAMB_PROTOTYPES = {
    "mvlt_lamb_version": (_i, []),
    "mvlt_lamb_check_tables": (_i, [_vp, _i, _vp, _i, _l, _i]),                                          # both tables: HOST arrays
    "mvlt_lamb_moments": (_i, [_vp, _vp, _vp, _vp, _l, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),    # tensors / chunks: DEVICE arrays from here on
    "mvlt_lamb_fold": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "mvlt_lamb_apply": (_i, [_vp, _vp, _vp, _vp, _l, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp]),
}
for _name, (_res, _args) in LAMB_PROTOTYPES.items():
    if not hasattr(lib, _name):
        raise ImportError(f"{LIB_PATH} does not export {_name} (include/mvlt_hip_lamb.h): stale build? run python -m mvlt_amd.build")
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

LAMB_VERSION = 1         # include/mvlt_hip_lamb.h MVLT_LAMB_VERSION this binding was written against
if lib.mvlt_lamb_version() != LAMB_VERSION:
    raise ImportError(f"LAMB entry points mismatch: {LIB_PATH} is version {lib.mvlt_lamb_version()}, the binding is version {LAMB_VERSION} (stale build? run python -m mvlt_amd.build)")

# The entry points of include/mvlt_hip_loss.h (cross entropy with label smoothing and class weights, docs/loss_options.md): a table of their own, bound and
# version-checked like the one above (tests/test_loss_cpu.py compares it with that header).
LOSS_PROTOTYPES = {
    "mvlt_loss_version": (_i, []),
    "mvlt_ce_smooth_fwd": (_i, [_vp, _vp, _l, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlt_ce_smooth_bwd": (_i, [_vp, _vp, _l, _f, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
}
for _name, (_res, _args) in LOSS_PROTOTYPES.items():
    if not hasattr(lib, _name):
        raise ImportError(f"{LIB_PATH} does not export {_name} (include/mvlt_hip_loss.h): stale build? run python -m mvlt_amd.build")
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

LOSS_VERSION = 1         # include/mvlt_hip_loss.h MVLT_LOSS_VERSION this binding was written against
if lib.mvlt_loss_version() != LOSS_VERSION:
    raise ImportError(f"loss entry points mismatch: {LIB_PATH} is version {lib.mvlt_loss_version()}, the binding is version {LOSS_VERSION} (stale build? run python -m mvlt_amd.build)")

# The entry points of include/mvlt_hip_ingest.h (uint8 pixels in, resized / flipped / grid-masked fp32 out, docs/ingest.md): a table of their own, bound and
# version-checked like the one above (tests/test_ingest_cases_cpu.py compares it with that header).
INGEST_PROTOTYPES = {
    "mvlt_ingest_version": (_i, []),
    "mvlt_image_ingest": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "mvlt_image_ingest_resize": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),      # rects_host (parameter 4): a HOST array
    "mvlt_flip_flags": (_i, [_vp, _i, _f, _u64, _u64, _vp]),
}
for _name, (_res, _args) in INGEST_PROTOTYPES.items():
    if not hasattr(lib, _name):
        raise ImportError(f"{LIB_PATH} does not export {_name} (include/mvlt_hip_ingest.h): stale build? run python -m mvlt_amd.build")
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

INGEST_VERSION = 1       # include/mvlt_hip_ingest.h MVLT_INGEST_VERSION this binding was written against
if lib.mvlt_ingest_version() != INGEST_VERSION:
    raise ImportError(f"ingest entry points mismatch: {LIB_PATH} is version {lib.mvlt_ingest_version()}, the binding is version {INGEST_VERSION} (stale build? run python -m mvlt_amd.build)")

DT = {torch.bfloat16: 0, torch.float32: 1}


def last_kernel():
    """name of the kernel instantiation launched last on this thread, e.g. "mlp_wgrad2_kernel<64, 4>" (the runtime's name for the launched
    function, demangled; return type, namespace and parameter list stripped)"""
    s = lib.mvlt_last_kernel().decode()
    s = s.replace("(anonymous namespace)::", "")
    if s.startswith("void "):
        s = s[5:]
    depth = 0
    for i, ch in enumerate(s):                   # cut at the '(' that opens the parameter list (outside the template brackets)
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def check(rc, what):
    if rc != 0:
        raise MVLTError(f"{what} failed ({rc}): {lib.mvlt_last_error().decode()}")


_raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice


def stream_ptr():
    """torch's current stream of the current device as a hipStream_t (two C calls: `torch.cuda.current_stream().cuda_stream` walks ~10 Python frames and
    builds a Stream object -- 358 launches per step made that 2.5 ms of a 10 ms host step, tools/host_profile.py)"""
    return _raw_stream(_cur_device())


def ptr(t):
    """the one way a tensor becomes an argument: its device address as a plain int (the c_void_p argtypes and struct fields convert it), None for None"""
    if t is None:
        return None
    if not t.is_cuda:
        raise MVLTError("mvlt_amd ops need CUDA/HIP tensors (no CPU fallback)")
    return t.data_ptr()


def rowmap(rows_per_batch=0, batch_stride=0, offset=0):
    return RowMap(0, rows_per_batch, batch_stride, offset, 0, 0, 0, 0, 0, 0, 0)


def patchmap(r, w_in, tokens_in, hw_out, w_out, c_seg):
    return RowMap(1, 0, 0, 0, r, w_in, tokens_in, hw_out, w_out, c_seg, 0)


def conv3map(h, w, tokens_in, c_seg):
    """3x3 / pad 1 neighbourhood gather over an h x w pixel grid stored pixel-major with `tokens_in` rows per batch"""
    return RowMap(2, 0, 0, 0, 3, w, tokens_in, h * w, w, c_seg, h)

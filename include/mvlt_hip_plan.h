/* mvlt_hip_plan.h -- what mvlt_gemm_nt / mvlt_gemm_tn, the mvlt_sr_attention_* and the mvlt_mlp_* entry points WOULD launch for an argument struct, without launching it: entry points of libmvlt_hip.so added
 * beside the C ABI of mvlt_hip.h (version 8) and the additions of mvlt_hip_ext.h and mvlt_hip_ema.h, whose lists of prototypes and versions stay as they are.
 *
 * The GEMM, the SR-attention and the fused-MLP entry points are "plan, then launch": the plan -- argument checks, choice of kernel instantiation, launch geometry, trailing kernel
 * arguments, partial-tile bookkeeping -- is a pure host function (mvlt_amd/csrc/gemm_plan.h, attn_plan.h, mlp_plan.h: no HIP call, no global state), and the entry points below
 * hand it out.  They touch no device: they run on a machine without a GPU, and tests/test_gemm_plan_cpu.py / tests/test_attn_plan_cpu.py / tests/test_mlp_plan_cpu.py pin them against recorded launches.
 * A binding compares mvlt_plan_version() with the MVLT_PLAN_VERSION it was written against (mvlt_amd/_lib.py PLAN_VERSION) before it calls anything here.
 */
#ifndef MVLT_HIP_PLAN_H
#define MVLT_HIP_PLAN_H
#include <stddef.h>
#include "mvlt_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: bumped whenever a signature or the struct below changes.
 *   1: mvlt_gemm_plan, mvlt_gemm_nt_plan(), mvlt_gemm_tn_plan(), mvlt_gemm_plan_name(), mvlt_gemm_plan_sizeof()
 *   2: + mvlt_attn_plan, mvlt_sr_attention_fwd_plan(), mvlt_sr_attention_bwd_plan(), mvlt_attn_plan_name(), mvlt_attn_plan_sizeof()
 *   3: + mvlt_mlp_plan, mvlt_mlp_fwd_plan(), mvlt_mlp_bwd_dx_plan(), mvlt_mlp_bwd_dw_plan(), mvlt_mlp_plan_name(), mvlt_mlp_plan_sizeof() */
#define MVLT_PLAN_VERSION 3
int mvlt_plan_version(void);

/* kernel families of the GEMMs (mvlt_amd/csrc/gemm_<family>.hip, dispatched by gemm.hip); tp[] holds the template arguments of the instantiation in the order the kernel declares them
 * (bool as 0 / 1, an element type as its dtype code) */
#define MVLT_GEMM_NONE 0        /* M == 0: nothing to launch */
#define MVLT_GEMM_NT_F32 1      /* gemm_nt_kernel<float, BN>                           tp = {BN} */
#define MVLT_GEMM_NT_DMA 2      /* gemm_nt_dma_kernel<BN, AMODE, EPI, BK, 128>         tp = {BN, AMODE, EPI, BK} */
#define MVLT_GEMM_NT_P8 3       /* gemm_nt_p8_kernel<EPI, HM, HN0, HN1, RAG>           tp = {EPI, HM, HN0, HN1, RAG} */
#define MVLT_GEMM_NT_CONV3 4    /* conv3_nt_kernel<W, BN, EPI>                         tp = {W, BN, EPI} */
#define MVLT_GEMM_TN_PLAIN 5    /* gemm_tn_kernel<T, BN>                               tp = {dtype, BN} */
#define MVLT_GEMM_TN_DMA 6      /* gemm_tn_dma_kernel<BMT, BN, BMODE, NS, DG>          tp = {BMT, BN, BMODE, NS, DG} */
#define MVLT_GEMM_TN_P8 7       /* gemm_tn_p8_kernel<HM, HN0, HN1, TRANS, RAG1, SWAP>  tp = {HM, HN0, HN1, TRANS, RAG1, SWAP} */
#define MVLT_GEMM_TN_CONV3 8    /* conv3_wgrad_kernel<W>                               tp = {W} */

typedef struct mvlt_gemm_plan {
  int family;                /* MVLT_GEMM_* */
  int tp[6];
  int grid[3];
  int block;
  int lds;                   /* dynamic LDS bytes */
  /* the scalar kernel arguments behind the argument struct, as each family uses them (0 where it has none) */
  int ns_flags;              /* NT_DMA: ring depth | 0x100 (early slot release) */
  int nbuf;                  /* NT_F32 */
  int per_split;             /* TN_PLAIN / TN_DMA: m_per_split (rows);  TN_P8: kt_per (64-row k-tiles);  TN_CONV3: tiles_per_split */
  int t1, t2;                /* TN_DMA / TN_P8: output tiles along N1 / N2 of the kernel's operands;  TN_CONV3: n_o, n_c (64-wide blocks of outputs / input channels) */
  int splits;                /* TN: m-splits */
  int swap_operands;         /* TN_P8 on 192 x 320 tiles when the 320-multiple side is the caller's N1: the kernel gets A and B (with their strides, sizes and column sums) exchanged */
  int fold;                  /* 1: the splits store bf16 partial tiles to the caller's scratch and an ordered fold adds them to C */
  int fold_grid;             /* workgroups of that fold (256 threads each) */
  long partials_need;        /* bytes of mvlt_gemm_tn_args.partials this launch takes; 0 = atomics or a plain store */
} mvlt_gemm_plan;

/* Argument checks + choice, exactly what mvlt_gemm_nt / mvlt_gemm_tn do before they launch: same return codes, same mvlt_last_error() texts.  Pointers are
 * looked at (null or not, low four address bits, equality), never followed. */
int mvlt_gemm_nt_plan(const mvlt_gemm_nt_args* args, mvlt_gemm_plan* plan);
int mvlt_gemm_tn_plan(const mvlt_gemm_tn_args* args, mvlt_gemm_plan* plan);
/* the planned kernel's name as mvlt_last_kernel() prints it, without return type, namespace and parameter list: "gemm_nt_p8_kernel<1, 3, 3, 2, true>"
 * ("" for MVLT_GEMM_NONE).  Returns the length written, <0 when buf is too small or the family unknown. */
int mvlt_gemm_plan_name(const mvlt_gemm_plan* plan, char* buf, size_t n);
int mvlt_gemm_plan_sizeof(void);

/* kernel families of SR-attention (mvlt_amd/csrc/attention_<family>.hip, dispatched by attention.hip); tp[] as above */
#define MVLT_ATTN_FWD 1         /* attn_fwd_kernel<T, NKT>                  tp = {dtype, NKT}          resident forward: fp32, and bf16 past 192 keys */
#define MVLT_ATTN_FWD2 2        /* attn_fwd2_kernel<NKT, PADDED, NW>        tp = {NKT, PADDED, NW}     resident bf16 forward up to 192 keys */
#define MVLT_ATTN_BWD 3         /* attn_bwd_kernel<T, NW, TPW>              tp = {dtype, NW, TPW}      resident fp32 backward */
#define MVLT_ATTN_BWD_DMA 4     /* attn_bwd_dma_kernel<NW, TPW>             tp = {NW, TPW}             resident bf16 backward */
#define MVLT_ATTN_FWD_STREAM 5  /* attn_fwd_stream_kernel<T, KB>            tp = {dtype, KB}           key-streamed forward, any M */
#define MVLT_ATTN_BWD_STREAM 6  /* attn_bwd_stream_kernel<T, NW, TPW>       tp = {dtype, NW, TPW}      key-streamed backward, any M */

typedef struct mvlt_attn_plan {
  int family;                /* MVLT_ATTN_* */
  int tp[4];
  int grid;                  /* workgroups (x) */
  int block;
  int lds;                   /* dynamic LDS bytes */
  int nq_chunks;             /* query chunks per (batch, head): the kernels' first scalar argument */
  int q_per_wg;              /* queries per chunk: their second (the streamed forward's is the constant 128 and no kernel argument) */
} mvlt_attn_plan;

/* Argument checks + choice, exactly what mvlt_sr_attention_fwd / _bwd (streamed == 0) and mvlt_sr_attention_fwd_streamed / _bwd_streamed (streamed != 0) do before they
 * launch: same return codes, same mvlt_last_error() texts.  Pointers are tested for null, never followed.  mvlt_sr_attention_bwd_chunks() is nq_chunks of the backward plan
 * for an fp32 dKV. */
int mvlt_sr_attention_fwd_plan(const mvlt_attn_args* args, int streamed, mvlt_attn_plan* plan);
int mvlt_sr_attention_bwd_plan(const mvlt_attn_bwd_args* args, int streamed, mvlt_attn_plan* plan);
/* as mvlt_gemm_plan_name: "attn_bwd_dma_kernel<4, 3>" */
int mvlt_attn_plan_name(const mvlt_attn_plan* plan, char* buf, size_t n);
int mvlt_attn_plan_sizeof(void);

/* kernel families of the fused MLP of stages 1-2 (mvlt_amd/csrc/mlp_<family>.hip, dispatched by mlp.hip); tp[] as above */
#define MVLT_MLP_NONE 0         /* M <= 0: nothing to launch */
#define MVLT_MLP_FUSED 1        /* mlp_fused_kernel<C, MODE>                tp = {C, MODE}             forward (MODE 0) / input gradient (1) with a pre-activation output or hid == 64 */
#define MVLT_MLP_PIPE 2         /* mlp_pipe_kernel<C, MODE>                 tp = {C, MODE}             software-pipelined forward / input gradient: every other launch */
#define MVLT_MLP_WGRAD 3        /* mlp_wgrad_kernel<C>                      tp = {C}                   weight gradients, DropPath factor per row (rows_per_scale no multiple of 64) */
#define MVLT_MLP_WGRAD2 4       /* mlp_wgrad2_kernel<C, NW>                 tp = {C, NW}               weight gradients, factor per 64-token tile (or none) */

typedef struct mvlt_mlp_plan {
  int family;                /* MVLT_MLP_* */
  int tp[2];
  int grid;                  /* workgroups (x) */
  int block;
  int lds;                   /* dynamic LDS bytes */
  /* the weight-gradient launches (0 elsewhere): the scalar kernel arguments behind the argument struct ... */
  int m_per_split;           /* token rows per split: whole 64-token tiles */
  int splits;                /* token splits */
  int ny;                    /* 128-unit blocks of the hidden dimension */
  /* ... and where dW1 / dW2 leave to */
  int fold;                  /* WGRAD2.  1: the splits store bf16 partial tiles to the caller's scratch and two ordered folds add them to dw1 / dw2;  0: fp32 atomics */
  int fold_grid[2];          /* workgroups of those folds (256 threads each); 0 without them */
  long partials_need;        /* WGRAD2: bytes of mvlt_mlp_args.partials the partial tiles of both gradients take, 2 * splits * hid * C * 2 */
} mvlt_mlp_plan;

/* Argument checks + choice, exactly what mvlt_mlp_fwd / mvlt_mlp_bwd_dx / mvlt_mlp_bwd_dw do before they launch: same return codes, same mvlt_last_error() texts.  Pointers
 * are looked at (null or not, low four address bits), never followed.  Beyond what the launching entry points refused before this header's version 3: a plan whose dynamic
 * LDS exceeds 160 KB or whose grid exceeds INT_MAX is MVLT_ERR_ARG with a text naming the size. */
int mvlt_mlp_fwd_plan(const mvlt_mlp_args* args, mvlt_mlp_plan* plan);
int mvlt_mlp_bwd_dx_plan(const mvlt_mlp_args* args, mvlt_mlp_plan* plan);
int mvlt_mlp_bwd_dw_plan(const mvlt_mlp_args* args, mvlt_mlp_plan* plan);
/* as mvlt_gemm_plan_name: "mlp_wgrad2_kernel<64, 4>" ("" for MVLT_MLP_NONE) */
int mvlt_mlp_plan_name(const mvlt_mlp_plan* plan, char* buf, size_t n);
int mvlt_mlp_plan_sizeof(void);

#ifdef __cplusplus
}
#endif
#endif

// MFMA GEMMs for the MVLT hot path (gfx950 / CDNA4, wave64).
//
//  mvlt_gemm_nt : C[M,N] = epilogue(A[M,K] . B[N,K]^T)      Linear forward / dgrad (with W^T) and the
//                 kernel==stride convolutions (PatchEmbed, Attention.sr) as gathered-row GEMMs.
//                 Replaces F.linear / nn.Conv2d call sites of reference libs/pvlt.py:66-69,98,104,108,118,168
//                 and libs/vl_heads.py:31,67,85,102.
//  mvlt_gemm_tn : C[N1,N2] += A[M,N1]^T . B[M,N2]  (fp32 atomics)   weight gradients (+ fused bias gradient).
//
// Tiling: 256 threads = 4 waves (2x2), block tile 128 x BN (BN = 128 or 64), wave tile 64 x BN/2 built from
// v_mfma_f32_16x16x32_bf16 (bf16) or 8 x v_mfma_f32_16x16x4_f32 (fp32: exact-f32 path for the 1e-3 parity bar).
// LDS rows are 128 B (64 bf16 / 32 fp32 of K) = 8 x 16-B chunks, XOR-swizzled by row so the ds_read_b128
// fragment reads are conflict-free; global->register->LDS staging is double-buffered (one barrier per K tile).
//
// One translation unit per kernel family, compiled in parallel: gemm_nt_dma.hip (register-staged + LDS-DMA NT), gemm_nt_p8.hip (8-phase NT), gemm_tn_dma.hip
// (register-staged + LDS-DMA TN, dgrad variant), gemm_tn_p8.hip (8-phase TN), gemm_conv3.hip (conv3x3 forward / dgrad and weight gradient); gemm_common.h holds
// what more than one of them uses.  This file keeps the partial-tile folds, the dispatch of a plan to its family's launch function and the C entry points.
#include "gemm_common.h"
#include <map>
#include <mutex>

namespace {

// ---- deferred folds (mvlt_gemm_tn_args.defer_fold): a fold is a ~8 us memory-bound launch between two long MFMA-bound ones (30 per step, 2.5 TB/s).  A deferring caller's
// partial tiles stay in its scratch -- each launch takes the next free region -- and up to FOLD_MAX of them are folded by ONE launch of tn_fold_multi_kernel: when the table or
// the scratch is full, when a non-deferring launch wants the scratch, or when the caller says mvlt_tn_fold_flush (before anything reads the gradients).  Same stream throughout.
constexpr int FOLD_MAX = 32;
struct FoldDesc { const bf16* part; float* C; int splits, N1, N2, ldc, wg0; };
struct FoldBatch { FoldDesc d[FOLD_MAX]; int n, total_wgs; };

// C[n1][n2] += sum over the splits of part[split][n1][n2] (bf16 partial tiles of gemm_tn_p8_kernel / gemm_tn_dma_kernel).  A workgroup covers 32 groups of eight consecutive n2;
// its 256 threads are 32 groups x 8 split subsets (a 320 x 320 output over 56 splits is only 12800 groups: one thread per group left 200 CUs idle and ran the 56 loads of a
// group one behind the other), the subsets meet in LDS and are added in a FIXED order: the result does not depend on timing.
__device__ __forceinline__ void tn_fold_body(const bf16* __restrict__ part, int splits, int N1, int N2, float* __restrict__ C, int ldc, int blk) {
  __shared__ float red[8][32][9];
  const int eg = threadIdx.x & 31, sk = threadIdx.x >> 5;
  const long g = (long)blk * 32 + eg;
  const long per = (long)N1 * N2;
  const bool ok = g * 8 < per;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    for (int z = sk; z < splits; z += 8) {
      const bf16x8 v = __builtin_bit_cast(bf16x8, ld_g<MVLT_NT_LD>((const u32x4*)(part + (size_t)z * per + g * 8)));
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[sk][eg][e] = s[e];
  __syncthreads();
  if (sk == 0 && ok) {
#pragma unroll
    for (int k = 1; k < 8; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += red[k][eg][e];
    const int n1 = (int)((g * 8) / N2), n2 = (int)((g * 8) - (long)n1 * N2);
    float* dst = C + (long)n1 * ldc + n2;
    const f32x4 a = *(const f32x4*)dst, b = *(const f32x4*)(dst + 4);
    *(f32x4*)dst = f32x4{a[0] + s[0], a[1] + s[1], a[2] + s[2], a[3] + s[3]};
    *(f32x4*)(dst + 4) = f32x4{b[0] + s[4], b[1] + s[5], b[2] + s[6], b[3] + s[7]};
  }
}

__global__ __launch_bounds__(256) void tn_fold_kernel(const bf16* __restrict__ part, int splits, int N1, int N2, float* __restrict__ C, int ldc) {
  tn_fold_body(part, splits, N1, N2, C, ldc, blockIdx.x);
}
// several folds in one launch: workgroup b belongs to the descriptor whose [wg0, next wg0) holds it
__global__ __launch_bounds__(256) void tn_fold_multi_kernel(FoldBatch b) {
  int i = 0;
#pragma unroll 1
  for (int k = 1; k < b.n; ++k) if ((int)blockIdx.x >= b.d[k].wg0) i = k;
  const FoldDesc& d = b.d[i];
  tn_fold_body(d.part, d.splits, d.N1, d.N2, d.C, d.ldc, (int)blockIdx.x - d.wg0);
}

// One pending table PER SCRATCH (= per owner: a FlatStore holds one scratch; ADVICE r5 -- a single process-global table let the start of one model's backward pass discard another
// model's pending folds, and a launch on another stream reused the scratch while the old stream's fold still read it).  The map and its tables are guarded by g_fold_mu; the launches
// themselves are asynchronous, so the lock is held for table bookkeeping + one enqueue.
struct FoldPending {
  FoldBatch b = {};
  long used = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;                         // recorded behind a fold when ANOTHER stream is about to reuse the scratch / read the gradients
};
std::mutex g_fold_mu;
std::map<const void*, FoldPending> g_fold;         // key: mvlt_gemm_tn_args.partials
int fold_wgs(const FoldDesc& d) { return (int)(((long)d.N1 * d.N2 / 8 + 31) / 32); }
// fold what is pending in `f` on the stream its producers ran on; `reader` (if it is another stream) is made to wait for that fold
void fold_flush_locked(FoldPending& f, hipStream_t reader, bool order_reader) {
  if (f.b.n > 0) {
    f.b.total_wgs = f.b.d[f.b.n - 1].wg0 + fold_wgs(f.b.d[f.b.n - 1]);
    MVLT_LAUNCH(tn_fold_multi_kernel, dim3((unsigned)f.b.total_wgs), dim3(256), 0, f.stream, f.b);
    if (order_reader && reader != f.stream) {
      if (!f.ev) (void)hipEventCreateWithFlags(&f.ev, hipEventDisableTiming);
      if (f.ev && hipEventRecord(f.ev, f.stream) == hipSuccess) (void)hipStreamWaitEvent(reader, f.ev, 0);
    }
  }
  f.b.n = 0;
  f.used = 0;
}
// the scratch region of this launch's partial tiles, or nullptr when they do not fit
bf16* fold_acquire(const mvlt_gemm_tn_args& a, long need, hipStream_t s, int room = 1) {
  if (!a.partials || ((uintptr_t)a.partials & 15) || need > a.partials_bytes) return nullptr;
  std::lock_guard<std::mutex> lk(g_fold_mu);
  FoldPending& f = g_fold[a.partials];
  bool flush = f.b.n > 0 && (!a.defer_fold || f.stream != s || f.b.n + room > FOLD_MAX || f.used + need > a.partials_bytes);
  // two pending folds into the same gradient would be two unordered read-modify-writes in one launch (the kv weight gradient takes its text rows and its image rows from two
  // GEMMs): an output that overlaps a pending one folds the pending ones first
  const float* c_lo = a.C;
  const float* c_hi = a.C + (size_t)(a.N1 - 1) * a.ldc + a.N2;
  for (int i = 0; i < f.b.n && !flush; ++i) {
    const FoldDesc& d = f.b.d[i];
    const float* d_lo = d.C;
    const float* d_hi = d.C + (size_t)(d.N1 - 1) * d.ldc + d.N2;
    if (c_lo < d_hi && d_lo < c_hi) flush = true;
  }
  if (flush) fold_flush_locked(f, s, true);        // a launch on another stream writes region 0 only behind the old stream's fold
  f.stream = s;
  if (!a.defer_fold) return (bf16*)a.partials;
  return (bf16*)((char*)a.partials + f.used);
}
void fold_launch(const mvlt_gemm_tn_args& a, const bf16* part, int splits, hipStream_t s) {
  const long groups = (long)a.N1 * a.N2 / 8;
  if (!a.defer_fold) {
    MVLT_LAUNCH(tn_fold_kernel, dim3((unsigned)((groups + 31) / 32)), dim3(256), 0, s, part, splits, a.N1, a.N2, a.C, a.ldc);
    return;
  }
  std::lock_guard<std::mutex> lk(g_fold_mu);
  FoldPending& f = g_fold[a.partials];
  FoldDesc& d = f.b.d[f.b.n];
  d.part = part; d.C = a.C; d.splits = splits; d.N1 = a.N1; d.N2 = a.N2; d.ldc = a.ldc;
  d.wg0 = f.b.n == 0 ? 0 : f.b.d[f.b.n - 1].wg0 + fold_wgs(f.b.d[f.b.n - 1]);
  ++f.b.n;
  f.used += ((long)splits * a.N1 * a.N2 * 2 + 255) & ~255L;
}

// ------------------------------------------------------------------------------------------------ plan -> launch
// What to launch is decided in gemm_plan.h; which instantiation a plan's template arguments name is the family file's case list (gemm_common.h declares the launch
// functions).  Here a plan goes to its family, nothing else: an unknown family is an error, never another kernel.
int launch_nt(const mvlt_gemm_plan& p, const mvlt_gemm_nt_args& a, hipStream_t s) {
  switch (p.family) {
    case MVLT_GEMM_NT_F32:
    case MVLT_GEMM_NT_DMA: return mvlt_launch_nt_dma(p, a, s);
    case MVLT_GEMM_NT_P8: return mvlt_launch_nt_p8(p, a, s);
    case MVLT_GEMM_NT_CONV3: return mvlt_launch_nt_conv3(p, a, s);
  }
  return no_instantiation("mvlt_gemm_nt", p);
}

int launch_tn(const mvlt_gemm_plan& p, const mvlt_gemm_tn_args& a, hipStream_t s) {
  const char* const who = "mvlt_gemm_tn";
  mvlt_gemm_tn_args k = a;                    // what the kernel sees: the caller's operands, or (192 x 320 tiles with the 320 side on N1) exchanged
  if (p.swap_operands) {
    k.A = a.B; k.B = a.A; k.lda = a.ldb; k.ldb = a.lda; k.N1 = a.N2; k.N2 = a.N1;
    k.colsum_a = a.colsum_b; k.colsum_b = a.colsum_a;
  }
  // [splits][caller N1][caller N2] bf16 in the caller's scratch; the plan has checked everything the bookkeeping can refuse on
  bf16* const part = p.fold ? fold_acquire(a, p.partials_need, s) : nullptr;
  if (p.fold && !part) { mvlt_set_error("%s: the planned %ld bytes of partial tiles do not fit the scratch", who, p.partials_need); return MVLT_ERR_ARG; }
  auto launch = [&]() -> int {
    switch (p.family) {
      case MVLT_GEMM_TN_PLAIN:
      case MVLT_GEMM_TN_DMA: return mvlt_launch_tn_dma(p, k, part, s);
      case MVLT_GEMM_TN_P8: return mvlt_launch_tn_p8(p, k, part, s);
      case MVLT_GEMM_TN_CONV3: return mvlt_launch_tn_conv3(p, k, part, s);
    }
    return no_instantiation(who, p);
  };
  // the fold (a launch, or an entry of the pending table) follows its producer on the same stream
  const int e = launch();
  if (e != MVLT_OK || !p.fold) return e;
  fold_launch(a, part, p.splits, s);
  return mvlt_check_launch(who);
}
}  // namespace

extern "C" int mvlt_gemm_nt(const mvlt_gemm_nt_args* a, void* stream) {
  mvlt_gemm_plan p;
  MVLT_REQUIRE(a, "mvlt_gemm_nt: null operand");
  if (int e = plan_gemm_nt(*a, p)) return e;
  return p.family == MVLT_GEMM_NONE ? MVLT_OK : launch_nt(p, *a, (hipStream_t)stream);
}

extern "C" int mvlt_gemm_tn(const mvlt_gemm_tn_args* a, void* stream) {
  mvlt_gemm_plan p;
  MVLT_REQUIRE(a, "mvlt_gemm_tn: null operand");
  if (int e = plan_gemm_tn(*a, p)) return e;
  return p.family == MVLT_GEMM_NONE ? MVLT_OK : launch_tn(p, *a, (hipStream_t)stream);
}

// the plan without the launch (include/mvlt_hip_plan.h): no device is touched
extern "C" int mvlt_plan_version(void) { return MVLT_PLAN_VERSION; }
extern "C" int mvlt_gemm_plan_sizeof(void) { return (int)sizeof(mvlt_gemm_plan); }
extern "C" int mvlt_gemm_nt_plan(const mvlt_gemm_nt_args* a, mvlt_gemm_plan* plan) {
  MVLT_REQUIRE(a && plan, "mvlt_gemm_nt_plan: null argument");
  return plan_gemm_nt(*a, *plan);
}
extern "C" int mvlt_gemm_tn_plan(const mvlt_gemm_tn_args* a, mvlt_gemm_plan* plan) {
  MVLT_REQUIRE(a && plan, "mvlt_gemm_tn_plan: null argument");
  return plan_gemm_tn(*a, *plan);
}
extern "C" int mvlt_gemm_plan_name(const mvlt_gemm_plan* plan, char* buf, size_t n) {
  MVLT_REQUIRE(plan && buf && n > 0, "mvlt_gemm_plan_name: null argument");
  return plan_kernel_name(*plan, buf, n);
}

bf16* mvlt_fold_acquire_ext(const mvlt_gemm_tn_args& a, long need, hipStream_t s, int descriptors) { return fold_acquire(a, need, s, descriptors); }
void mvlt_fold_launch_ext(const mvlt_gemm_tn_args& a, const bf16* part, int splits, hipStream_t s) { fold_launch(a, part, splits, s); }

extern "C" int mvlt_tn_fold_discard(const void* partials) {
  // forget the pending folds of one scratch (NULL: of every scratch) without launching anything: their producers belong to a pass that was abandoned
  std::lock_guard<std::mutex> lk(g_fold_mu);
  for (auto& kv : g_fold)
    if (!partials || kv.first == partials) { kv.second.b.n = 0; kv.second.used = 0; }
  return MVLT_OK;
}

extern "C" int mvlt_tn_fold_flush(const void* partials, void* stream) {
  // the pending folds run on the stream their producers ran on; `stream` -- the stream of whoever reads the gradients next -- waits for them when it is another one
  std::lock_guard<std::mutex> lk(g_fold_mu);
  for (auto& kv : g_fold)
    if (!partials || kv.first == partials) fold_flush_locked(kv.second, (hipStream_t)stream, true);
  return mvlt_check_launch("mvlt_tn_fold_flush");
}

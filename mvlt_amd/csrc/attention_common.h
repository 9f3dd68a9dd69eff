// What more than one SR-attention translation unit uses (attention.hip and one attention_<family>.hip per kernel family; the overview is at the top of attention.hip).
// First part, plain C++ (attn_plan.h includes it under a host compiler alone): the sizes both the plan and the kernels are built on -- above all the dynamic LDS bytes
// of every instantiation as constexpr functions of its template arguments; each kernel static_asserts its own carve-up of `smem` against them.  Second part (HIP only):
// fragments, MFMA wrappers, the swizzled tile layout, and the per-family launch functions attention.hip calls across the files.
#pragma once
#include <stddef.h>

namespace mvlt_attn {

constexpr int NT = 256;                         // threads of the 4-wave kernels
constexpr int HD = 64;                          // head dimension
constexpr int STREAM_QPW = 128;                 // queries per workgroup of both streamed kernels (bwd: the fp32 dQ tile in LDS)
constexpr int DQS = HD + 4;                     // row stride of the streamed backward's fp32 dQ tile (floats)
// key block of the streamed kernels by element size `es` (2: bf16, 4: fp32): 33 / 34 KB per ring slot of the forward; backward blocks of 16 NW TPW = 128 / 64 keys
constexpr int stream_kb_fwd(int es) { return es == 2 ? 128 : 64; }
constexpr int stream_bwd_tpw(int es) { return es == 2 ? 2 : 1; }
constexpr int STREAM_BWD_NW = 4;

// ---- dynamic LDS bytes.  MP / KB = padded keys, es = element size, 16 / es = the 16 bytes of padding per transposed row
constexpr size_t fwd_lds(int es, int nkt) { return (size_t)(nkt * 32 * HD + HD * (nkt * 32 + 4)) * es; }                          // K [MP][64] | V^T [64][MP + 4]
constexpr size_t fwd2_lds(int nkt, int nw) { return (size_t)(nkt * 32 * HD + HD * (nkt * 32 + 8)) * 2 + nw * 4096 + nw * 2304; }   // K | V^T [64][MP + 8] | Q tiles | O staging
constexpr size_t bwd_tiles_lds(int es, int keys) {                                                                                // K^T [64][keys + pad] | dS [32][..] | Q^T, dO^T [64][32 + pad]
  return (size_t)(HD * (keys + 16 / es) + 32 * (keys + 16 / es) + 2 * HD * (32 + 16 / es)) * es;
}
constexpr size_t bwd_lds(int es, int nw, int tpw) { return bwd_tiles_lds(es, nw * tpw * 16) + 64 * sizeof(float); }               // ... | D [32] | lse [32]
constexpr size_t bwd_dma_lds(int nw, int tpw) {                                                                                   // K^T | dS | ring [2][Q | dO | O] | dQ | D, lse [NW][32]
  return (size_t)(HD * (nw * tpw * 16 + 8) + 32 * (nw * tpw * 16 + 8)) * 2 + 2 * 3 * 4096 + 4096 + 2 * nw * 32 * sizeof(float);
}
constexpr size_t fwd_stream_lds(int es, int kb) { return (size_t)2 * (kb * HD + HD * (kb + 4)) * es; }                            // two ring slots of K [KB][64] | V^T [64][KB + 4]
constexpr size_t bwd_stream_lds(int es, int nw, int tpw) { return bwd_tiles_lds(es, nw * tpw * 16) + (size_t)STREAM_QPW * (DQS + 2) * sizeof(float); }      // ... | dQ | D | lse
static_assert(bwd_stream_lds(2, STREAM_BWD_NW, stream_bwd_tpw(2)) <= 80 * 1024 && bwd_stream_lds(4, STREAM_BWD_NW, stream_bwd_tpw(4)) <= 80 * 1024, "two workgroups per CU");

}  // namespace mvlt_attn

#ifdef __HIPCC__
#include "common.h"
#include <type_traits>
#include "attn_plan.h"
#include "../../include/mvlt_hip.h"

// One launch function per family file: the plan's template arguments -> that file's instantiation (a case list, no shape condition), or MVLT_ERR_UNSUPPORTED.
int mvlt_launch_attn_fwd(const mvlt_attn_args& a, const mvlt_attn_plan& p, hipStream_t s);             // attention_fwd.hip
int mvlt_launch_attn_fwd2(const mvlt_attn_args& a, const mvlt_attn_plan& p, hipStream_t s);            // attention_fwd2.hip
int mvlt_launch_attn_bwd(const mvlt_attn_bwd_args& a, const mvlt_attn_plan& p, hipStream_t s);         // attention_bwd.hip
int mvlt_launch_attn_bwd_dma(const mvlt_attn_bwd_args& a, const mvlt_attn_plan& p, hipStream_t s);     // attention_bwd_dma.hip
int mvlt_launch_attn_fwd_stream(const mvlt_attn_args& a, const mvlt_attn_plan& p, hipStream_t s);      // attention_stream.hip
int mvlt_launch_attn_bwd_stream(const mvlt_attn_bwd_args& a, const mvlt_attn_plan& p, hipStream_t s);  // attention_stream.hip

namespace {

using mvlt_attn::NT;
using mvlt_attn::HD;
using mvlt_attn::STREAM_QPW;
using mvlt_attn::DQS;

template <typename T> struct Frag;                 // 8 consecutive-K elements of one MFMA operand row
template <> struct Frag<bf16> { bf16x8 v; };
template <> struct Frag<float> { float v[8]; };

__device__ __forceinline__ void mma32(f32x16& acc, const Frag<bf16>& a, const Frag<bf16>& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma32(f32x16& acc, const Frag<float>& a, const Frag<float>& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], acc, 0, 0, 0);
}
__device__ __forceinline__ void mma16(f32x4& acc, const Frag<bf16>& a, const Frag<bf16>& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma16(f32x4& acc, const Frag<float>& a, const Frag<float>& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

template <typename T> __device__ __forceinline__ Frag<T> load_frag8(const T* p);      // 8 contiguous elements
template <> __device__ __forceinline__ Frag<bf16> load_frag8<bf16>(const bf16* p) {
  Frag<bf16> f; f.v = *(const bf16x8*)p; return f;
}
template <> __device__ __forceinline__ Frag<float> load_frag8<float>(const float* p) {
  Frag<float> f;
  f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
template <typename T> __device__ __forceinline__ Frag<T> zero_frag() {
  Frag<T> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = (T)0.f;
  return f;
}
// 4 + 4 contiguous elements from two places (the V^T / transposed-tile fragments)
template <typename T> __device__ __forceinline__ Frag<T> load_frag44(const T* p0, const T* p1);
template <> __device__ __forceinline__ Frag<bf16> load_frag44<bf16>(const bf16* p0, const bf16* p1) {
  bf16x4 a = *(const bf16x4*)p0, b = *(const bf16x4*)p1;
  Frag<bf16> f;
  f.v = bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return f;
}
template <> __device__ __forceinline__ Frag<float> load_frag44<float>(const float* p0, const float* p1) {
  f32x4 a = *(const f32x4*)p0, b = *(const f32x4*)p1;
  Frag<float> f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}

template <typename T> struct Lds {
  static constexpr int PC = 16 / sizeof(T);             // elements per 16-B chunk
  static constexpr int NCH = HD / PC;                   // chunks per 64-wide row (8 / 16)
  static __device__ __forceinline__ int swz(int row, int chunk) {
    // fp32: an 8-element fragment spans two adjacent chunks, so only even XOR masks keep it contiguous
    return (sizeof(T) == 2) ? (chunk ^ ((row >> 1) & 7)) : (chunk ^ ((row & 7) << 1));
  }
  // element offset of (row, d) in a [rows][64] row-major swizzled tile; d must be a multiple of PC
  static __device__ __forceinline__ int off(int row, int d) { return row * HD + swz(row, d / PC) * PC; }
};

template <typename T> struct StreamKB { static constexpr int fwd = mvlt_attn::stream_kb_fwd(sizeof(T)), bwd_tpw = mvlt_attn::stream_bwd_tpw(sizeof(T)); };

// ---- plan -> launch: a case of a family's list is one instantiation; `who` names the entry point in a launch error
constexpr int tkey(int a, int b = 0, int c = 0, int d = 0) { return ((a * 16 + b) * 16 + c) * 256 + d; }
#define MVLT_ATTN_CASE(KERNEL, KEY, ...)                                                        \
  case tkey KEY:                                                                                \
    mvlt_max_lds<KERNEL>();                                                                     \
    MVLT_LAUNCH(KERNEL, dim3((unsigned)p.grid), dim3((unsigned)p.block), (size_t)p.lds, s, a, __VA_ARGS__); \
    return mvlt_check_launch(who);
inline int attn_no_instantiation(const char* who, const mvlt_attn_plan& p) {
  char name[128] = "?";
  plan_attn_name(p, name, sizeof(name));
  mvlt_set_error("%s: the plan names %s (family %d), which this library does not instantiate", who, name, p.family);
  return MVLT_ERR_UNSUPPORTED;
}

}  // namespace
#endif

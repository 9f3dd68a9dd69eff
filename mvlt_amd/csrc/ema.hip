// Exponential moving average of the model's weights over the flat parameter buffers (gfx950): what timm.utils.ModelEma.update does with three ATen
// launches per state_dict entry (reference engine_grid_masking.py:130-131), as one streaming pass -- 8 B read and 4 (+ 2 for the bf16 copy) written per
// element, like the fused AdamW step of elementwise.hip it is modelled on -- plus one small launch for the module buffers.  include/mvlt_hip_ema.h.
#include "common.h"
#include "../../include/mvlt_hip.h"
#include "../../include/mvlt_hip_ema.h"

namespace {

constexpr int NT = 256;
constexpr int EMA_MAX_WGS = 8192;      // grid cap of ema_update_kernel: one trip of its grid-stride loop covers EMA_MAX_WGS * NT * 4 = 8,388,608 elements

// e * decay + p * (1 - decay) with the two products and the sum each rounded on its own: timm's formula as torch evaluates it in fp32 (three kernels, so
// never fused).  The file is compiled with -ffp-contract=fast, which lets the code generator contract ANY mul + add pair into v_fma_f32 / v_fmac_f32 /
// v_pk_fma_f32: the __fmul_rn / __fadd_rn of this toolchain's headers are plain `*` and `+` and do not stop it, and neither does a contract(off) pragma
// (both were tried: the vector loop came out as v_pk_fma_f32).  The empty asm statements do, whatever the flags: each product passes through one as an
// opaque register value, so the sum that follows has no multiplication left to absorb.  They emit no instruction.
__device__ __forceinline__ float ema_rn(float e, float p, float decay, float omd) {
  float a = __fmul_rn(e, decay);
  float b = __fmul_rn(p, omd);
  asm("" : "+v"(a));
  asm("" : "+v"(b));
  return __fadd_rn(a, b);
}

// Mask byte MVLT_ADAMW_FROZEN: the element is left alone.  The four mask bytes of a 16-byte vector are read first: an all-frozen vector costs that one
// read, a vector without a frozen byte takes the vector path; parameters start at 8-element offsets, so a mixed vector exists only where a frozen
// tensor's ragged tail meets its alignment gap (at most one per tensor) and is written lane by lane.
__global__ __launch_bounds__(NT) void ema_update_kernel(float* ema, const float* p, bf16* e16, long n, float decay, float omd, const uint8_t* mask) {
  for (long i = ((long)blockIdx.x * NT + threadIdx.x) * 4; i < n; i += (long)gridDim.x * NT * 4) {
    const uint32_t mk = mask ? *(const uint32_t*)(mask + i) : 0u;
    uint32_t fz = 0u;                                                       // bit 8 * e: lane e is frozen
#pragma unroll
    for (int e = 0; e < 4; ++e) fz |= (((mk >> (8 * e)) & 0xffu) == (uint32_t)MVLT_ADAMW_FROZEN ? 1u : 0u) << (8 * e);
    if (fz == 0x01010101u) continue;
    const f32x4 ev = *(const f32x4*)(ema + i), pv = *(const f32x4*)(p + i);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = ema_rn(ev[e], pv[e], decay, omd);
    if (fz == 0u) {
      *(f32x4*)(ema + i) = o;
      if (e16) {
        bf16x4 h = {(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
        *(bf16x4*)(e16 + i) = h;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if ((fz >> (8 * e)) & 1u) continue;            // (what a frozen lane computed above -- NaN included -- is dropped here)
        ema[i + e] = o[e];
        if (e16) e16[i + e] = (bf16)o[e];
      }
    }
  }
}

// Module buffers: row t of the device table = {dst address, src address, numel, kind}, handled by workgroup t (the row is read through uniform
// addresses, like the descriptor of weight_prep_kernel).  The tensors are short (BatchNorm statistics: 64-192 floats, counters: one int64) and start
// wherever the allocator put them: 4- and 8-byte accesses, one element per lane and trip.
__global__ __launch_bounds__(NT) void ema_buffers_kernel(const int64_t* table, float decay, float omd) {
  const int64_t* row = table + 4 * (long)blockIdx.x;
  const int64_t dst = row[0], src = row[1], numel = row[2], kind = row[3];
  if (kind == 0) {
    float* d = (float*)dst;
    const float* s = (const float*)src;
    for (int64_t i = threadIdx.x; i < numel; i += NT) d[i] = ema_rn(d[i], s[i], decay, omd);
  } else if (kind == 1) {
    int64_t* d = (int64_t*)dst;
    const int64_t* s = (const int64_t*)src;
    for (int64_t i = threadIdx.x; i < numel; i += NT) d[i] = s[i];
  }
}

inline bool unit_interval(float x) { return x >= 0.0f && x <= 1.0f; }      // false for NaN

}  // namespace

extern "C" int mvlt_ema_version(void) { return MVLT_EMA_VERSION; }

extern "C" int mvlt_ema_update(float* ema, const float* p, void* ema_bf16, long n, float decay, float one_minus_decay, const uint8_t* mask, void* stream) {
  MVLT_REQUIRE(ema && p, "mvlt_ema_update: null pointer (ema and p are required)");
  MVLT_REQUIRE(n >= 0, "mvlt_ema_update: n must not be negative, got %ld", n);
  MVLT_REQUIRE(n % 4 == 0, "mvlt_ema_update: n must be a multiple of 4, got %ld", n);
  MVLT_REQUIRE(unit_interval(decay) && unit_interval(one_minus_decay), "mvlt_ema_update: decay and one_minus_decay must lie in [0, 1], got %g and %g",
               (double)decay, (double)one_minus_decay);
  MVLT_REQUIRE((((uintptr_t)ema | (uintptr_t)p) & 15) == 0 && ((uintptr_t)ema_bf16 & 7) == 0 && ((uintptr_t)mask & 3) == 0,
               "mvlt_ema_update: ema and p must be 16-byte aligned, ema_bf16 8-byte aligned, mask 4-byte aligned");
  if (n == 0) return MVLT_OK;
  long wgs = (n / 4 + NT - 1) / NT;
  if (wgs > EMA_MAX_WGS) wgs = EMA_MAX_WGS;
  MVLT_LAUNCH(ema_update_kernel, dim3((unsigned)wgs), dim3(NT), 0, (hipStream_t)stream, ema, p, (bf16*)ema_bf16, n, decay, one_minus_decay, mask);
  return mvlt_check_launch("mvlt_ema_update");
}

extern "C" int mvlt_ema_update_buffers(const int64_t* table, int n_tensors, float decay, float one_minus_decay, void* stream) {
  MVLT_REQUIRE(table, "mvlt_ema_update_buffers: null pointer (table is required)");
  MVLT_REQUIRE(n_tensors >= 0, "mvlt_ema_update_buffers: n_tensors must not be negative, got %d", n_tensors);
  MVLT_REQUIRE(unit_interval(decay) && unit_interval(one_minus_decay),
               "mvlt_ema_update_buffers: decay and one_minus_decay must lie in [0, 1], got %g and %g", (double)decay, (double)one_minus_decay);
  MVLT_REQUIRE(((uintptr_t)table & 7) == 0, "mvlt_ema_update_buffers: table must be 8-byte aligned");
  if (n_tensors == 0) return MVLT_OK;
  MVLT_LAUNCH(ema_buffers_kernel, dim3((unsigned)n_tensors), dim3(NT), 0, (hipStream_t)stream, table, decay, one_minus_decay);
  return mvlt_check_launch("mvlt_ema_update_buffers");
}

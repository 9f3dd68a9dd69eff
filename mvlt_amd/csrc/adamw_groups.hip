// Fused AdamW over the flat fp32 parameter buffer with a learning rate and a weight decay PER PARAMETER GROUP (gfx950): adamw_kernel of elementwise.hip
// with its two uniform scalars looked up per lane.  HBM-bound like that kernel (20 B read, 12 + 2 written, + 1 group byte per element), so the lookup --
// at most 254 x 16 B, staged once per workgroup in LDS -- rides for free.  include/mvlt_hip_opt.h.
#include "common.h"
#include "../../include/mvlt_hip_opt.h"

namespace {

constexpr int NT = 256;
constexpr int OPT_MAX_WGS = 8192;      // grid cap, as mvlt_adamw_step's: one trip of the grid-stride loop covers OPT_MAX_WGS * NT * 4 = 8,388,608 elements

// hp = {-, beta1, beta2, eps, -, bias_corr1, bias_corr2, grad_scale} (slots 0 and 4 of mvlt_adamw_step's row are not read), table[k] = {lr, weight_decay}.
// s_tab[k] = {lr / bias_corr1, 1 - lr * weight_decay, weight_decay, 0}: adamw_kernel's `step_size` and its decay factor, the same operations on the same
// operands, formed once per group instead of once per launch; the loop body below is that kernel's, expression by expression, so a launch whose bytes name
// one group gives the bits of mvlt_adamw_step(hp[0] = lr, hp[4] = weight_decay, mask of 1s).  That includes the SELECT around the decay product (there: the
// mask bit; here: weight_decay != 0, and p * (1 - lr * 0) = p * 1 = p either way): the file is compiled with -ffp-contract=fast, and without the select
// between them the product and the subtraction that follows are contracted into one fma, which rounds once where adamw_kernel rounds twice.
// Group byte >= n_groups (MVLT_OPT_FROZEN = 255, and every byte that would index past the table): the lane is frozen -- p, m, v and the bf16 copy are not
// written; what the lane computed from g / m / v (NaN included) and from entry 0 of the table is dropped.  The four bytes of a 16-byte vector are read FIRST:
// an all-frozen vector costs that one read.  Unlike the decay mask of adamw_kernel, ANY four bytes may share a vector.
// GATED: gscale_dev is the fp32[4] gate of mvlt_step_gate; every thread reads gate[2] first and returns on 0 before it has touched anything else (the
// whole grid returns: the value is uniform, so no thread is left waiting at the barrier below).
template <bool GATED>
__global__ __launch_bounds__(NT) void adamw_groups_kernel(float* p, const float* g, float* m, float* v, bf16* p16, long n, const float* hp,
                                                          const uint8_t* group_of, const float* table, int n_groups, const float* gscale_dev) {
  __shared__ f32x4 s_tab[MVLT_OPT_MAX_GROUPS];
  if constexpr (GATED) {
    if (gscale_dev[2] == 0.0f) return;
  }
  const float b1 = hp[1], b2 = hp[2], eps = hp[3], bc1 = hp[5], bc2 = hp[6];
  const float gs = GATED ? hp[7] * gscale_dev[1] : gscale_dev ? hp[7] * gscale_dev[0] : hp[7];
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  for (int k = threadIdx.x; k < n_groups; k += NT) {
    const float lr = table[2 * k], wd = table[2 * k + 1];
    f32x4 t = {lr / bc1, 1.0f - lr * wd, wd, 0.0f};
    s_tab[k] = t;
  }
  __syncthreads();
  const uint32_t ng = (uint32_t)n_groups;
  for (long i = ((long)blockIdx.x * NT + threadIdx.x) * 4; i < n; i += (long)gridDim.x * NT * 4) {
    const uint32_t gb = *(const uint32_t*)(group_of + i);                    // 1 byte per parameter element
    uint32_t fz = 0u;                                                        // bit 8 * e: lane e is frozen
#pragma unroll
    for (int e = 0; e < 4; ++e) fz |= (((gb >> (8 * e)) & 0xffu) >= ng ? 1u : 0u) << (8 * e);
    if (fz == 0x01010101u) continue;
    f32x4 pv = *(f32x4*)(p + i), gv = *(const f32x4*)(g + i), mv = *(f32x4*)(m + i), vv = *(f32x4*)(v + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t k = (gb >> (8 * e)) & 0xffu;
      const f32x4 t = s_tab[k < ng ? k : 0u];                                // (never past the staged entries)
      const float step_size = t[0];
      float gr = gv[e] * gs;
      float pp = t[2] != 0.0f ? pv[e] * t[1] : pv[e];
      float mm = b1 * mv[e] + (1.0f - b1) * gr;
      float v2 = b2 * vv[e] + (1.0f - b2) * gr * gr;
      float denom = sqrtf(v2) * inv_sqrt_bc2 + eps;
      pv[e] = pp - step_size * mm / denom;
      mv[e] = mm; vv[e] = v2;
    }
    if (fz == 0u) {
      *(f32x4*)(p + i) = pv; *(f32x4*)(m + i) = mv; *(f32x4*)(v + i) = vv;
      if (p16) {
        bf16x4 o = {(bf16)pv[0], (bf16)pv[1], (bf16)pv[2], (bf16)pv[3]};
        *(bf16x4*)(p16 + i) = o;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if ((fz >> (8 * e)) & 1u) continue;            // (what a frozen lane computed above -- NaN included -- is dropped here)
        p[i + e] = pv[e]; m[i + e] = mv[e]; v[i + e] = vv[e];
        if (p16) p16[i + e] = (bf16)pv[e];
      }
    }
  }
}

}  // namespace

extern "C" int mvlt_opt_version(void) { return MVLT_OPT_VERSION; }

extern "C" int mvlt_adamw_step_groups(float* p, const float* g, float* m, float* v, void* p_bf16, long n, const float* hp, const uint8_t* group_of,
                                      const float* table, int n_groups, const float* gscale_dev, const float* gate, void* stream) {
  MVLT_REQUIRE(p && g && m && v && hp && group_of && table, "mvlt_adamw_step_groups: null pointer (p, g, m, v, hp, group_of and table are required)");
  MVLT_REQUIRE(n >= 0 && n % 4 == 0, "mvlt_adamw_step_groups: n must be a non-negative multiple of 4, got %ld", n);
  MVLT_REQUIRE(n_groups >= 1 && n_groups <= MVLT_OPT_MAX_GROUPS, "mvlt_adamw_step_groups: n_groups must be in [1, %d], got %d (byte %d means frozen)",
               MVLT_OPT_MAX_GROUPS, n_groups, MVLT_OPT_FROZEN);
  MVLT_REQUIRE(!(gscale_dev && gate), "mvlt_adamw_step_groups: both gscale_dev and gate are given (the gate carries its own coefficient)");
  MVLT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && (((uintptr_t)p_bf16 | (uintptr_t)table) & 7) == 0 &&
                   ((uintptr_t)group_of & 3) == 0,
               "mvlt_adamw_step_groups: p, g, m, v must be 16-byte aligned, p_bf16 and table 8-byte aligned, group_of 4-byte aligned");
  if (n == 0) return MVLT_OK;
  long wgs = (n / 4 + NT - 1) / NT;
  if (wgs > OPT_MAX_WGS) wgs = OPT_MAX_WGS;
  if (gate)
    MVLT_LAUNCH((adamw_groups_kernel<true>), dim3((unsigned)wgs), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, (bf16*)p_bf16, n, hp, group_of, table, n_groups, gate);
  else
    MVLT_LAUNCH((adamw_groups_kernel<false>), dim3((unsigned)wgs), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, (bf16*)p_bf16, n, hp, group_of, table, n_groups,
                gscale_dev);
  return mvlt_check_launch("mvlt_adamw_step_groups");
}

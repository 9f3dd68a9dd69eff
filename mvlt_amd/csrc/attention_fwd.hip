// SR-attention, resident forward (fp32, and bf16 past 192 keys): attn_fwd_kernel and its launch.  Overview: attention.hip; dispatch: attn_plan.h.
#include "attention_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ forward
template <typename T, int NKT>
__global__ __launch_bounds__(NT, 2) void attn_fwd_kernel(mvlt_attn_args p, int nq_chunks, int q_per_wg) {
  constexpr int MP = NKT * 32;                // padded key count
  constexpr int VS = MP + 4;                  // V^T row stride (elements): conflict-free 8-B / 16-B column reads
  constexpr int PC = Lds<T>::PC, NCH = Lds<T>::NCH;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sK = (T*)smem;                           // [MP][64] swizzled
  T* sVt = sK + MP * HD;                      // [64][VS]
  static_assert((MP * HD + HD * VS) * sizeof(T) == mvlt_attn::fwd_lds(sizeof(T), NKT), "the plan sizes this launch with attention_common.h's formula");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, l31 = lane & 31;
  // XCD-aware placement: all query chunks of one (batch, head) run on the same XCD (block id % 8) and share K/V in its L2
  const int bid = blockIdx.x;
  const int xcd = bid & 7, j = bid >> 3;
  const int gidx = xcd + 8 * (j / nq_chunks);
  const int chunk_id = j % nq_chunks;
  if (gidx >= p.B * p.H) return;
  const int b = gidx / p.H, h = gidx % p.H;

  const T* Qg = (const T*)p.Q + (long)b * p.N * p.ldq + h * HD;
  const T* Kg = (const T*)p.KV + (long)b * p.M * p.ldkv + p.k_off + h * HD;
  const T* Vg = (const T*)p.KV + (long)b * p.M * p.ldkv + p.v_off + h * HD;
  T* Og = (T*)p.O + (long)b * p.N * p.ldo + h * HD;

  // ---- stage K (swizzled rows) and V^T (transposed) in LDS; rows >= M are zero
  for (int u = tid; u < MP * NCH; u += NT) {
    int r = u / NCH, c = u % NCH;
    u32x4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
    if (r < p.M) {
      kv = *(const u32x4*)(Kg + (long)r * p.ldkv + c * PC);
      vv = *(const u32x4*)(Vg + (long)r * p.ldkv + c * PC);
    }
    *(u32x4*)(sK + Lds<T>::off(r, c * PC)) = kv;
    T ve[PC];
    *(u32x4*)ve = vv;
#pragma unroll
    for (int e = 0; e < PC; ++e) sVt[(c * PC + e) * VS + r] = ve[e];
  }
  __syncthreads();

  const float sl2 = p.scale * 1.44269504088896340736f;
  const int q_begin = chunk_id * q_per_wg;
  const int q_end = min(p.N, q_begin + q_per_wg);
  // Keys are walked in NBLK blocks of <= BT tiles (32 keys each).  NKT <= 7 is ONE block: plain single-pass softmax.
  // Larger M (384-px inputs: 272 keys) uses two blocks merged with the usual running-max rescale, which keeps the
  // score accumulators at <= 80 registers instead of 144-160 (no spills, 2 waves per SIMD).
  constexpr int NBLK = (NKT <= 7) ? 1 : 2;
  constexpr int BT = (NKT + NBLK - 1) / NBLK;
  for (int q0 = q_begin + wave * 32; q0 < q_end; q0 += 4 * 32) {
    const int q = q0 + l31;
    const bool q_ok = q < q_end;
    Frag<T> qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = q_ok ? load_frag8<T>(Qg + (long)q * p.ldq + 16 * s + 8 * g) : zero_frag<T>();

    f32x16 oacc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    }
    float m_run = -INFINITY, sum_loc = 0.f;
#pragma unroll
    for (int blk = 0; blk < NBLK; ++blk) {
      const int t0 = blk * BT;
      f32x16 acc[BT];
      // K fragments one tile ahead of their MFMAs (two tiles' worth live): a tile's four LDS reads issued right in front of the MFMAs
      // that use them put one LDS latency in front of every tile, and both waves of a SIMD stall the same way
      Frag<T> kf[2][4];
#pragma unroll
      for (int s = 0; s < 4; ++s) kf[0][s] = load_frag8<T>(sK + Lds<T>::off(t0 * 32 + l31, 16 * s + 8 * g));
#pragma unroll
      for (int ti = 0; ti < BT; ++ti) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ti][r] = 0.f;
        if (ti + 1 < BT && t0 + ti + 1 < NKT) {
#pragma unroll
          for (int s = 0; s < 4; ++s) kf[(ti + 1) & 1][s] = load_frag8<T>(sK + Lds<T>::off((t0 + ti + 1) * 32 + l31, 16 * s + 8 * g));
        }
        if (t0 + ti < NKT) {
#pragma unroll
          for (int s = 0; s < 4; ++s) mma32(acc[ti], kf[ti & 1][s], qf[s]);          // rows = keys, cols = queries
        }
        __builtin_amdgcn_sched_barrier(0);      // keep only two tiles' K fragments live (register budget: 2 waves/SIMD)
      }
      // acc[ti][r] = S[q = l31][key = 32 (t0+ti) + (r&3) + 8 (r>>2) + 4 g]
      float mb = -INFINITY;
      if (p.M == MP && NKT % NBLK == 0) {         // no padded key anywhere (M = 192 at 256 px): no masking pass
#pragma unroll
        for (int ti = 0; ti < BT; ++ti)
#pragma unroll
          for (int r = 0; r < 16; ++r) mb = fmaxf(mb, acc[ti][r]);
      } else {
#pragma unroll
        for (int ti = 0; ti < BT; ++ti)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            int key = 32 * (t0 + ti) + (r & 3) + 8 * (r >> 2) + 4 * g;
            float sv = (t0 + ti < NKT && key < p.M) ? acc[ti][r] : -INFINITY;
            acc[ti][r] = sv;
            mb = fmaxf(mb, sv);
          }
      }
      mb = fmaxf(mb, __shfl_xor(mb, 32));
      const float m_new = fmaxf(m_run, mb);     // finite: every block holds >= 1 valid key
      if (blk > 0) {
        const float alpha = exp2f((m_run - m_new) * sl2);
        sum_loc *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
      }
      m_run = m_new;
      // bf16: the bare v_exp_f32 (libm's exp2f wraps it in a denormal-range rescale, five more VALU per score; results below 2^-126
      // feed a bf16 P and a sum >= 1 either way); the fp32 parity path keeps libm's
      const float mneg = -m_new * sl2;
#pragma unroll
      for (int ti = 0; ti < BT; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float e;
          if constexpr (sizeof(T) == 2) e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[ti][r], sl2, mneg));
          else e = exp2f((acc[ti][r] - m_new) * sl2);
          acc[ti][r] = e;
          sum_loc += e;
        }
      // PV: step u = (key tile, 16-key half); the V^T fragments of step u + 1 are read while step u's MFMAs run
      Frag<T> vf[2][2];
      {
        const int kb = 32 * t0 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) { const T* vr = sVt + (32 * dt + l31) * VS + kb; vf[0][dt] = load_frag44<T>(vr, vr + 8); }
      }
#pragma unroll
      for (int u = 0; u < 2 * BT; ++u) {
        const int ti = u >> 1, s2 = u & 1;
        if (t0 + ti >= NKT) continue;
        if (u + 1 < 2 * BT && t0 + ((u + 1) >> 1) < NKT) {
          const int kb = 32 * (t0 + ((u + 1) >> 1)) + 16 * ((u + 1) & 1) + 4 * g;
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) { const T* vr = sVt + (32 * dt + l31) * VS + kb; vf[(u + 1) & 1][dt] = load_frag44<T>(vr, vr + 8); }
        }
        Frag<T> pf;                             // B operand: P^T, k-slot (g, jj) <-> key 32kt + 16 s2 + 4g + 8 (jj>>2) + (jj&3)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) pf.v[jj] = (T)acc[ti][8 * s2 + jj];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) mma32(oacc[dt], vf[u & 1][dt], pf);            // rows = d, cols = queries
        __builtin_amdgcn_sched_barrier(0);      // do not hoist every V^T fragment above the first PV MFMA
      }
    }
    const float sum = sum_loc + __shfl_xor(sum_loc, 32);
    const float inv = 1.0f / sum;
    // oacc[dt][r] = O[q = l31][d = 32 dt + (r&3) + 8 (r>>2) + 4 g]
    if (q_ok) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          T o4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) o4[e] = (T)(oacc[dt][4 * rq + e] * inv);
          T* dst = Og + (long)q * p.ldo + 32 * dt + 8 * rq + 4 * g;
          if constexpr (sizeof(T) == 2) *(u32x2*)dst = *(u32x2*)o4; else *(u32x4*)dst = *(u32x4*)o4;
        }
      if (g == 0 && p.lse) p.lse[((long)b * p.H + h) * p.N + q] = m_run * p.scale + logf(sum);
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
int mvlt_launch_attn_fwd(const mvlt_attn_args& a, const mvlt_attn_plan& p, hipStream_t s) {
  const char* const who = "mvlt_sr_attention_fwd";
#define FWD(T, DT, NKT) MVLT_ATTN_CASE((attn_fwd_kernel<T, NKT>), (DT, NKT), p.nq_chunks, p.q_per_wg)
  switch (tkey(p.tp[0], p.tp[1])) {
    FWD(bf16, 0, 7) FWD(bf16, 0, 8) FWD(bf16, 0, 9) FWD(bf16, 0, 10)                 // (up to 6 key tiles bf16 is attn_fwd2_kernel's)
    FWD(float, 1, 1) FWD(float, 1, 2) FWD(float, 1, 3) FWD(float, 1, 4) FWD(float, 1, 5) FWD(float, 1, 6) FWD(float, 1, 7) FWD(float, 1, 8) FWD(float, 1, 9)
  }
#undef FWD
  return attn_no_instantiation(who, p);
}

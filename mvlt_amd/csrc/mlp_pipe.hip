// Fused MLP of stages 1-2, software-pipelined forward / input gradient: mlp_pipe_kernel and its launch.  Overview: mlp.hip; dispatch: mlp_plan.h.
#include "mlp_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ software-pipelined fused MLP
// Round 3.  The kernel above runs, per wave and hidden chunk, 16 producer MFMAs, then ~270 VALU instructions of GELU, then 16 consumer
// MFMAs -- strictly one after the other (ISA: tools/isa_mix.py), so the matrix pipe idles through every activation block and the VALU
// through every MFMA block unless ANOTHER wave of the SIMD happens to be in the opposite phase (counters: MFMA busy 0.20-0.28 of SIMD
// cycles, VALU active ~0.25 per wave).  Here the three stages of a 32-hidden-unit slice u are spread over three loop iterations of ONE
// wave -- iteration i issues the producer MFMAs of slice i+1, the activation of slice i and the consumer MFMAs of slice i-1, which are
// independent instruction streams the scheduler may interleave (MFMAs issue asynchronously: the VALU work of a wave runs in the shadow
// of its own matrix instructions):
//
//     P(i+1): H = W1[slice] x^T + b1      (+ dG = W2^T[slice] dy^T)     -> hacc[(i+1)&1]      [MFMA]
//     G(i)  : g = gelu(H)                 (dH = dG * gelu'(H))          -> gfrag[i&1] (bf16)  [VALU]
//     C(i-1): out += g W2[:, slice]^T     (dx += dH W1^T[:, slice])                            [MFMA]
//
// Producer tiles are transposed (rows = hidden units, columns = tokens) and the hidden unit of tile row rho is chosen as
// 32 u + 8 (rho >> 2) + 4 h + (rho & 3) for the two tiles h = 0, 1 of a slice: lane (fr, fg) then ends up with the EIGHT CONSECUTIVE
// hidden units 32 u + 8 fg .. + 7 of token fr = one A-operand fragment of the consumer MFMA in natural k order, and the consumer's B
// fragment is ONE 16-byte LDS read (the kernel above pairs tiles 16 apart: two 8-byte reads that hipcc fuses into ds_read2st64_b64,
// which is 2-way bank conflicted: lds_conflict_frac 0.25-0.31).  fc1's bias is the producer's accumulator initialiser (no VALU add).
// Weight slices arrive by LDS-DMA (no staging registers, no ds_write), two small rings of two slots: the producer side (W1 [, W2^T]
// rows of slice i+2) and the consumer side (Wb columns of slice i) are fetched in iteration i, one barrier per iteration.
template <int C> __device__ __forceinline__ int pipe_fP(int rho) {       // 16-B slot swizzle of a producer-tile row (row = hidden unit in slice)
  return C == 64 ? (((rho >> 1) & 1) | (((rho >> 3) & 3) << 1)) : ((rho & 3) | (((rho >> 3) & 3) << 2));
}
__device__ __forceinline__ int pipe_gC(int n) { return (0 - (n >> 2)) & 3; }   // same for a consumer-tile row (row = channel, 64-B rows)

__device__ __forceinline__ float gelu_fast1(float x) {
#if MVLT_GELU_POLY & 2
  return gelu_poly1(x);
#endif
  const float xc = __builtin_amdgcn_fmed3f(x, -7.0f, 7.0f);
  const float x2 = xc * xc;
  const float t = xc * __builtin_fmaf(__builtin_fmaf(x2, -MVLT_LOG2E * MVLT_GP2, -MVLT_LOG2E * MVLT_GP1), x2, -MVLT_LOG2E * MVLT_GP0);
  const float e = __builtin_amdgcn_exp2f(t);
  return x * __builtin_amdgcn_rcpf(e + 1.0f);
}
__device__ __forceinline__ float gelu_fast_grad1(float x) {
#if MVLT_GELU_POLY & 1
  return gelu_poly_grad1(x);
#endif
  const float xc = __builtin_amdgcn_fmed3f(x, -7.0f, 7.0f);
  const float x2 = xc * xc;
  const float t = xc * __builtin_fmaf(__builtin_fmaf(x2, -MVLT_LOG2E * MVLT_GP2, -MVLT_LOG2E * MVLT_GP1), x2, -MVLT_LOG2E * MVLT_GP0);
  const float e = __builtin_amdgcn_exp2f(t);
  const float sg = __builtin_amdgcn_rcpf(e + 1.0f);
  const float up = __builtin_fmaf(__builtin_fmaf(x2, 5.0f * MVLT_GP2, 3.0f * MVLT_GP1), x2, MVLT_GP0);
  return __builtin_fmaf(x * up, sg * sg * e, sg);
}

// Waves per SIMD the register allocation is held to.  A wave of these kernels issues one VALU instruction per ~3.5 ns however few waves share
// its SIMD (tools/probes/valu_rates.hip: 16 x {MFMA + 8 v_fma} takes 38.8 / 27.5 / 21.5 ticks per SIMD at 2 / 3 / 4 waves), so occupancy is
// throughput here.  The C = 64 input-gradient kernel needs 171 registers with the polynomial GELU' (174 with the sigmoid form); held to 168
// = THREE waves per SIMD it spills two dwords outside the slice loop (8 B of scratch per lane, none in the loop) and its epilogue requests
// the LayerNorm-backward operands one 16-row tile at a time (PFALL = false in mlp_epilogue: half the registers; the third wave covers the
// round trip): bare launch 359 -> 326 us, step -0.1 ms (same-box A/B).  The sigmoid form at three waves with the all-rows prefetch spilled
// inside the epilogue: +0.5 ms per step.  Four waves (128 registers) spill 328 B per lane: 1778 us.  C = 128 forward at three waves: 260 B
// of scratch, 213 -> 390 us.
// The activation is the polynomial / sigmoid form of common.h, not the table of mlp_wgrad.hip: three to four waves per SIMD already hide it and the gather's LDS latency
// is not hidden (by table: input gradients 325 -> 324 / 301 -> 306 us, forward 265 -> 283 / 204 -> 210 us).
template <int C, int MODE>
__global__ __launch_bounds__(NT, (C == 64 && MODE == 1) ? 3 : 2) void mlp_pipe_kernel(mvlt_mlp_args p) {
  constexpr int MT = 2, CT = C / 16, KS_C = C / 32;
  constexpr int NP = MODE == 1 ? 2 : 1;          // producer-side tiles per slice: W1 (, W2^T)
  constexpr int RB = 2 * C;                      // bytes per producer-tile row
  constexpr int SPR = RB / 16;                   // 16-B slots per row: 8 / 16
  constexpr int RPI = 64 / SPR;                  // rows per DMA instruction: 8 / 4
  constexpr int IPW = 32 / RPI / 4;              // DMA instructions per wave per producer tile: 1 / 2
  constexpr int PB = 32 * RB;                    // producer tile bytes: 4 / 8 KB
  constexpr int CB = C * 64;                     // consumer tile [C][32] bytes: 4 / 8 KB
  constexpr int IPWC = C / 16 / 4;               // DMA instructions per wave per consumer tile: 1 / 2
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [2][NP][PB] producer ring | [2][CB] consumer ring | b1 [hid] floats
  char* const sP = smem;
  char* const sC = smem + 2 * NP * PB;
  float* const sB1 = (float*)(sC + 2 * CB);
  static_assert(2 * NP * PB + 2 * CB == mvlt_mlp::pipe_tiles_bytes(C, MODE) && sizeof(*sB1) * 64 == mvlt_mlp::bias_bytes(64),
                "the plan sizes this launch with mlp_common.h's formula: the two rings, then bias_bytes(hid)");
  const unsigned sP_lds = (unsigned)(uintptr_t)sP, sC_lds = (unsigned)(uintptr_t)sC;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int m0 = blockIdx.x * 128;
  const int hid = p.hid, NU = hid / 32;

  // ---- DMA geometry: per-lane source pointers of slice 0, advanced by a wave-uniform slice offset
  const char* srcP[NP][IPW];
  const char* srcC[IPWC];
#pragma unroll
  for (int it = 0; it < IPW; ++it) {
    const int q = wave + 4 * it, row = q * RPI + lane / SPR, slot = lane % SPR;
    const long off = (long)row * RB + ((slot ^ pipe_fP<C>(row)) << 4);
    srcP[0][it] = (const char*)p.w1 + off;
    if (MODE == 1) srcP[NP - 1][it] = (const char*)p.wc + off;
  }
#pragma unroll
  for (int it = 0; it < IPWC; ++it) {
    const int q = wave + 4 * it, n = q * 16 + (lane >> 2), slot = lane & 3;
    srcC[it] = (const char*)p.wb + (long)n * hid * 2 + ((slot ^ pipe_gC(n)) << 4);
  }
  auto dmaP = [&](int u, int ring) {             // producer tile(s) of slice u -> ring slot
    const long so = (long)u * PB;
#pragma unroll
    for (int t = 0; t < NP; ++t)
#pragma unroll
      for (int it = 0; it < IPW; ++it)
        glds16(srcP[t][it] + so, __builtin_amdgcn_readfirstlane(sP_lds + (ring * NP + t) * PB + (wave + 4 * it) * 1024));
  };
  auto dmaC = [&](int u, int ring) {
#pragma unroll
    for (int it = 0; it < IPWC; ++it)
      glds16(srcC[it] + u * 64, __builtin_amdgcn_readfirstlane(sC_lds + ring * CB + (wave + 4 * it) * 1024));
  };
  dmaP(0, 0);
  if (NU > 1) dmaP(1, 1);
  for (int u = tid; u < hid; u += NT) sB1[u] = p.b1[u];

  bf16x8 xfr[MT][KS_C], yfr[MODE == 1 ? MT : 1][KS_C];
  mlp_load_rows<C, MODE>(p, m0, wave, fr, fg, xfr, yfr);

  // ---- fragment geometry (byte offsets inside a tile)
  const int rho0 = 8 * (fr >> 2) + (fr & 3);                         // tile h: row rho0 + 4 h
  int poff[KS_C];
#pragma unroll
  for (int ks = 0; ks < KS_C; ++ks) poff[ks] = rho0 * RB + (((ks * 4 + fg) ^ pipe_fP<C>(rho0)) << 4);
  const int coff = fr * 64 + ((fg ^ pipe_gC(fr)) << 4);             // tile j: + j * 16 * 64

  f32x4 oacc[MT][CT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) oacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 hacc[2][2][MT], dgacc[MODE == 1 ? 2 : 1][2][MT];
  u32x4 gfrag[2][MT];                            // bf16 pairs: word 2 h + (r >> 1) of token tile mt = hidden units 8 fg + 4 h + r

  // One iteration = NSLOT slots of {a few MFMAs, two activations per lane}, pinned apart by sched_barrier(0): hipcc otherwise emits an
  // iteration's MFMAs as one block and its ~150 VALU instructions as another (checked in the ISA; sched_group_barrier requests did
  // not change that), which is exactly the serialisation this kernel exists to remove.  Inside a slot the MFMAs come first, so the
  // activation's VALU / transcendental instructions issue while the matrix pipe works.
  //   PAR = parity of the slice being ACTIVATED (i): hacc[PAR] -> gfrag[PAR]; producers write hacc[PAR ^ 1] (slice i + 1) from producer
  //   ring slot PAR ^ 1; consumers read gfrag[PAR ^ 1] (slice i - 1) and consumer ring slot PAR ^ 1.
  constexpr int NSLOT = 8;
  constexpr int PK = KS_C / 2;                   // producer k-steps per slot (a tile takes two slots)
  constexpr int CPS = CT * MT / NSLOT;           // consumer MFMAs per slot: 1 / 2
  auto iteration = [&](auto parc, auto dopc, auto docc, auto dogc, int u_next) {
    constexpr int PAR = decltype(parc)::value;
    constexpr bool DO_P = decltype(dopc)::value, DO_C = decltype(docc)::value, DO_G = decltype(dogc)::value;
    const char* tp = sP + (PAR ^ 1) * NP * PB;
    const char* tc = sC + (PAR ^ 1) * CB;
    // operand fragments of slot sl are read one slot ahead into set sl & 1 (only slot 0's reads wait for LDS in front of their MFMAs)
    bf16x8 af[2][PK], cf[MODE == 1 ? 2 : 1][PK], bfr[2][CPS];
    f32x4 b1v;
    auto read_frags = [&](auto slc) {
      constexpr int sl = decltype(slc)::value, t = sl >> 1, half = sl & 1, h = t >> 1;
      if (DO_P) {
#pragma unroll
        for (int k = 0; k < PK; ++k) {
          af[sl & 1][k] = *(const bf16x8*)(tp + h * 4 * RB + poff[half * PK + k]);
          if (MODE == 1) cf[sl & 1][k] = *(const bf16x8*)(tp + PB + h * 4 * RB + poff[half * PK + k]);
        }
        if ((sl & 3) == 0) b1v = *(const f32x4*)(sB1 + u_next * 32 + 8 * fg + 4 * h);       // first slot of the two tiles sharing h
      }
      if (DO_C) {
#pragma unroll
        for (int k = 0; k < CPS; ++k) bfr[sl & 1][k] = *(const bf16x8*)(tc + ((sl * CPS + k) / MT) * 16 * 64 + coff);
      }
    };
    read_frags(std::integral_constant<int, 0>{});
    auto slot = [&](auto slc) {
      constexpr int sl = decltype(slc)::value;
      constexpr int t = sl >> 1, half = sl & 1;  // producer tile (h, mt) = (t >> 1, t & 1) and activation group: same order
      constexpr int h = t >> 1, mt = t & 1;
      if constexpr (sl + 1 < NSLOT) read_frags(std::integral_constant<int, sl + 1>{});
      if (DO_P) {
        f32x4 hh = half == 0 ? b1v : hacc[PAR ^ 1][h][mt];
        f32x4 dg = half == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : dgacc[MODE == 1 ? (PAR ^ 1) : 0][h][mt];
#pragma unroll
        for (int k = 0; k < PK; ++k) {
          hh = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[sl & 1][k], xfr[mt][half * PK + k], hh, 0, 0, 0);
          if (MODE == 1) dg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cf[sl & 1][k], yfr[mt][half * PK + k], dg, 0, 0, 0);
        }
        hacc[PAR ^ 1][h][mt] = hh;
        if (MODE == 1) dgacc[PAR ^ 1][h][mt] = dg;
      }
      if (DO_C) {
#pragma unroll
        for (int k = 0; k < CPS; ++k) {
          constexpr int c0 = sl * CPS;
          const int c = c0 + k, j = c / MT, i = c % MT;
          oacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gfrag[PAR ^ 1][i]), bfr[sl & 1][k], oacc[i][j], 0, 0, 0);
        }
      }
      if (DO_G) {
        const float h0 = hacc[PAR][h][mt][2 * half], h1 = hacc[PAR][h][mt][2 * half + 1];
        float g0, g1;
        if (MODE == 0) { g0 = gelu_fast1(h0); g1 = gelu_fast1(h1); }
        else {
          g0 = dgacc[MODE == 1 ? PAR : 0][h][mt][2 * half] * gelu_fast_grad1(h0);
          g1 = dgacc[MODE == 1 ? PAR : 0][h][mt][2 * half + 1] * gelu_fast_grad1(h1);
        }
        gfrag[PAR][mt][2 * h + half] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{g0, g1}, bf16x2));
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    slot(std::integral_constant<int, 0>{}); slot(std::integral_constant<int, 1>{}); slot(std::integral_constant<int, 2>{});
    slot(std::integral_constant<int, 3>{}); slot(std::integral_constant<int, 4>{}); slot(std::integral_constant<int, 5>{});
    slot(std::integral_constant<int, 6>{}); slot(std::integral_constant<int, 7>{});
  };
  auto fence = [&]() {                           // this iteration's DMAs have landed for every wave; its LDS reads are done
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using Y = std::true_type;
  using N = std::false_type;

  fence();                                       // slices 0, 1 of the producer side and the bias are in LDS
  iteration(P1{}, Y{}, N{}, N{}, 0);             // "iteration -1": producers of slice 0 (ring slot 0) -> hacc[0]
  fence();                                       // ring slot 0 may be refilled
  // iteration 0: P(1), G(0)
  dmaP(min(2, NU - 1), 0);
  dmaC(0, 0);
  iteration(P0{}, Y{}, N{}, Y{}, 1);
  fence();
  // steady state, two iterations per trip: i odd, then i + 1 even (NU is even and >= 4: mlp_plan.h hands this kernel whole 64-unit chunks, two or more)
  for (int i = 1; i + 1 < NU - 1; i += 2) {
    dmaP(min(i + 2, NU - 1), 1);
    dmaC(i, 1);
    iteration(P1{}, Y{}, Y{}, Y{}, i + 1);
    fence();
    dmaP(min(i + 3, NU - 1), 0);
    dmaC(i + 1, 0);
    iteration(P0{}, Y{}, Y{}, Y{}, i + 2);
    fence();
  }
  // last iteration i = NU - 1 (odd): G(NU-1), C(NU-2); then the consumers of the last slice alone
  dmaC(NU - 1, 1);
  iteration(P1{}, N{}, Y{}, Y{}, 0);
  fence();
  iteration(P0{}, N{}, Y{}, N{}, 0);
  __syncthreads();                               // the epilogue stages through the same LDS
  mlp_epilogue<C, MODE, !(C == 64 && MODE == 1)>(p, smem, m0, tid, oacc);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
#define PIPE(C, MODE) MVLT_MLP_CASE((mlp_pipe_kernel<C, MODE>), (C, MODE))
int mvlt_launch_mlp_pipe(const mvlt_mlp_args& a, const mvlt_mlp_plan& p, hipStream_t s, const char* who) {
  switch (mkey(p.tp[0], p.tp[1])) {
    PIPE(64, 0) PIPE(64, 1) PIPE(128, 0) PIPE(128, 1)
    default: return mlp_no_instantiation(who, p);
  }
  return mvlt_check_launch(who);
}

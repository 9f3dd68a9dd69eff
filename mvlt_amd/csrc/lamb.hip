// LAMB over the flat fp32 parameter buffer (gfx950): AdamW's moments, then every tensor's update scaled by ||p|| / ||update|| of THAT tensor -- a segmented
// reduction over a buffer whose segments run from 64 elements to 23.4 M.  Three launches, no atomics, no host read, two floats of scratch per chunk:
//   lamb_moments_kernel   one workgroup per chunk of one tensor: p, g, m, v in, m, v out, u in registers, {sum p^2, sum u^2} of the chunk to its own slot
//   lamb_fold_kernel      one workgroup per tensor: its slots summed in a fixed order -> ratios[T]
//   lamb_apply_kernel     one workgroup per chunk: u again from the m, v, p just written (the same expressions), p -= lr * ratios[T] * u, bf16 copy
// HBM-bound: 16 B read + 8 written, then 12 B read + 4 (+ 2) written per element.  include/mvlt_hip_lamb.h, docs/lamb.md.
#include "common.h"
#include "../../include/mvlt_hip_lamb.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = MVLT_LAMB_CHUNK;      // elements per workgroup: 16 trips of NT 16-byte vectors
constexpr int ROW = MVLT_LAMB_ROW;
static_assert(CHUNK % (NT * 4) == 0, "a chunk is whole trips of the workgroup");

// What workgroup blockIdx.x works on, from the two tables (uniform addresses: scalar loads).  false = nothing: a frozen tensor, or a row that names
// something outside the buffers (mvlt_lamb_check_tables refuses such tables with a message; here they cost a return, never an access).  The value is the
// same for every thread of the workgroup, so a false leaves nobody waiting at a barrier.
__device__ __forceinline__ bool chunk_of(const int64_t* tensors, int n_tensors, const int32_t* chunks, long n, int n_groups, long& off, int& len, int& tensor,
                                         int& group) {
  tensor = chunks[2 * (long)blockIdx.x];
  const int k = chunks[2 * (long)blockIdx.x + 1];
  if ((unsigned)tensor >= (unsigned)n_tensors || k < 0) return false;
  const int64_t* row = tensors + ROW * (long)tensor;
  const long t_off = row[0], t_len = row[1];
  group = (int)row[2];
  if (row[3] != 0) return false;                                                // frozen
  const long lo = (long)k * CHUNK;
  if (t_off < 0 || (t_off & 3) != 0 || t_len <= lo || t_len > n || t_off > n - t_len || (unsigned)group >= (unsigned)n_groups) return false;
  off = t_off + lo;
  len = (int)(t_len - lo < (long)CHUNK ? t_len - lo : (long)CHUNK);
  return true;
}

// u of one element from its NEW moments.  Launch 1 and launch 3 both call this with mm / v2 as opaque register values (launch 1: behind the empty asm
// below; launch 3: loaded), so -ffp-contract=fast has the same multiplications to contract in both and the two u agree.
__device__ __forceinline__ float lamb_u(float mm, float v2, float p, float inv_bc1, float inv_sqrt_bc2, float eps, float wd) {
  const float denom = sqrtf(v2) * inv_sqrt_bc2 + eps;
  return (mm * inv_bc1) / denom + wd * p;
}

// mm / v2 in the bits adamw_kernel (elementwise.hip) leaves.  That kernel writes b1 * m + (1 - b1) * gr and b2 * v + (1 - b2) * gr * gr and is compiled with
// -ffp-contract=fast: which product of each sum is absorbed into the fma is the compiler's choice there -- it rounds b1 * m and fuses (1 - b1) * gr; it
// rounds ((1 - b2) * gr) * gr and fuses b2 * v.  The same two source lines HERE came out differently (the vectoriser paired the products of the first sum
// into one v_pk_mul_f32 and added them: no fma at all; in the second it fused the other product), so the roundings are spelled out: an explicit fma
// takes no part in contraction, and a product that feeds one has no addition to be contracted with.  tests/test_lamb_gpu.py compares the bits.
// The empty asm statements make the results opaque before anything else uses them.
__device__ __forceinline__ void lamb_moments(float g, float m, float v, float gs, float b1, float b2, float& mm, float& v2) {
  const float gr = g * gs;
  mm = __builtin_fmaf(1.0f - b1, gr, b1 * m);
  v2 = __builtin_fmaf(b2, v, ((1.0f - b2) * gr) * gr);
  asm("" : "+v"(mm));
  asm("" : "+v"(v2));
}

// {a, b} summed over the workgroup in a fixed order: the xor butterfly of each wave (6 levels), then the NT / 64 = 4 waves as (w0 + w1) + (w2 + w3).
// Valid in thread 0.
__device__ __forceinline__ void block_sum2(float& a, float& b, float* s_red) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_red[2 * w] = a; s_red[2 * w + 1] = b; }
  __syncthreads();
  a = (s_red[0] + s_red[2]) + (s_red[4] + s_red[6]);
  b = (s_red[1] + s_red[3]) + (s_red[5] + s_red[7]);
}

// GATED: gscale_dev is the fp32[4] gate of mvlt_step_gate; every thread reads gate[2] first and returns on 0 before it has touched anything else.
// Per lane: at most CHUNK / (NT * 4) = 16 trips, each adding ONE value -- the four squares of its vector summed as (0 + 1) + (2 + 3) -- to the running
// sums; the ragged tail of a tensor (length % 4 elements, one lane, its last trip) adds lane by lane.
template <bool GATED>
__global__ __launch_bounds__(NT) void lamb_moments_kernel(const float* p, const float* g, float* m, float* v, long n, const float* hp, const int64_t* tensors,
                                                          int n_tensors, const int32_t* chunks, const float* table, int n_groups, float* partials,
                                                          const float* gscale_dev) {
  __shared__ float s_red[2 * NT / 64];
  if constexpr (GATED) {
    if (gscale_dev[2] == 0.0f) return;
  }
  long off;
  int len, tensor, group;
  if (!chunk_of(tensors, n_tensors, chunks, n, n_groups, off, len, tensor, group)) return;
  const float b1 = hp[1], b2 = hp[2], eps = hp[3], bc1 = hp[5], bc2 = hp[6];
  const float gs = GATED ? hp[7] * gscale_dev[1] : gscale_dev ? hp[7] * gscale_dev[0] : hp[7];
  const float inv_bc1 = 1.0f / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
  const float wd = table[2 * group + 1];
  p += off; g += off; m += off; v += off;
  float sp = 0.0f, su = 0.0f;
  for (int i = threadIdx.x * 4; i < len; i += NT * 4) {
    if (i + 4 <= len) {
      const f32x4 pv = *(const f32x4*)(p + i), gv = *(const f32x4*)(g + i);
      f32x4 mv = *(const f32x4*)(m + i), vv = *(const f32x4*)(v + i), pp, uu;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float mm, v2;
        lamb_moments(gv[e], mv[e], vv[e], gs, b1, b2, mm, v2);
        const float u = lamb_u(mm, v2, pv[e], inv_bc1, inv_sqrt_bc2, eps, wd);
        mv[e] = mm; vv[e] = v2;
        pp[e] = pv[e] * pv[e]; uu[e] = u * u;
      }
      *(f32x4*)(m + i) = mv; *(f32x4*)(v + i) = vv;
      sp += (pp[0] + pp[1]) + (pp[2] + pp[3]);
      su += (uu[0] + uu[1]) + (uu[2] + uu[3]);
    } else {
      for (int e = i; e < len; ++e) {                   // the tail of a tensor whose length is no multiple of 4: never a load or a store past its end
        float mm, v2;
        const float pe = p[e];
        lamb_moments(g[e], m[e], v[e], gs, b1, b2, mm, v2);
        const float u = lamb_u(mm, v2, pe, inv_bc1, inv_sqrt_bc2, eps, wd);
        m[e] = mm; v[e] = v2;
        sp += pe * pe; su += u * u;
      }
    }
  }
  block_sum2(sp, su, s_red);
  if (threadIdx.x == 0) {
    partials[2 * (long)blockIdx.x] = sp;
    partials[2 * (long)blockIdx.x + 1] = su;
  }
}

// One workgroup per tensor.  Lane l adds slots l, l + NT, l + 2 NT, ... of the tensor in that order, then block_sum2: a function of the tensor's own chunks
// alone, so a tensor's ratio does not depend on what stands next to it.
template <bool GATED>
__global__ __launch_bounds__(NT) void lamb_fold_kernel(const float* partials, int n_chunks, const int64_t* tensors, const float* table, int n_groups, int flags,
                                                       float* ratios, const float* gate) {
  __shared__ float s_red[2 * NT / 64];
  if constexpr (GATED) {
    if (gate[2] == 0.0f) return;
  }
  const int64_t* row = tensors + ROW * (long)blockIdx.x;
  const long group = row[2], first = row[4], cnt = row[5];
  if (row[3] != 0) return;                                                      // frozen: ratios[T] keeps what it held
  if (group < 0 || group >= n_groups || first < 0 || cnt < 0 || first > (long)n_chunks - cnt) return;
  float sp = 0.0f, su = 0.0f;
  for (long c = threadIdx.x; c < cnt; c += NT) {
    sp += partials[2 * (first + c)];
    su += partials[2 * (first + c) + 1];
  }
  block_sum2(sp, su, s_red);
  if (threadIdx.x == 0) {
    const float wn = sqrtf(sp), un = sqrtf(su), wd = table[2 * group + 1];
    float r = 1.0f;
    if ((wd != 0.0f || (flags & MVLT_LAMB_ALWAYS_ADAPT)) && wn > 0.0f && un > 0.0f) r = wn / un;
    if (flags & MVLT_LAMB_TRUST_CLIP) r = fminf(r, 1.0f);
    ratios[blockIdx.x] = r;
  }
}

template <bool GATED>
__global__ __launch_bounds__(NT) void lamb_apply_kernel(float* p, const float* m, const float* v, bf16* p16, long n, const float* hp, const int64_t* tensors,
                                                        int n_tensors, const int32_t* chunks, const float* table, int n_groups, const float* ratios,
                                                        const float* gate) {
  if constexpr (GATED) {
    if (gate[2] == 0.0f) return;
  }
  long off;
  int len, tensor, group;
  if (!chunk_of(tensors, n_tensors, chunks, n, n_groups, off, len, tensor, group)) return;
  const float eps = hp[3], bc1 = hp[5], bc2 = hp[6];
  const float inv_bc1 = 1.0f / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
  const float lr = table[2 * group], wd = table[2 * group + 1];
  const float step = lr * ratios[tensor];
  p += off; m += off; v += off;
  if (p16) p16 += off;
  for (int i = threadIdx.x * 4; i < len; i += NT * 4) {
    if (i + 4 <= len) {
      f32x4 pv = *(const f32x4*)(p + i);
      const f32x4 mv = *(const f32x4*)(m + i), vv = *(const f32x4*)(v + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) pv[e] = pv[e] - step * lamb_u(mv[e], vv[e], pv[e], inv_bc1, inv_sqrt_bc2, eps, wd);
      *(f32x4*)(p + i) = pv;
      if (p16) {
        bf16x4 o = {(bf16)pv[0], (bf16)pv[1], (bf16)pv[2], (bf16)pv[3]};
        *(bf16x4*)(p16 + i) = o;
      }
    } else {
      for (int e = i; e < len; ++e) {
        const float pe = p[e] - step * lamb_u(m[e], v[e], p[e], inv_bc1, inv_sqrt_bc2, eps, wd);
        p[e] = pe;
        if (p16) p16[e] = (bf16)pe;
      }
    }
  }
}

inline bool aligned(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }

}  // namespace

extern "C" int mvlt_lamb_version(void) { return MVLT_LAMB_VERSION; }

extern "C" int mvlt_lamb_check_tables(const int64_t* tensors, int n_tensors, const int32_t* chunks, int n_chunks, long n, int n_groups) {
  MVLT_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && n >= 0, "mvlt_lamb_check_tables: n_tensors, n_chunks and n must not be negative, got %d, %d, %ld", n_tensors,
               n_chunks, n);
  MVLT_REQUIRE((tensors || n_tensors == 0) && (chunks || n_chunks == 0), "mvlt_lamb_check_tables: null pointer (tensors and chunks are required)");
  MVLT_REQUIRE(n_groups >= 1 && n_groups <= 254, "mvlt_lamb_check_tables: n_groups must be in [1, 254], got %d", n_groups);
  long next = 0, end = 0;
  for (int t = 0; t < n_tensors; ++t) {
    const int64_t* r = tensors + ROW * (long)t;
    MVLT_REQUIRE(r[0] >= 0 && r[1] >= 0 && r[1] <= n && r[0] <= n - r[1], "mvlt_lamb_check_tables: tensor %d = [%ld, %ld + %ld) points past n = %ld", t,
                 (long)r[0], (long)r[0], (long)r[1], n);
    MVLT_REQUIRE(r[0] % 4 == 0, "mvlt_lamb_check_tables: tensor %d starts at %ld, not a multiple of 4", t, (long)r[0]);
    MVLT_REQUIRE(r[0] >= end, "mvlt_lamb_check_tables: tensor %d starts at %ld, inside or in front of its predecessor (which ends at %ld)", t, (long)r[0], end);
    MVLT_REQUIRE(r[2] >= 0 && r[2] < n_groups, "mvlt_lamb_check_tables: tensor %d names group %ld of %d", t, (long)r[2], n_groups);
    const long want = ((long)r[1] + CHUNK - 1) / CHUNK;
    MVLT_REQUIRE(r[4] == next && r[5] == want, "mvlt_lamb_check_tables: tensor %d of %ld elements owns chunks [%ld, %ld + %ld), expected [%ld, %ld + %ld)", t,
                 (long)r[1], (long)r[4], (long)r[4], (long)r[5], next, next, want);
    next += want;
    end = r[0] + r[1];
  }
  MVLT_REQUIRE(next == n_chunks, "mvlt_lamb_check_tables: the tensors own %ld chunks, the chunk table has %d", next, n_chunks);
  for (int c = 0; c < n_chunks; ++c) {
    const int t = chunks[2 * (long)c], k = chunks[2 * (long)c + 1];
    MVLT_REQUIRE(t >= 0 && t < n_tensors, "mvlt_lamb_check_tables: chunk %d names tensor %d of %d", c, t, n_tensors);
    const int64_t* r = tensors + ROW * (long)t;
    MVLT_REQUIRE(k >= 0 && k < r[5] && r[4] + k == c, "mvlt_lamb_check_tables: chunk %d is {tensor %d, index %d}, but that tensor owns chunks [%ld, %ld + %ld)",
                 c, t, k, (long)r[4], (long)r[4], (long)r[5]);
  }
  return MVLT_OK;
}

extern "C" int mvlt_lamb_moments(const float* p, const float* g, float* m, float* v, long n, const float* hp, const int64_t* tensors, int n_tensors,
                                 const int32_t* chunks, int n_chunks, const float* table, int n_groups, float* partials, const float* gscale_dev,
                                 const float* gate, void* stream) {
  MVLT_REQUIRE(p && g && m && v && hp && tensors && chunks && table && partials,
               "mvlt_lamb_moments: null pointer (p, g, m, v, hp, tensors, chunks, table and partials are required)");
  MVLT_REQUIRE(n >= 0 && n_tensors >= 0 && n_chunks >= 0, "mvlt_lamb_moments: n, n_tensors and n_chunks must not be negative, got %ld, %d, %d", n, n_tensors,
               n_chunks);
  MVLT_REQUIRE(n_groups >= 1 && n_groups <= 254, "mvlt_lamb_moments: n_groups must be in [1, 254], got %d", n_groups);
  MVLT_REQUIRE(!(gscale_dev && gate), "mvlt_lamb_moments: both gscale_dev and gate are given (the gate carries its own coefficient)");
  MVLT_REQUIRE(aligned(p, 16) && aligned(g, 16) && aligned(m, 16) && aligned(v, 16) && aligned(table, 8) && aligned(tensors, 8) && aligned(partials, 8) &&
                   aligned(chunks, 4),
               "mvlt_lamb_moments: p, g, m, v must be 16-byte aligned, table, tensors and partials 8-byte aligned, chunks 4-byte aligned");
  if (n == 0 || n_tensors == 0 || n_chunks == 0) return MVLT_OK;
  if (gate)
    MVLT_LAUNCH((lamb_moments_kernel<true>), dim3((unsigned)n_chunks), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, n, hp, tensors, n_tensors, chunks, table,
                n_groups, partials, gate);
  else
    MVLT_LAUNCH((lamb_moments_kernel<false>), dim3((unsigned)n_chunks), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, n, hp, tensors, n_tensors, chunks, table,
                n_groups, partials, gscale_dev);
  return mvlt_check_launch("mvlt_lamb_moments");
}

extern "C" int mvlt_lamb_fold(const float* partials, int n_chunks, const int64_t* tensors, int n_tensors, const float* table, int n_groups, int flags,
                              float* ratios, const float* gate, void* stream) {
  MVLT_REQUIRE(partials && tensors && table && ratios, "mvlt_lamb_fold: null pointer (partials, tensors, table and ratios are required)");
  MVLT_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "mvlt_lamb_fold: n_tensors and n_chunks must not be negative, got %d, %d", n_tensors, n_chunks);
  MVLT_REQUIRE(n_groups >= 1 && n_groups <= 254, "mvlt_lamb_fold: n_groups must be in [1, 254], got %d", n_groups);
  MVLT_REQUIRE((flags & ~(MVLT_LAMB_ALWAYS_ADAPT | MVLT_LAMB_TRUST_CLIP)) == 0, "mvlt_lamb_fold: unknown flags 0x%x", flags);
  MVLT_REQUIRE(aligned(partials, 8) && aligned(tensors, 8) && aligned(table, 8) && aligned(ratios, 4),
               "mvlt_lamb_fold: partials, tensors and table must be 8-byte aligned, ratios 4-byte aligned");
  if (n_tensors == 0 || n_chunks == 0) return MVLT_OK;
  if (gate)
    MVLT_LAUNCH((lamb_fold_kernel<true>), dim3((unsigned)n_tensors), dim3(NT), 0, (hipStream_t)stream, partials, n_chunks, tensors, table, n_groups, flags,
                ratios, gate);
  else
    MVLT_LAUNCH((lamb_fold_kernel<false>), dim3((unsigned)n_tensors), dim3(NT), 0, (hipStream_t)stream, partials, n_chunks, tensors, table, n_groups, flags,
                ratios, gate);
  return mvlt_check_launch("mvlt_lamb_fold");
}

extern "C" int mvlt_lamb_apply(float* p, const float* m, const float* v, void* p_bf16, long n, const float* hp, const int64_t* tensors, int n_tensors,
                               const int32_t* chunks, int n_chunks, const float* table, int n_groups, const float* ratios, const float* gate, void* stream) {
  MVLT_REQUIRE(p && m && v && hp && tensors && chunks && table && ratios,
               "mvlt_lamb_apply: null pointer (p, m, v, hp, tensors, chunks, table and ratios are required)");
  MVLT_REQUIRE(n >= 0 && n_tensors >= 0 && n_chunks >= 0, "mvlt_lamb_apply: n, n_tensors and n_chunks must not be negative, got %ld, %d, %d", n, n_tensors,
               n_chunks);
  MVLT_REQUIRE(n_groups >= 1 && n_groups <= 254, "mvlt_lamb_apply: n_groups must be in [1, 254], got %d", n_groups);
  MVLT_REQUIRE(aligned(p, 16) && aligned(m, 16) && aligned(v, 16) && aligned(p_bf16, 8) && aligned(table, 8) && aligned(tensors, 8) && aligned(chunks, 4) &&
                   aligned(ratios, 4),
               "mvlt_lamb_apply: p, m, v must be 16-byte aligned, p_bf16, table and tensors 8-byte aligned, chunks and ratios 4-byte aligned");
  if (n == 0 || n_tensors == 0 || n_chunks == 0) return MVLT_OK;
  if (gate)
    MVLT_LAUNCH((lamb_apply_kernel<true>), dim3((unsigned)n_chunks), dim3(NT), 0, (hipStream_t)stream, p, m, v, (bf16*)p_bf16, n, hp, tensors, n_tensors, chunks,
                table, n_groups, ratios, gate);
  else
    MVLT_LAUNCH((lamb_apply_kernel<false>), dim3((unsigned)n_chunks), dim3(NT), 0, (hipStream_t)stream, p, m, v, (bf16*)p_bf16, n, hp, tensors, n_tensors, chunks,
                table, n_groups, ratios, gate);
  return mvlt_check_launch("mvlt_lamb_apply");
}

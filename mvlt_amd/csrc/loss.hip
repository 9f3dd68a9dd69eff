// Cross entropy with label smoothing and class weights over the rows of an fp32 logits matrix (gfx950): F.cross_entropy(x, y, weight=w, ignore_index=i,
// label_smoothing=e), mean reduction, forward and backward.  The plain loss stays where it is (ce_fwd_kernel / ce_loss_finish_kernel / ce_bwd_kernel in
// elementwise.hip); these are their siblings, launched only when an option is on.  Three kernels, no atomics:
//   ce_smooth_fwd_kernel      one workgroup per row, ONE pass over it: lse[r] and, for e > 0, smooth[r] = W lse_r - sum_c w_c x[r, c]
//   ce_smooth_finish_kernel   one workgroup, rows in a fixed order: acc = {numerator of the loss, den = sum of w[y_r] over the kept rows, W = sum_c w_c}
//   ce_smooth_bwd_kernel      one workgroup per row: dlogits[r, k] = (a + b W) p_k - a [k == y_r] - b w_k,  a = (1 - e) w[y_r] g, b = (e / V) g, g = gscale / den
// HBM-bound row reductions like the plain ones (4 B read per logit forward; 4 read + 4 or 2 written backward); the weights are V floats that every row
// re-reads from L2.  include/mvlt_hip_loss.h states the contract, docs/loss_options.md the measurements.
#include "common.h"
#include "../../include/mvlt_hip_loss.h"

namespace {

constexpr int NT = 256;

inline bool aligned(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }

// the -inf-safe shift of ce_fwd_kernel (elementwise.hip): while the running maximum is still -inf, 0 is subtracted instead, so that a row with at least one
// finite logit gets its exact lse wherever the -inf columns lie
__device__ __forceinline__ float ce_shift(float running_max) { return running_max == -INFINITY ? 0.f : running_max; }

// MODE 0: lse alone (e == 0: weights only -- nothing of the row but its lse and its label column enters the loss, and no weight is loaded here).
// MODE 1: + t = sum_c (x_c - x0), unweighted (one subtract and one add per element on top of MODE 0; W = V).
// MODE 2: + t = sum_c w_c (x_c - x0) and W = sum_c w_c, the weights loaded beside the logits.
// The row's smoothing term W lse - sum_c w_c x_c is then W ((max - x0) + log sum) - t: formed directly, both products are ~V |x| and the difference ~V log V,
// so logits near 3e4 would leave one or two digits in fp32; against the pivot x0 = x[r, 0] every addend is of the size of the row's spread.
// The loads are ce_fwd_kernel's: 16-byte, eight in flight per thread, one rescale of the running sum per 32 columns.
template <int MODE>
__global__ __launch_bounds__(NT) void ce_smooth_fwd_kernel(const float* logits, const float* weight, float* lse, float* smooth, int V, int ld) {
  __shared__ float s_m[NT / 64], s_s[NT / 64], s_t[NT / 64], s_w[NT / 64];
  const int row = blockIdx.x;
  const float* lr = logits + (long)row * ld;
  const float piv = MODE > 0 ? lr[0] : 0.f;
  float m = -INFINITY, s = 0.f, t = 0.f, ws = 0.f;
  int c_first = 0;
  if ((ld & 3) == 0 && (((uintptr_t)logits) & 15) == 0 && (MODE < 2 || (((uintptr_t)weight) & 15) == 0)) {
    const int V4 = V & ~3;
    constexpr int U = 8;
    int c = threadIdx.x * 4;
    for (; c + (U - 1) * NT * 4 < V4; c += U * NT * 4) {
      f32x4 x[U], w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = *(const f32x4*)(lr + c + u * NT * 4);
      if constexpr (MODE == 2) {
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = *(const f32x4*)(weight + c + u * NT * 4);
      }
      float nm = m;
#pragma unroll
      for (int u = 0; u < U; ++u) nm = fmaxf(nm, fmaxf(fmaxf(x[u][0], x[u][1]), fmaxf(x[u][2], x[u][3])));
      const float sub = ce_shift(nm);
      float a = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) a += (__expf(x[u][0] - sub) + __expf(x[u][1] - sub)) + (__expf(x[u][2] - sub) + __expf(x[u][3] - sub));
      s = s * __expf(m - sub) + a;
      m = nm;
      if constexpr (MODE == 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) t += ((x[u][0] - piv) + (x[u][1] - piv)) + ((x[u][2] - piv) + (x[u][3] - piv));
      }
      if constexpr (MODE == 2) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          t += (w[u][0] * (x[u][0] - piv) + w[u][1] * (x[u][1] - piv)) + (w[u][2] * (x[u][2] - piv) + w[u][3] * (x[u][3] - piv));
          ws += (w[u][0] + w[u][1]) + (w[u][2] + w[u][3]);
        }
      }
    }
    for (; c < V4; c += NT * 4) {
      const f32x4 x = *(const f32x4*)(lr + c);
      const float nm = fmaxf(m, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
      const float sub = ce_shift(nm);
      s = s * __expf(m - sub) + (__expf(x[0] - sub) + __expf(x[1] - sub)) + (__expf(x[2] - sub) + __expf(x[3] - sub));
      m = nm;
      if constexpr (MODE == 1) t += ((x[0] - piv) + (x[1] - piv)) + ((x[2] - piv) + (x[3] - piv));
      if constexpr (MODE == 2) {
        const f32x4 w = *(const f32x4*)(weight + c);
        t += (w[0] * (x[0] - piv) + w[1] * (x[1] - piv)) + (w[2] * (x[2] - piv) + w[3] * (x[3] - piv));
        ws += (w[0] + w[1]) + (w[2] + w[3]);
      }
    }
    c_first = V4;
  }
  // rows off the 16-byte grid (a base pointer or an ld that is no multiple of 4 floats) and the V & 3 tail: element by element
  for (int c = c_first + threadIdx.x; c < V; c += NT) {
    const float x = lr[c];
    const float nm = fmaxf(m, x);
    const float sub = ce_shift(nm);
    s = s * __expf(m - sub) + __expf(x - sub);
    m = nm;
    if constexpr (MODE == 1) t += x - piv;
    if constexpr (MODE == 2) {
      const float w = weight[c];
      t += w * (x - piv);
      ws += w;
    }
  }
  // combine the (m, s) pairs, wave then block, as ce_fwd_kernel does; t and W are plain sums in the same fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o), os = __shfl_xor(s, o);
    const float nm = fmaxf(m, om);
    const float sub = ce_shift(nm);
    s = s * __expf(m - sub) + os * __expf(om - sub);
    m = nm;
  }
  if constexpr (MODE > 0) t = wave_sum(t);
  if constexpr (MODE == 2) ws = wave_sum(ws);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_m[wave] = m; s_s[wave] = s; s_t[wave] = t; s_w[wave] = ws; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = s_m[0], S = s_s[0];
    for (int w = 1; w < NT / 64; ++w) {
      const float nm = fmaxf(M, s_m[w]);
      const float sub = ce_shift(nm);
      S = S * __expf(M - sub) + s_s[w] * __expf(s_m[w] - sub);
      M = nm;
    }
    const float ls = logf(S);
    lse[row] = M + ls;
    if constexpr (MODE > 0) {
      const float T = (s_t[0] + s_t[1]) + (s_t[2] + s_t[3]);
      const float W = MODE == 2 ? (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]) : (float)V;
      smooth[row] = W * ((M - piv) + ls) - T;         // lse - x0 WITHOUT the rounding of lse itself (half an ulp of 3e4 is 2e-3, times W)
    }
  }
}
static_assert(NT / 64 == 4, "the block combine above adds four waves");

// acc = {sum over the kept rows of (1 - e) w[y_r] (lse_r - x[r, y_r]) + (e / V) smooth[r],  den = sum over the kept rows of w[y_r],  W = sum_c w_c}.
// ONE workgroup, a fixed order, plain stores (ce_loss_finish_kernel's reasons: two atomics per row were the whole cost of the row kernel once).  A label
// outside [0, V) that is not `ignore` reads nothing and makes the numerator NaN.
__global__ __launch_bounds__(1024) void ce_smooth_finish_kernel(const float* logits, const long* labels, long ignore, float e, const float* weight,
                                                                 const float* lse, const float* smooth, float* acc, int rows, int V, int ld) {
  __shared__ float s_l[16], s_d[16], s_w[16];
  const float ev = e / (float)V;
  float l = 0.f, d = 0.f, w = 0.f;
  for (int r = threadIdx.x; r < rows; r += 1024) {
    const long lab = labels[r];
    if (lab == ignore) continue;
    if ((unsigned long)lab >= (unsigned long)V) { l = __builtin_nanf(""); continue; }
    const float wy = weight ? weight[lab] : 1.f;
    float term = (1.f - e) * wy * (lse[r] - logits[(long)r * ld + lab]);
    if (e > 0.f) term += ev * smooth[r];
    l += term;
    d += wy;
  }
  if (weight) {
    // eight independent loads per trip: one load per trip left this single workgroup waiting out 30 memory round trips in a row at V = 30522 (+8 us)
    constexpr int U = 8;
    for (int c = threadIdx.x; c < V; c += 1024 * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = c + u * 1024 < V ? weight[c + u * 1024] : 0.f;
      w += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
  }
  l = wave_sum(l); d = wave_sum(d); w = wave_sum(w);
  if ((threadIdx.x & 63) == 0) { s_l[threadIdx.x >> 6] = l; s_d[threadIdx.x >> 6] = d; s_w[threadIdx.x >> 6] = w; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f, D = 0.f, W = 0.f;
    for (int k = 0; k < 16; ++k) { L += s_l[k]; D += s_d[k]; W += s_w[k]; }
    acc[0] = L;
    acc[1] = D;
    acc[2] = weight ? W : (float)V;
  }
}

// dlogits[r, k] = keep_r [ (1 - e) w[y_r] (p_k - [k == y_r]) + (e / V) (W p_k - w_k) ] gscale / den
//               = cp p_k - a [k == y_r] - b w_k,   a = (1 - e) w[y_r] g,  b = (e / V) g,  cp = a + b W,  g = keep_r gscale / den  (den > 0, else 0: no clamp --
// with weights den < 1 is legitimate).  Unweighted: w_k = 1, W = V, cp = g.  The vector / scalar split and the zeroed padding columns [V, ldd) are ce_bwd_kernel's.
template <typename TO, bool HASW>
__global__ __launch_bounds__(NT) void ce_smooth_bwd_kernel(const float* logits, const long* labels, long ignore, float e, const float* weight, const float* lse,
                                                            const float* gscale, const float* acc, TO* dlogits, int V, int ld, int ldd) {
  const int row = blockIdx.x;
  const float* lr = logits + (long)row * ld;
  TO* dr = dlogits + (long)row * ldd;
  const long lab = labels[row];
  const float l = lse[row];
  const float den = acc[1];
  const bool keep = lab != ignore, valid = (unsigned long)lab < (unsigned long)V;
  float g = keep ? gscale[0] * (den > 0.f ? 1.0f / den : 0.f) : 0.f;
  if (keep && !valid) g = __builtin_nanf("");                            // a label that names no class: the row's gradient says so
  const float wy = (HASW && keep && valid) ? weight[lab] : 1.f;
  const float a = (1.f - e) * wy * g, b = (e / (float)V) * g;
  const float cp = HASW ? a + b * acc[2] : g;
  int c_first = 0;
  if ((ld & 3) == 0 && (ldd & 3) == 0 && (((uintptr_t)logits) & 15) == 0 && (((uintptr_t)dlogits) & 15) == 0 && (!HASW || (((uintptr_t)weight) & 15) == 0)) {
    const int V4 = V & ~3;
    for (int c = threadIdx.x * 4; c < V4; c += NT * 4) {
      const f32x4 x = *(const f32x4*)(lr + c);
      f32x4 bw = {b, b, b, b};
      if constexpr (HASW) bw = *(const f32x4*)(weight + c) * b;
      f32x4 gk;
#pragma unroll
      for (int k = 0; k < 4; ++k) gk[k] = cp * __expf(x[k] - l) - (c + k == lab ? a : 0.f) - bw[k];
      if constexpr (sizeof(TO) == 2) *(bf16x4*)((bf16*)dr + c) = bf16x4{(bf16)gk[0], (bf16)gk[1], (bf16)gk[2], (bf16)gk[3]};
      else *(f32x4*)((float*)dr + c) = gk;
    }
    c_first = V4;
  }
  for (int c = c_first + threadIdx.x; c < ldd; c += NT) {
    float gk = 0.f;
    if (c < V) gk = cp * __expf(lr[c] - l) - (c == lab ? a : 0.f) - (HASW ? weight[c] * b : b);
    dr[c] = (TO)gk;                        // padding columns [V, ldd) are zeroed
  }
}

int check_common(const char* fn, const void* logits, const long* labels, float e, int rows, int V, int ld, int dtype) {
  MVLT_REQUIRE(logits && labels, "%s: null pointer (logits and labels are required)", fn);
  MVLT_REQUIRE(rows >= 0, "%s: rows must not be negative, got %d", fn, rows);
  MVLT_REQUIRE(V > 0, "%s: V must be positive, got %d", fn, V);
  MVLT_REQUIRE(ld >= V, "%s: ld = %d is smaller than V = %d", fn, ld, V);
  MVLT_REQUIRE(e >= 0.f && e < 1.f, "%s: label_smoothing must be in [0, 1), got %g", fn, (double)e);
  MVLT_REQUIRE(dtype == 1, "%s: the logits must be fp32 (dtype 1), got dtype %d", fn, dtype);
  MVLT_REQUIRE(aligned(logits, 4) && aligned(labels, 8), "%s: logits must be 4-byte aligned, labels 8-byte aligned", fn);
  return MVLT_OK;
}

}  // namespace

extern "C" int mvlt_loss_version(void) { return MVLT_LOSS_VERSION; }

extern "C" int mvlt_ce_smooth_fwd(const void* logits, const long* labels, long ignore_index, float label_smoothing, const float* weight, float* lse,
                                  float* smooth, float* acc, int rows, int V, int ld, int dtype, void* stream) {
  if (const int rc = check_common("mvlt_ce_smooth_fwd", logits, labels, label_smoothing, rows, V, ld, dtype)) return rc;
  MVLT_REQUIRE(lse && smooth && acc, "mvlt_ce_smooth_fwd: null pointer (lse, smooth and acc are required)");
  MVLT_REQUIRE(aligned(lse, 4) && aligned(smooth, 4) && aligned(acc, 4) && aligned(weight, 4), "mvlt_ce_smooth_fwd: lse, smooth, acc and weight must be 4-byte aligned");
  const float* x = (const float*)logits;
  hipStream_t s = (hipStream_t)stream;
  if (rows > 0) {
    const dim3 grid((unsigned)rows), block(NT);
    if (label_smoothing == 0.f) MVLT_LAUNCH((ce_smooth_fwd_kernel<0>), grid, block, 0, s, x, weight, lse, smooth, V, ld);
    else if (!weight) MVLT_LAUNCH((ce_smooth_fwd_kernel<1>), grid, block, 0, s, x, weight, lse, smooth, V, ld);
    else MVLT_LAUNCH((ce_smooth_fwd_kernel<2>), grid, block, 0, s, x, weight, lse, smooth, V, ld);
  }
  MVLT_LAUNCH(ce_smooth_finish_kernel, dim3(1), dim3(1024), 0, s, x, labels, ignore_index, label_smoothing, weight, (const float*)lse, (const float*)smooth, acc,
              rows, V, ld);
  return mvlt_check_launch("mvlt_ce_smooth_fwd");
}

extern "C" int mvlt_ce_smooth_bwd(const void* logits, const long* labels, long ignore_index, float label_smoothing, const float* weight, const float* lse,
                                  const float* gscale, const float* acc, void* dlogits, int rows, int V, int ld, int ldd, int dtype, int out_dtype, void* stream) {
  if (const int rc = check_common("mvlt_ce_smooth_bwd", logits, labels, label_smoothing, rows, V, ld, dtype)) return rc;
  MVLT_REQUIRE(lse && gscale && acc && dlogits, "mvlt_ce_smooth_bwd: null pointer (lse, gscale, acc and dlogits are required)");
  MVLT_REQUIRE(ldd >= V, "mvlt_ce_smooth_bwd: ldd = %d is smaller than V = %d", ldd, V);
  MVLT_REQUIRE(out_dtype == 0 || out_dtype == 1, "mvlt_ce_smooth_bwd: dlogits must be bf16 (0) or fp32 (1), got out_dtype %d", out_dtype);
  MVLT_REQUIRE(aligned(lse, 4) && aligned(gscale, 4) && aligned(acc, 4) && aligned(weight, 4) && aligned(dlogits, out_dtype == 0 ? 2 : 4),
               "mvlt_ce_smooth_bwd: lse, gscale, acc and weight must be 4-byte aligned, dlogits aligned to its element");
  if (rows == 0) return MVLT_OK;
  const float* x = (const float*)logits;
  const dim3 grid((unsigned)rows), block(NT);
  hipStream_t s = (hipStream_t)stream;
  const float e = label_smoothing;
  if (out_dtype == 0 && weight) MVLT_LAUNCH((ce_smooth_bwd_kernel<bf16, true>), grid, block, 0, s, x, labels, ignore_index, e, weight, lse, gscale, acc, (bf16*)dlogits, V, ld, ldd);
  else if (out_dtype == 0) MVLT_LAUNCH((ce_smooth_bwd_kernel<bf16, false>), grid, block, 0, s, x, labels, ignore_index, e, weight, lse, gscale, acc, (bf16*)dlogits, V, ld, ldd);
  else if (weight) MVLT_LAUNCH((ce_smooth_bwd_kernel<float, true>), grid, block, 0, s, x, labels, ignore_index, e, weight, lse, gscale, acc, (float*)dlogits, V, ld, ldd);
  else MVLT_LAUNCH((ce_smooth_bwd_kernel<float, false>), grid, block, 0, s, x, labels, ignore_index, e, weight, lse, gscale, acc, (float*)dlogits, V, ld, ldd);
  return mvlt_check_launch("mvlt_ce_smooth_bwd");
}

// Device-side image ingest (docs/ingest.md): what the reference's dataset does per sample on the host between the decoder and the grid mask -- the content
// crop (mcloader/fashion_gen.py:411-428), transforms.Resize + ToTensor (+ Normalize) (:108-111), a horizontal flip -- from the uint8 pixels the loader decoded,
// writing the clean fp32 image and its grid-masked copy (:176) in ONE pass: 1 byte per pixel channel crosses the link instead of 4, and the masked copy costs no
// second read of the image.
#include "common.h"
#include "philox.h"
#include "../../include/mvlt_hip_ingest.h"

namespace {
constexpr int NT = 256;

// ---- no resampling: a pure streaming pass.  One thread owns 4 consecutive pixels of one row: 12 contiguous source bytes (three 4-byte loads, lane after lane:
// the HWC -> CHW transpose happens in registers, never as byte-strided loads) or one 4-byte load per plane (CHW), three 16-byte stores per output.
template <bool VEC>
__global__ __launch_bounds__(NT) void ingest_kernel(const uint8_t* src, int layout, const float* table, float* image, float* masked, const uint8_t* flags,
                                                    long ngroups, int H, int W, int patch, float fill) {
  __shared__ float tab[3 * 256];
  for (int t = threadIdx.x; t < 3 * 256; t += NT) tab[t] = table[t];
  __syncthreads();
  const int W4 = (W + 3) / 4;
  const int gh = flags ? H / patch : 0, gw = flags ? W / patch : 0;
  const long plane = (long)H * W;
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < ngroups; i += (long)gridDim.x * NT) {
    const int x0 = (int)(i % W4) * 4;
    const long r = i / W4;                 // b*H + y
    const int y = (int)(r % H);
    const long b = r / H;
    uint32_t v[3][4];
    if constexpr (VEC) {
      if (layout == 0) {
        const uint32_t* p = (const uint32_t*)(src + (r * W + x0) * 3);
        const uint32_t wd[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k % 3][k / 3] = (wd[k >> 2] >> (8 * (k & 3))) & 255u;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t wd = *(const uint32_t*)(src + ((b * 3 + c) * H + y) * (long)W + x0);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[c][e] = (wd >> (8 * e)) & 255u;
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int x = x0 + e < W ? x0 + e : W - 1;
          v[c][e] = layout == 0 ? src[(r * W + x) * 3 + c] : src[((b * 3 + c) * H + y) * (long)W + x];
        }
    }
    bool m[4] = {false, false, false, false};
    if (flags) {
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = x0 + e < W && flags[(b * gh + y / patch) * gw + (x0 + e) / patch];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 o = {tab[c * 256 + v[c][0]], tab[c * 256 + v[c][1]], tab[c * 256 + v[c][2]], tab[c * 256 + v[c][3]]};
      const f32x4 om = {m[0] ? fill : o[0], m[1] ? fill : o[1], m[2] ? fill : o[2], m[3] ? fill : o[3]};
      const long at = (b * 3 + c) * plane + (long)y * W + x0;
      if constexpr (VEC) {
        *(f32x4*)(image + at) = o;
        if (masked) *(f32x4*)(masked + at) = om;
      } else {
        for (int e = 0; e < 4 && x0 + e < W; ++e) {
          image[at + e] = o[e];
          if (masked) masked[at + e] = om[e];
        }
      }
    }
  }
}

// ---- resampling.  The taps of output index i along an axis of n input and m output samples, D = 2 max(n, m): the x in [0, n) with |(2x+1) m - (2i+1) n| < D.
// They are the integers of [tap_lo, tap_hi): the smallest x with (2x+1) m > (2i+1) n - D, and the smallest x with (2x+1) m >= (2i+1) n + D, clipped to n.
__device__ __forceinline__ int tap_lo(int i, int n, int m, int D) {
  const int a = (2 * i + 1) * n - D - m;           // 2 m x > a
  return a < 0 ? 0 : a / (2 * m) + 1;
}
__device__ __forceinline__ int tap_hi(int i, int n, int m, int D) {
  const int a = (2 * i + 1) * n + D - m;           // 2 m x >= a, a > 0
  const int x = (a + 2 * m - 1) / (2 * m);
  return x < n ? x : n;
}
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

constexpr int MAXF = MVLT_INGEST_MAX_FACTOR;
constexpr int TH = 8, TW = 32;                       // output rows x columns of a workgroup
constexpr int RMAX = (TH + 1) * MAXF + 1;            // source rows under a band: tap_hi(i0+TH-1) - tap_lo(i0) <= (TH+1) n/m + 1
constexpr int PXMAX = (TW + 1) * MAXF + 1;           // source pixels under a tile, the same way
constexpr int RC = 16;                               // raw source rows staged at a time
constexpr int RAWW = (PXMAX * 3 + 3 + 3) / 4;        // dwords of one staged row: its bytes plus up to 3 in front of them (the row is loaded from a 4-byte boundary)

// One workgroup: sample blockIdx.z, output rows [i0, i0+TH) x columns [j0, j0+TW) (columns counted BEFORE the flip).  Per chunk of RC source rows: the bytes under
// the tile come in by coalesced 4-byte loads into LDS, the horizontal pass turns them into fp32 intermediates in LDS (one thread per source row x output column,
// three channels); then the vertical pass reads 16 bytes of intermediates per tap and stores 16 bytes per output.
__global__ __launch_bounds__(NT) void ingest_resize_kernel(const uint8_t* src, long src_bytes, int Hmax, int Wmax, const int* rects, const uint8_t* flip,
                                                           const float* norm, float* image, float* masked, const uint8_t* flags, int H, int W, int patch,
                                                           float fill, int vec) {
  __shared__ uint32_t raw[RC][RAWW];
  __shared__ __attribute__((aligned(16))) float inter[3][RMAX][TW];
  const int b = blockIdx.z, i0 = blockIdx.y * TH, j0 = blockIdx.x * TW, tid = threadIdx.x;
  const int y0 = rects[4 * b], x0 = rects[4 * b + 1], h = rects[4 * b + 2], w = rects[4 * b + 3];
  // what the entry point refused on the host copy: a device copy that disagrees must not make this kernel read outside the slab or write outside its LDS
  if (h < 1 || w < 1 || y0 < 0 || x0 < 0 || y0 > Hmax - h || x0 > Wmax - w || h > MAXF * H || w > MAXF * W) return;
  const int Dx = 2 * (w > W ? w : W), Dy = 2 * (h > H ? h : H);
  const int i1 = i0 + TH < H ? i0 + TH : H, j1 = j0 + TW < W ? j0 + TW : W;
  const int xa = tap_lo(j0, w, W, Dx), xb = tap_hi(j1 - 1, w, W, Dx);
  const int ra = tap_lo(i0, h, H, Dy), rb = tap_hi(i1 - 1, h, H, Dy);
  const int nbytes = (xb - xa) * 3;
  for (int rc = ra; rc < rb; rc += RC) {
    const int nr = rb - rc < RC ? rb - rc : RC;
    for (int idx = tid; idx < nr * RAWW; idx += NT) {
      const int rr = idx / RAWW, dw = idx - rr * RAWW;
      const long g = (((long)b * Hmax + y0 + rc + rr) * Wmax + x0 + xa) * 3;
      const int off = (int)(g & 3);
      if (dw * 4 < off + nbytes) {
        const long at = (g - off) + 4L * dw;
        uint32_t word = 0;
        if (at + 4 <= src_bytes) word = *(const uint32_t*)(src + at);
        else for (int e = 0; at + e < src_bytes; ++e) word |= (uint32_t)src[at + e] << (8 * e);       // the last bytes of the slab
        raw[rr][dw] = word;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nr * TW; idx += NT) {
      const int rr = idx / TW, jl = idx % TW, j = j0 + jl;
      if (j >= j1) continue;
      const long g = (((long)b * Hmax + y0 + rc + rr) * Wmax + x0 + xa) * 3;
      const uint8_t* px = (const uint8_t*)raw[rr] + (int)(g & 3);
      const int lo = tap_lo(j, w, W, Dx), hi = tap_hi(j, w, W, Dx);
      int s0 = 0, s1 = 0, s2 = 0, ws = 0;
      for (int x = lo; x < hi; ++x) {
        const int wt = Dx - iabs((2 * x + 1) * W - (2 * j + 1) * w);
        const uint8_t* p = px + (x - xa) * 3;
        s0 += wt * p[0]; s1 += wt * p[1]; s2 += wt * p[2];
        ws += wt;
      }
      const float fws = (float)ws;
      const int row = rc - ra + rr;
      inter[0][row][jl] = __fdiv_rn((float)s0, fws);
      inter[1][row][jl] = __fdiv_rn((float)s1, fws);
      inter[2][row][jl] = __fdiv_rn((float)s2, fws);
    }
    __syncthreads();
  }
  if (tid >= 3 * TH * (TW / 4)) return;
  const int c = tid / (TH * (TW / 4)), rem = tid % (TH * (TW / 4));
  const int i = i0 + rem / (TW / 4), jg = j0 + (rem % (TW / 4)) * 4;
  if (i >= i1 || jg >= j1) return;
  const int lo = tap_lo(i, h, H, Dy), hi = tap_hi(i, h, H, Dy);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int ws = 0;
  for (int y = lo; y < hi; ++y) {
    const int wt = Dy - iabs((2 * y + 1) * H - (2 * i + 1) * h);
    const float fw = (float)wt;
    const f32x4 v = *(const f32x4*)&inter[c][y - ra][jg - j0];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(fw, v[e], acc[e]);
    ws += wt;
  }
  const float fws = (float)ws;
  const bool fl = flip && flip[b];
  const int gh = flags ? H / patch : 0, gw = flags ? W / patch : 0;
  float o[4], om[4];                                    // by OUTPUT position: o[e] is column xo + e
  const int xo = fl ? W - 4 - jg : jg;                  // (vec: W % 4 == 0, so every group is whole)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float r = __fdiv_rn(__fdiv_rn(acc[fl ? 3 - e : e], fws), 255.0f);
    if (norm) r = __fdiv_rn(__fsub_rn(r, norm[c]), norm[3 + c]);
    o[e] = r;
    const int x = xo + e;
    const bool m = flags && x >= 0 && x < W && flags[((long)b * gh + i / patch) * gw + x / patch];
    om[e] = m ? fill : r;
  }
  const long at = (((long)b * 3 + c) * H + i) * W + xo;
  if (vec) {
    *(f32x4*)(image + at) = f32x4{o[0], o[1], o[2], o[3]};
    if (masked) *(f32x4*)(masked + at) = f32x4{om[0], om[1], om[2], om[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = fl ? jg + 3 - e : jg + e;            // the column (before the flip) behind output position xo + e
      if (j < j1) {
        image[at + e] = o[e];
        if (masked) masked[at + e] = om[e];
      }
    }
  }
}

__global__ __launch_bounds__(NT) void flip_flags_kernel(uint8_t* flip, int B, uint32_t threshold, uint64_t seed, uint64_t sample0) {
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b < B) flip[b] = (draws(seed, sample0 + b, 0, 6).x >> 8) < threshold;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
}  // namespace

extern "C" int mvlt_ingest_version(void) { return MVLT_INGEST_VERSION; }

static int check_outputs(const char* who, const float* image, const float* masked, const uint8_t* flags, int B, int H, int W, int patch) {
  MVLT_REQUIRE(image && B >= 0 && H > 0 && W > 0, "%s: bad arguments (image must not be null, B >= 0, H and W positive)", who);
  MVLT_REQUIRE(H <= MVLT_INGEST_MAX_SIDE && W <= MVLT_INGEST_MAX_SIDE, "%s: H = %d, W = %d exceed %d", who, H, W, MVLT_INGEST_MAX_SIDE);
  MVLT_REQUIRE((masked != nullptr) == (flags != nullptr), "%s: masked and flags go together (both or neither)", who);
  MVLT_REQUIRE(aligned(image, 4) && aligned(masked, 4), "%s: image / masked must be 4-byte aligned", who);
  if (flags) MVLT_REQUIRE(patch > 0 && H % patch == 0 && W % patch == 0, "%s: H = %d and W = %d must be multiples of patch = %d when flags are given", who, H, W, patch);
  return MVLT_OK;
}

extern "C" int mvlt_image_ingest(const uint8_t* src, int layout, const float* table, float* image, float* masked, const uint8_t* flags, int B, int H, int W,
                                 int patch, float fill, void* stream) {
  if (int rc = check_outputs("mvlt_image_ingest", image, masked, flags, B, H, W, patch)) return rc;
  MVLT_REQUIRE(src && table && aligned(table, 4), "mvlt_image_ingest: src and table must not be null (table 4-byte aligned)");
  MVLT_REQUIRE(layout == 0 || layout == 1, "mvlt_image_ingest: layout must be 0 (B,H,W,3) or 1 (B,3,H,W), got %d", layout);
  const long ngroups = (long)B * H * ((W + 3) / 4);
  if (ngroups == 0) return MVLT_OK;
  const bool vec = W % 4 == 0 && aligned(src, 4) && aligned(image, 16) && aligned(masked, 16);
  const long blocks = (ngroups + NT - 1) / NT;
  const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
  if (vec) MVLT_LAUNCH(ingest_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, src, layout, table, image, masked, flags, ngroups, H, W, patch, fill);
  else MVLT_LAUNCH(ingest_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, src, layout, table, image, masked, flags, ngroups, H, W, patch, fill);
  return mvlt_check_launch("mvlt_image_ingest");
}

extern "C" int mvlt_image_ingest_resize(const uint8_t* src, int Hmax, int Wmax, const int* rects, const int* rects_host, const uint8_t* flip, const float* norm,
                                        float* image, float* masked, const uint8_t* flags, int B, int H, int W, int patch, float fill, void* stream) {
  if (int rc = check_outputs("mvlt_image_ingest_resize", image, masked, flags, B, H, W, patch)) return rc;
  MVLT_REQUIRE(src && rects && rects_host, "mvlt_image_ingest_resize: src, rects and rects_host must not be null");
  MVLT_REQUIRE(aligned(src, 4) && aligned(rects, 4) && aligned(rects_host, 4) && aligned(norm, 4), "mvlt_image_ingest_resize: src, rects and norm must be 4-byte aligned");
  MVLT_REQUIRE(Hmax > 0 && Wmax > 0 && Hmax <= MVLT_INGEST_MAX_SIDE && Wmax <= MVLT_INGEST_MAX_SIDE, "mvlt_image_ingest_resize: the slab must be 1 .. %d pixels a side, got %d x %d",
               MVLT_INGEST_MAX_SIDE, Hmax, Wmax);
  MVLT_REQUIRE(B <= 65535, "mvlt_image_ingest_resize: at most 65535 samples per call, got %d", B);
  for (int b = 0; b < B; ++b) {
    const int y0 = rects_host[4 * b], x0 = rects_host[4 * b + 1], h = rects_host[4 * b + 2], w = rects_host[4 * b + 3];
    MVLT_REQUIRE(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 <= Hmax - h && x0 <= Wmax - w,
                 "mvlt_image_ingest_resize: rectangle %d {y0 %d, x0 %d, h %d, w %d} leaves the %d x %d slab", b, y0, x0, h, w, Hmax, Wmax);
    MVLT_REQUIRE(h <= MAXF * H && w <= MAXF * W, "mvlt_image_ingest_resize: rectangle %d (%d x %d -> %d x %d) exceeds the maximum downscale factor %d", b, h, w, H, W, MAXF);
  }
  if (B == 0) return MVLT_OK;
  const int vec = W % 4 == 0 && aligned(image, 16) && aligned(masked, 16);
  const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, B);
  MVLT_LAUNCH(ingest_resize_kernel, grid, dim3(NT), 0, (hipStream_t)stream, src, (long)B * Hmax * Wmax * 3, Hmax, Wmax, rects, flip, norm, image, masked, flags, H, W,
              patch, fill, vec);
  return mvlt_check_launch("mvlt_image_ingest_resize");
}

extern "C" int mvlt_flip_flags(uint8_t* flip, int B, float p, uint64_t seed, uint64_t sample0, void* stream) {
  MVLT_REQUIRE(flip && B >= 0, "mvlt_flip_flags: bad arguments");
  MVLT_REQUIRE(p >= 0.f && p <= 1.f, "mvlt_flip_flags: p must be in [0, 1]");
  if (B == 0) return MVLT_OK;
  const uint32_t threshold = (uint32_t)__builtin_rint((double)p * 16777216.0);
  MVLT_LAUNCH(flip_flags_kernel, dim3((B + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, flip, B, threshold, seed, sample0);
  return mvlt_check_launch("mvlt_flip_flags");
}

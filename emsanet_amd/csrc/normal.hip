// The surface-normal task on device: L1 loss, multi-scale targets, augmentation, unit-length
// post-processing and the mean angular error.  The task-specific code of the reference lives in the
// un-vendored nicr_mt_scene_analysis library, so every rule is a restatement ([U]); the rules are stated
// in emsanet_amd/loss.py, targets.py, augment.py, postprocessing.py and metrics.py and pinned by
// tests/normal_reference.py.  All kernels are single passes at HBM rate:
//   l1 fwd / bwd   sum over valid pixels of |p - t| / (3 n_valid); a pixel is valid iff its target is
//                  not exactly (0, 0, 0).  Per-workgroup partials in fixed slots, a fixed-order second
//                  stage with fp64 / integer sums: bit-reproducible
//   targets        every scale from the full-resolution map in one launch (the scale is a grid dimension)
//   augment        the composed resize / crop / flip index of csrc/augment.hip with the nearest rule;
//                  channel 0 is negated on a flipped sample
//   unit           v / max(|v|, 1e-12)
//   angular error  atan2(|p x t|, p . t) per valid pixel, rounded once to 2^-20 rad and added as an
//                  integer: the sums do not depend on the launch geometry or the order of the atomics
// A ground-truth map is [n][h][w][3] (HWC) or [n][3][h][w] (CHW); the maps written here are HWC.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxDim = 32767;
constexpr int kMaxResized = 16384;                 // as csrc/augment.hip
constexpr int kMaxSide = 4096;
constexpr long kMaxElements = 0x7FFFFFFFl;         // flat element indices are 32-bit
constexpr float kAngleOne = (float)EMSA_NORMAL_ANGLE_ONE;

int grid_for(long items) {
  long g = (items + kThreads - 1) / kThreads;
  return (int)(g > kMaxBlocks ? kMaxBlocks : (g < 1 ? 1 : g));
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// the three components of ground-truth pixel p of a map with hw pixels per image
__device__ __forceinline__ void load_gt(const float* __restrict__ t, uint32_t hw, int chw, uint32_t p,
                                        float& a, float& b, float& c) {
  if (chw) {
    const uint32_t img = p / hw, r = p - img * hw;
    const float* base = t + (long)img * 3 * hw + r;
    a = base[0];
    b = base[hw];
    c = base[2 * (long)hw];
  } else {
    const float* base = t + (long)p * 3;
    a = base[0];
    b = base[1];
    c = base[2];
  }
}

template <bool VEC>
__device__ __forceinline__ void load_pred(const float* __restrict__ x, int ld, long p, float& a, float& b,
                                          float& c) {
  if (VEC) {                                       // one 16-byte chunk of the pixel's row
    const float4 v = emsa_ld4(x + p * ld);
    a = v.x;
    b = v.y;
    c = v.z;
  } else {
    a = x[p * ld];
    b = x[p * ld + 1];
    c = x[p * ld + 2];
  }
}

// ---- L1 loss -------------------------------------------------------------------------------------
// partial: float[blocks] sums of |p - t|, then uint32[blocks] numbers of valid pixels
template <bool VEC>
__global__ __launch_bounds__(kThreads) void normal_l1_fwd_kernel(
    const float* __restrict__ pred, int ld, const float* __restrict__ target, uint32_t hw, int chw,
    uint32_t pixels, float* __restrict__ partial) {
  __shared__ float red_s[kThreads / EMSA_WAVE];
  __shared__ uint32_t red_n[kThreads / EMSA_WAVE];
  float s = 0.f;
  uint32_t cnt = 0u;
  for (long p = blockIdx.x * (long)kThreads + threadIdx.x; p < (long)pixels; p += (long)gridDim.x * kThreads) {
    float t0, t1, t2;
    load_gt(target, hw, chw, (uint32_t)p, t0, t1, t2);
    if (t0 == 0.f && t1 == 0.f && t2 == 0.f) continue;
    float p0, p1, p2;
    load_pred<VEC>(pred, ld, p, p0, p1, p2);
    s += fabsf(p0 - t0) + fabsf(p1 - t1) + fabsf(p2 - t2);
    cnt += 1u;
  }
  // deterministic block reduction: wave shuffles, then the 4 waves through LDS
#pragma unroll
  for (int o = EMSA_WAVE / 2; o > 0; o >>= 1) {
    s += __shfl_down(s, o);
    cnt += __shfl_down(cnt, o);
  }
  if ((threadIdx.x & (EMSA_WAVE - 1)) == 0) {
    red_s[threadIdx.x / EMSA_WAVE] = s;
    red_n[threadIdx.x / EMSA_WAVE] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f;
    uint32_t b = 0u;
#pragma unroll
    for (int k = 0; k < kThreads / EMSA_WAVE; ++k) {
      a += red_s[k];
      b += red_n[k];
    }
    partial[blockIdx.x] = a;
    reinterpret_cast<uint32_t*>(partial)[gridDim.x + blockIdx.x] = b;
  }
}

// out[0] = loss, out[1] = n_valid as fp32 (exact up to 2^24, what the backward divides by); fixed
// summation order, fp64 sum and an integer count
__global__ __launch_bounds__(kThreads) void normal_l1_finalize_kernel(const float* __restrict__ partial,
                                                                      int n, float* __restrict__ out) {
  __shared__ double sa[kThreads];
  __shared__ unsigned long long sb[kThreads];
  const uint32_t* counts = reinterpret_cast<const uint32_t*>(partial) + n;
  double a = 0.0;
  unsigned long long b = 0ull;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    a += (double)partial[i];
    b += counts[i];
  }
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sa[threadIdx.x] += sa[threadIdx.x + o];
      sb[threadIdx.x] += sb[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = sb[0] ? (float)(sa[0] / (3.0 * (double)sb[0])) : 0.f;
    out[1] = (float)sb[0];
  }
}

// every element of the ld_d-wide gradient rows: g sign(p - t) / (3 n_valid) in the three channels of a
// valid pixel, 0 elsewhere and in the padding
template <bool VEC, bool VEC_D>
__global__ __launch_bounds__(kThreads) void normal_l1_bwd_kernel(
    const float* __restrict__ pred, int ld, const float* __restrict__ target, uint32_t hw, int chw,
    uint32_t pixels, const float* __restrict__ sums, const float* __restrict__ gout,
    float* __restrict__ d, int ld_d) {
  const float nv = sums[1];
  const float k = nv > 0.f ? gout[0] / (3.f * nv) : 0.f;
  for (long p = blockIdx.x * (long)kThreads + threadIdx.x; p < (long)pixels; p += (long)gridDim.x * kThreads) {
    float t0, t1, t2;
    load_gt(target, hw, chw, (uint32_t)p, t0, t1, t2);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (!(t0 == 0.f && t1 == 0.f && t2 == 0.f)) {
      float p0, p1, p2;
      load_pred<VEC>(pred, ld, p, p0, p1, p2);
      const float e0 = p0 - t0, e1 = p1 - t1, e2 = p2 - t2;
      g0 = e0 > 0.f ? k : (e0 < 0.f ? -k : 0.f);
      g1 = e1 > 0.f ? k : (e1 < 0.f ? -k : 0.f);
      g2 = e2 > 0.f ? k : (e2 < 0.f ? -k : 0.f);
    }
    float* row = d + p * ld_d;
    if (VEC_D) {
      emsa_st4(row, make_float4(g0, g1, g2, 0.f));
      for (int c = 4; c < ld_d; c += 4) emsa_st4(row + c, emsa_zero4());
    } else {
      row[0] = g0;
      row[1] = g1;
      row[2] = g2;
      for (int c = 3; c < ld_d; ++c) row[c] = 0.f;
    }
  }
}

// ---- flat HWC outputs ----------------------------------------------------------------------------
// The targets and the augmented map are written as flat float arrays, four consecutive elements per
// thread (one 16-byte store); the four elements belong to at most two pixels.
struct ScaleTable {
  int32_t s[EMSA_TARGETS_MAX_SCALES], hs[EMSA_TARGETS_MAX_SCALES], ws[EMSA_TARGETS_MAX_SCALES];
  float* out[EMSA_TARGETS_MAX_SCALES];
};

__device__ __forceinline__ void store_chunk(float* __restrict__ out, uint32_t e0, uint32_t total,
                                            const float* v) {
  if (e0 + 4u <= total) {
    emsa_st4(out + e0, make_float4(v[0], v[1], v[2], v[3]));
  } else {
    for (uint32_t j = 0; e0 + j < total; ++j) out[e0 + j] = v[j];
  }
}

// grid (chunks of the scale with the most, scale).  COPY: the source is HWC and 16-byte aligned, so the
// full-resolution scale is a plain copy with 16-byte loads.
template <bool CHW, bool COPY>
__global__ __launch_bounds__(kThreads) void normal_targets_kernel(const float* __restrict__ src, int n,
                                                                  int h, int w, ScaleTable S) {
  const int z = blockIdx.y;
  const int s = S.s[z], hs = S.hs[z], ws = S.ws[z];
  float* __restrict__ out = S.out[z];
  const uint32_t per_img = (uint32_t)hs * ws, total = (uint32_t)n * per_img * 3u;
  const uint32_t chunk = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (chunk >= (total + 3u) / 4u) return;
  const uint32_t e0 = chunk * 4u;
  if (COPY && s == 1 && e0 + 4u <= total) {                  // (same element index on both sides)
    emsa_st4(out + e0, emsa_ld4(src + e0));
    return;
  }
  uint32_t gp = e0 / 3u, c = e0 - gp * 3u;
  const long plane = (long)h * w;
  long base = 0;
  bool fresh = true;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (e0 + j >= total) break;
    if (fresh) {
      const uint32_t img = gp / per_img, r = gp - img * per_img;
      const uint32_t y = r / ws, x = r - y * ws;
      const long pix = (long)(y * s) * w + x * s;            // y * s < h, x * s < w
      base = CHW ? (long)img * 3 * plane + pix : ((long)img * plane + pix) * 3;
      fresh = false;
    }
    v[j] = CHW ? src[base + c * plane] : src[base + c];
    if (++c == 3u) {
      c = 0u;
      ++gp;
      fresh = true;
    }
  }
  store_chunk(out, e0, total, v);
}

__device__ __forceinline__ int nearest_axis(int X, int n_in, int n_out) {    // as csrc/augment.hip
  return min((int)((uint32_t)(X * n_in) / (uint32_t)n_out), n_in - 1);
}

// grid (chunks); out [n][h][w][3].  Every source index is clamped to its frame, whatever the table holds.
template <bool CHW>
__global__ __launch_bounds__(kThreads) void augment_normal_kernel(
    const float* __restrict__ src, const int32_t* __restrict__ params, int n, int hs, int ws, int h, int w,
    float* __restrict__ out) {
  const uint32_t per_img = (uint32_t)h * w, total = (uint32_t)n * per_img * 3u;
  const uint32_t chunk = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (chunk >= (total + 3u) / 4u) return;
  const uint32_t e0 = chunk * 4u;
  uint32_t gp = e0 / 3u, c = e0 - gp * 3u;
  const long plane = (long)hs * ws;
  long base = 0;
  bool fresh = true, flip = false;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (e0 + j >= total) break;
    if (fresh) {
      const uint32_t img = gp / per_img, r = gp - img * per_img;
      const int y = (int)(r / (uint32_t)w), x = (int)(r - (uint32_t)y * w);
      const int32_t* row = params + (long)img * 8;
      const int hr = min(max(row[0], 1), kMaxResized), wr = min(max(row[1], 1), kMaxResized);
      flip = row[4] != 0;
      const int X = min(max(row[3] + (flip ? w - 1 - x : x), 0), kMaxResized - 1);
      const int Y = min(max(row[2] + y, 0), kMaxResized - 1);
      const long pix = (long)nearest_axis(Y, hs, hr) * ws + nearest_axis(X, ws, wr);
      base = CHW ? (long)img * 3 * plane + pix : ((long)img * plane + pix) * 3;
      fresh = false;
    }
    const float a = CHW ? src[base + c * plane] : src[base + c];
    v[j] = (flip && c == 0u) ? -a : a;
    if (++c == 3u) {
      c = 0u;
      ++gp;
      fresh = true;
    }
  }
  store_chunk(out, e0, total, v);
}

// ---- unit vectors --------------------------------------------------------------------------------
// One thread per pixel; the block's 3 * 256 results leave through LDS as 16-byte stores.
#pragma clang fp contract(off)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void normal_unit_kernel(const float* __restrict__ x, int ld,
                                                               uint32_t pixels, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tile[kThreads * 3];
  const uint32_t p0 = blockIdx.x * (uint32_t)kThreads, p = p0 + threadIdx.x;
  if (p < pixels) {
    float a, b, c;
    load_pred<VEC>(x, ld, (long)p, a, b, c);
    const float d = fmaxf(sqrtf(a * a + b * b + c * c), 1e-12f);
    tile[threadIdx.x * 3] = a / d;
    tile[threadIdx.x * 3 + 1] = b / d;
    tile[threadIdx.x * 3 + 2] = c / d;
  }
  __syncthreads();
  const uint32_t left = pixels - p0;                       // p0 < pixels: the grid is exact
  float* dst = out + (long)p0 * 3;
  if (left >= (uint32_t)kThreads) {
    if (threadIdx.x < kThreads * 3 / 4) emsa_st4(dst + threadIdx.x * 4, emsa_ld4(tile + threadIdx.x * 4));
  } else {
    for (uint32_t k = threadIdx.x; k < left * 3u; k += kThreads) dst[k] = tile[k];
  }
}

// ---- angular error -------------------------------------------------------------------------------
// acc[0] += sum of round(angle * 2^20), acc[1] += compared pixels; *flag |= 1 for a non-finite angle
// (such a pixel is not compared).  pred [n][h][w] rows of ld floats, target n x H x W.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void normal_angular_error_kernel(
    const float* __restrict__ pred, int ld, int h, int w, const float* __restrict__ target, int chw, int H,
    int W, uint32_t pixels, unsigned long long* __restrict__ acc, int32_t* __restrict__ flag) {
  __shared__ unsigned long long red_s[kThreads / EMSA_WAVE];
  __shared__ uint32_t red_n[kThreads / EMSA_WAVE];
  const uint32_t HW = (uint32_t)H * W;
  const bool same = h == H && w == W;
  unsigned long long s = 0ull;
  uint32_t cnt = 0u;
  bool bad = false;
  for (long q = blockIdx.x * (long)kThreads + threadIdx.x; q < (long)pixels; q += (long)gridDim.x * kThreads) {
    float t0, t1, t2;
    load_gt(target, HW, chw, (uint32_t)q, t0, t1, t2);
    if (t0 == 0.f && t1 == 0.f && t2 == 0.f) continue;
    long pp = q;
    if (!same) {
      const uint32_t img = (uint32_t)q / HW, r = (uint32_t)q - img * HW;
      const int y = (int)(r / (uint32_t)W), x = (int)(r - (uint32_t)y * W);
      pp = ((long)img * h + emsa_nearest_src(y, h, H)) * w + emsa_nearest_src(x, w, W);
    }
    float p0, p1, p2;
    load_pred<VEC>(pred, ld, pp, p0, p1, p2);
    const float cx = p1 * t2 - p2 * t1, cy = p2 * t0 - p0 * t2, cz = p0 * t1 - p1 * t0;
    const float dot = p0 * t0 + p1 * t1 + p2 * t2;
    const float angle = atan2f(sqrtf(cx * cx + cy * cy + cz * cz), dot);       // in [0, pi]
    if (angle >= 0.f && angle <= 4.f) {
      s += (unsigned long long)llrintf(angle * kAngleOne);
      cnt += 1u;
    } else {
      bad = true;
    }
  }
#pragma unroll
  for (int o = EMSA_WAVE / 2; o > 0; o >>= 1) {
    s += __shfl_down(s, o);
    cnt += __shfl_down(cnt, o);
  }
  if ((threadIdx.x & (EMSA_WAVE - 1)) == 0) {
    red_s[threadIdx.x / EMSA_WAVE] = s;
    red_n[threadIdx.x / EMSA_WAVE] = cnt;
  }
  if (bad) atomicOr(flag, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0ull;
    uint32_t b = 0u;
#pragma unroll
    for (int k = 0; k < kThreads / EMSA_WAVE; ++k) {
      a += red_s[k];
      b += red_n[k];
    }
    if (b) {
      atomicAdd(acc, a);
      atomicAdd(acc + 1, (unsigned long long)b);
    }
  }
}
#pragma clang fp contract(fast)

// host: the pixel count of n maps of h x w, or 0 if the sizes are out of range
long checked_pixels(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || h < 1 || w < 1 || h > kMaxDim || w > kMaxDim) return 0;
  const long pixels = (long)n * h * w;
  return pixels * 3 > kMaxElements ? 0 : pixels;
}

int check_l1(const float* pred, int32_t ld, const float* target, int64_t hw, int64_t pixels) {
  if (!pred || !target) return EMSA_E_ARG;
  if (ld < 3 || hw < 1 || pixels < 1 || pixels * 3 > kMaxElements || pixels % hw) return EMSA_E_SHAPE;
  return EMSA_OK;
}

}  // namespace

extern "C" {

int emsa_normal_l1_blocks(int64_t pixels) { return grid_for((long)pixels); }

int emsa_normal_l1_fwd(const float* pred, int32_t ld, const float* target, int32_t target_chw, int64_t hw,
                       int64_t pixels, float* partial, float* out, void* stream) {
  const int rc = check_l1(pred, ld, target, hw, pixels);
  if (rc != EMSA_OK) return rc;
  if (!partial || !out) return EMSA_E_ARG;
  const int grid = grid_for((long)pixels);
  hipStream_t st = (hipStream_t)stream;
  if (ld % 4 == 0 && aligned16(pred))
    hipLaunchKernelGGL(normal_l1_fwd_kernel<true>, dim3(grid), dim3(kThreads), 0, st, pred, ld, target,
                       (uint32_t)hw, target_chw ? 1 : 0, (uint32_t)pixels, partial);
  else
    hipLaunchKernelGGL(normal_l1_fwd_kernel<false>, dim3(grid), dim3(kThreads), 0, st, pred, ld, target,
                       (uint32_t)hw, target_chw ? 1 : 0, (uint32_t)pixels, partial);
  hipLaunchKernelGGL(normal_l1_finalize_kernel, dim3(1), dim3(kThreads), 0, st, partial, grid, out);
  return emsa_launch_status();
}

int emsa_normal_l1_bwd(const float* pred, int32_t ld, const float* target, int32_t target_chw, int64_t hw,
                       int64_t pixels, const float* sums, const float* grad_out, float* d_pred,
                       int32_t ld_d, void* stream) {
  const int rc = check_l1(pred, ld, target, hw, pixels);
  if (rc != EMSA_OK) return rc;
  if (!sums || !grad_out || !d_pred) return EMSA_E_ARG;
  if (ld_d < 3) return EMSA_E_SHAPE;
  const int grid = grid_for((long)pixels), chw = target_chw ? 1 : 0;
  const bool vec = ld % 4 == 0 && aligned16(pred), vec_d = ld_d % 4 == 0 && aligned16(d_pred);
  hipStream_t st = (hipStream_t)stream;
#define EMSA_NORMAL_BWD(V, VD)                                                                          \
  hipLaunchKernelGGL((normal_l1_bwd_kernel<V, VD>), dim3(grid), dim3(kThreads), 0, st, pred, ld, target, \
                     (uint32_t)hw, chw, (uint32_t)pixels, sums, grad_out, d_pred, ld_d)
  if (vec && vec_d) EMSA_NORMAL_BWD(true, true);
  else if (vec) EMSA_NORMAL_BWD(true, false);
  else if (vec_d) EMSA_NORMAL_BWD(false, true);
  else EMSA_NORMAL_BWD(false, false);
#undef EMSA_NORMAL_BWD
  return emsa_launch_status();
}

int emsa_normal_targets(const float* normal, int32_t chw, int32_t n, int32_t h, int32_t w,
                        const EmsaNormalScale* scales, int32_t n_scales, void* stream) {
  if (!normal || !scales) return EMSA_E_ARG;
  if (!checked_pixels(n, h, w) || n_scales < 1 || n_scales > EMSA_TARGETS_MAX_SCALES) return EMSA_E_SHAPE;
  ScaleTable S = {};
  long chunks = 0;
  for (int z = 0; z < n_scales; ++z) {
    const EmsaNormalScale& e = scales[z];
    if (e.scale < 1 || h % e.scale || w % e.scale) return EMSA_E_SHAPE;
    if (!e.out || !aligned16(e.out)) return EMSA_E_ARG;
    S.s[z] = e.scale;
    S.hs[z] = h / e.scale;
    S.ws[z] = w / e.scale;
    S.out[z] = e.out;
    const long c = ((long)n * S.hs[z] * S.ws[z] * 3 + 3) / 4;
    chunks = c > chunks ? c : chunks;
  }
  const dim3 grid((unsigned)((chunks + kThreads - 1) / kThreads), n_scales);
  hipStream_t st = (hipStream_t)stream;
  if (chw)
    hipLaunchKernelGGL((normal_targets_kernel<true, false>), grid, dim3(kThreads), 0, st, normal, n, h, w, S);
  else if (aligned16(normal))
    hipLaunchKernelGGL((normal_targets_kernel<false, true>), grid, dim3(kThreads), 0, st, normal, n, h, w, S);
  else
    hipLaunchKernelGGL((normal_targets_kernel<false, false>), grid, dim3(kThreads), 0, st, normal, n, h, w, S);
  return emsa_launch_status();
}

int emsa_augment_normal(const float* normal, int32_t chw, const int32_t* params, int32_t n, int32_t hs,
                        int32_t ws, int32_t h, int32_t w, float* out, void* stream) {
  if (!normal || !params || !out || !aligned16(out)) return EMSA_E_ARG;
  if (n < 1 || hs < 1 || ws < 1 || h < 1 || w < 1 || hs > kMaxSide || ws > kMaxSide || h > kMaxSide ||
      w > kMaxSide || !checked_pixels(n, h, w) || !checked_pixels(n, hs, ws))
    return EMSA_E_SHAPE;
  const long chunks = ((long)n * h * w * 3 + 3) / 4;
  const dim3 grid((unsigned)((chunks + kThreads - 1) / kThreads));
  hipStream_t st = (hipStream_t)stream;
  if (chw)
    hipLaunchKernelGGL(augment_normal_kernel<true>, grid, dim3(kThreads), 0, st, normal, params, n, hs, ws,
                       h, w, out);
  else
    hipLaunchKernelGGL(augment_normal_kernel<false>, grid, dim3(kThreads), 0, st, normal, params, n, hs, ws,
                       h, w, out);
  return emsa_launch_status();
}

int emsa_normal_unit(const float* pred, int32_t ld, int64_t pixels, float* out, void* stream) {
  if (!pred || !out || !aligned16(out)) return EMSA_E_ARG;
  if (ld < 3 || pixels < 1 || pixels * 3 > kMaxElements) return EMSA_E_SHAPE;
  const dim3 grid((unsigned)((pixels + kThreads - 1) / kThreads));
  hipStream_t st = (hipStream_t)stream;
  if (ld % 4 == 0 && aligned16(pred))
    hipLaunchKernelGGL(normal_unit_kernel<true>, grid, dim3(kThreads), 0, st, pred, ld, (uint32_t)pixels, out);
  else
    hipLaunchKernelGGL(normal_unit_kernel<false>, grid, dim3(kThreads), 0, st, pred, ld, (uint32_t)pixels, out);
  return emsa_launch_status();
}

int emsa_normal_angular_error(const float* pred, int32_t ld, int32_t n, int32_t h, int32_t w,
                              const float* target, int32_t target_chw, int32_t th, int32_t tw,
                              int64_t* acc, int32_t* flag, void* stream) {
  if (!pred || !target || !acc || !flag) return EMSA_E_ARG;
  const long pixels = checked_pixels(n, th, tw);
  if (ld < 3 || !pixels || !checked_pixels(n, h, w)) return EMSA_E_SHAPE;
  const int grid = grid_for(pixels), chw = target_chw ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (ld % 4 == 0 && aligned16(pred))
    hipLaunchKernelGGL(normal_angular_error_kernel<true>, dim3(grid), dim3(kThreads), 0, st, pred, ld, h, w,
                       target, chw, th, tw, (uint32_t)pixels, (unsigned long long*)acc, flag);
  else
    hipLaunchKernelGGL(normal_angular_error_kernel<false>, dim3(grid), dim3(kThreads), 0, st, pred, ld, h, w,
                       target, chw, th, tw, (uint32_t)pixels, (unsigned long long*)acc, flag);
  return emsa_launch_status();
}

}  // extern "C"

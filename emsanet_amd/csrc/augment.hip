// Training augmentation on device: the reference's RandomResize -> RandomCrop -> RandomHSVJitter ->
// RandomHorizontalFlip (/root/reference/emsanet/preprocessing.py:106-123) fused with NormalizeRGB /
// NormalizeDepth + HWC->CHW, from the raw uint8 / uint16 frames and the integer label maps of a batch.
// The rules are stated in emsanet_amd/augment.py.  Three kernels:
//   params        the per-sample row (Hr, Wr, cy, cx, flip, dh, ds, dv) from a counter-based hash of
//                 (seed, step, sample, draw); the step lives on the device and is advanced by the
//                 kernel, so a replayed graph draws fresh parameters
//   apply         every output pixel of every map of the batch in one launch: integer bilinear for RGB,
//                 nearest for depth and labels, HSV jitter and normalisation in fp32
//   orientations  theta -> (2 pi - theta) mod 2 pi for the flipped samples
// The resized frame is never materialised; resize, crop and flip are one composed index.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLanesX = 32;                        // threads along x; each produces 4 consecutive pixels
constexpr int kTileW = kLanesX * 4;                // 128
constexpr int kRowsPerThread = 4;
constexpr int kTileH = (kThreads / kLanesX) * kRowsPerThread;   // 32
constexpr int kMaxSide = 4096;                     // source and crop sides: the integer products below
constexpr int kMaxResized = 16384;                 // stay under 2^31 ((2 X + 1) n_in <= 2^15 * 2^12)

__device__ __forceinline__ uint32_t augment_hash(uint32_t seed, uint32_t step, uint32_t sample,
                                                 uint32_t draw) {
  uint32_t h = emsa_lowbias32(seed + 0x9E3779B9u);
  h = emsa_lowbias32(h + step);
  h = emsa_lowbias32(h + sample);
  return emsa_lowbias32(h + draw);
}

__device__ __forceinline__ uint32_t uniform_below(uint32_t hash, uint32_t n) {
  return (uint32_t)(((unsigned long long)hash * n) >> 32);
}

// one workgroup; state = {seed, step} as uint32
__global__ __launch_bounds__(kThreads) void augment_params_kernel(
    uint32_t* __restrict__ state, int32_t* __restrict__ table, int n, int hs, int ws, int h, int w,
    int q_min, int q_max, unsigned long long flip_threshold, float amp_h, float amp_s, float amp_v) {
  const uint32_t seed = state[0], step = state[1];
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int q = q_min + (int)uniform_below(augment_hash(seed, step, i, 0), (uint32_t)(q_max - q_min + 1));
    const int hr = (hs * q + 512) >> 10, wr = (ws * q + 512) >> 10;
    const int cy = (int)uniform_below(augment_hash(seed, step, i, 1), (uint32_t)(hr - h + 1));
    const int cx = (int)uniform_below(augment_hash(seed, step, i, 2), (uint32_t)(wr - w + 1));
    const int flip = (unsigned long long)augment_hash(seed, step, i, 3) < flip_threshold ? 1 : 0;
    int32_t* row = table + (long)i * 8;
    row[0] = hr;
    row[1] = wr;
    row[2] = cy;
    row[3] = cx;
    row[4] = flip;
    const float amp[3] = {amp_h, amp_s, amp_v};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t u = augment_hash(seed, step, i, 4 + k) >> 8;               // 24 bits
      const float d = (float)((int)(2u * u) - (1 << 24)) * amp[k];              // amp = amplitude / 2^24
      row[5 + k] = __float_as_int(d);
    }
  }
  __syncthreads();                       // every thread has read the step
  if (threadIdx.x == 0) state[1] = step + 1u;
}

// one axis of the bilinear resize with half-pixel centres, in integers: the two clamped source
// indices and the weight a in [0, 2048] of the second
__device__ __forceinline__ void bilinear_axis(int X, int n_in, int n_out, int* i0, int* i1, int* a) {
  const int t = (2 * X + 1) * n_in - n_out, d = 2 * n_out;
  int q, r;
  if (t < 0) {                           // (t > -d: up-scaling, first half pixel)
    q = -1;
    r = t + d;
  } else {
    q = (int)((uint32_t)t / (uint32_t)d);
    r = t - q * d;
  }
  *a = (int)((uint32_t)(r * 2048 + n_out) / (uint32_t)d);
  *i0 = min(max(q, 0), n_in - 1);
  *i1 = min(max(q + 1, 0), n_in - 1);
}

__device__ __forceinline__ int nearest_axis(int X, int n_in, int n_out) {
  return min((int)((uint32_t)(X * n_in) / (uint32_t)n_out), n_in - 1);
}

struct ApplyArgs {
  const uint8_t* rgb;          // [n][hs][ws][3] or null
  const uint16_t* depth;       // [n][hs][ws] or null
  const uint8_t* label[2];     // [n][hs][ws] elements of label_size bytes, or null
  float* out_rgb;              // [n][3][h][w]
  float* out_depth;            // [n][1][h][w]
  uint8_t* out_label[2];       // [n][h][w]
  const int32_t* params;       // [n][8]
  int32_t label_size[2];
  int32_t n, hs, ws, h, w;
  float scale, m0, m1, m2, i0, i1, i2;       // RGB: (v * scale - m) * i
  float depth_mean, depth_inv_std;
  int32_t keep_zero;
};

#pragma clang fp contract(off)
// hue in [0, 6), saturation, value of r, g, b in [0, 1]; then the jitter; then back
__device__ __forceinline__ void hsv_jitter(float& r, float& g, float& b, float dh, float ds, float dv) {
  const float v = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b)), c = v - mn;
  const float s = v > 0.f ? c / v : 0.f;
  float hue = 0.f;
  if (c > 0.f) {
    if (v == r) {
      hue = (g - b) / c;
      if (hue < 0.f) hue += 6.f;
    } else if (v == g) {
      hue = (b - r) / c + 2.f;
    } else {
      hue = (r - g) / c + 4.f;
    }
  }
  hue = hue + 6.f * dh;
  hue = hue - 6.f * floorf(hue / 6.f);
  const float s2 = fminf(fmaxf(s + ds, 0.f), 1.f), v2 = fminf(fmaxf(v + dv, 0.f), 1.f);
  const float vs = v2 * s2;
  float out[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float k = (float)(5 - 2 * ch) + hue;                      // n = 5, 3, 1 for r, g, b
    k = k - 6.f * floorf(k / 6.f);
    const float m = fminf(fmaxf(fminf(k, 4.f - k), 0.f), 1.f);
    out[ch] = v2 - vs * m;
  }
  r = out[0];
  g = out[1];
  b = out[2];
}

// the expressions of normalize_rgb_kernel / normalize_depth_kernel (csrc/postproc.hip).  That file is
// compiled with the default contraction, which fuses `v * scale - m` into one fma; the fma is written
// out here so that the same bits come out whatever surrounds the expression.
__device__ __forceinline__ float norm_u8(float v, float scale, float m, float i) {
  return __builtin_fmaf(v, scale, -m) * i;
}
__device__ __forceinline__ float norm_unit(float v, float m, float i) { return (v - m) * i; }
__device__ __forceinline__ float norm_depth(uint16_t raw, float mean, float inv_std, int keep_zero) {
  const float v = (float)raw;
  return (keep_zero && raw == 0) ? 0.f : (v - mean) * inv_std;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, const float* v, int count) {
  if (VEC && count == 4) {
    emsa_st4(p, make_float4(v[0], v[1], v[2], v[3]));
  } else {
    for (int j = 0; j < count; ++j) p[j] = v[j];
  }
}

// four labels of `size` bytes gathered from `row` at xn[0..3] and stored at dst (element index)
template <bool VEC>
__device__ __forceinline__ void copy_labels(const uint8_t* __restrict__ row, uint8_t* __restrict__ dst,
                                            int size, const int* xn, int count) {
  switch (size) {
    case 1: {
      uint8_t v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = row[xn[j]];
      if (VEC && count == 4) {
        *reinterpret_cast<uint32_t*>(dst) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) |
                                            ((uint32_t)v[3] << 24);
      } else {
        for (int j = 0; j < count; ++j) dst[j] = v[j];
      }
    } break;
    case 2: {
      const uint16_t* s = (const uint16_t*)row;
      uint16_t* d = (uint16_t*)dst;
      uint16_t v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = s[xn[j]];
      if (VEC && count == 4) {
        *reinterpret_cast<uint2*>(d) = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16),
                                                  (uint32_t)v[2] | ((uint32_t)v[3] << 16));
      } else {
        for (int j = 0; j < count; ++j) d[j] = v[j];
      }
    } break;
    case 4: {
      const uint32_t* s = (const uint32_t*)row;
      uint32_t* d = (uint32_t*)dst;
      uint32_t v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = s[xn[j]];
      if (VEC && count == 4) {
        *reinterpret_cast<uint4*>(d) = make_uint4(v[0], v[1], v[2], v[3]);
      } else {
        for (int j = 0; j < count; ++j) d[j] = v[j];
      }
    } break;
    default: {
      const unsigned long long* s = (const unsigned long long*)row;
      unsigned long long* d = (unsigned long long*)dst;
      unsigned long long v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = s[xn[j]];
      if (VEC && count == 4) {
        *reinterpret_cast<ulonglong2*>(d) = make_ulonglong2(v[0], v[1]);
        *reinterpret_cast<ulonglong2*>(d + 2) = make_ulonglong2(v[2], v[3]);
      } else {
        for (int j = 0; j < count; ++j) d[j] = v[j];
      }
    } break;
  }
}

// grid (x tiles, y tiles, image).  HSV: the jitter stage is compiled in; VEC: w % 4 == 0, so the four
// pixels of a thread are one aligned 16-byte store per fp32 plane (a packed store per label map).
// Every source index is clamped to its frame, whatever the table holds.
template <bool HSV, bool VEC>
__global__ __launch_bounds__(kThreads) void augment_apply_kernel(ApplyArgs A) {
  const int img = blockIdx.z;
  const int x = blockIdx.x * kTileW + (threadIdx.x % kLanesX) * 4;
  const int ty = blockIdx.y * kTileH + threadIdx.x / kLanesX;
  if (x >= A.w) return;
  const int count = min(4, A.w - x);
  const int32_t* row = A.params + (long)img * 8;
  const int hr = min(max(row[0], 1), kMaxResized), wr = min(max(row[1], 1), kMaxResized);
  const int cy = row[2], cx = row[3], flip = row[4];
  const float dh = __int_as_float(row[5]), ds = __int_as_float(row[6]), dv = __int_as_float(row[7]);

  // per thread, once for all of its rows: the x side of the four pixels
  int x0[4], x1[4], ax[4], xn[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int xo = min(x + j, A.w - 1);
    const int X = min(max(cx + (flip ? A.w - 1 - xo : xo), 0), kMaxResized - 1);
    bilinear_axis(X, A.ws, wr, &x0[j], &x1[j], &ax[j]);
    xn[j] = nearest_axis(X, A.ws, wr);
    x0[j] *= 3;
    x1[j] *= 3;
  }
  const long src_img = (long)img * A.hs, hw = (long)A.h * A.w;
#pragma unroll 1
  for (int k = 0; k < kRowsPerThread; ++k) {
    const int y = ty + k * (kThreads / kLanesX);
    if (y >= A.h) return;
    const int Y = min(max(cy + y, 0), kMaxResized - 1);
    const long pix = ((long)img * A.h + y) * A.w + x;         // in an [n][h][w] map
    const int yn = nearest_axis(Y, A.hs, hr);
    if (A.rgb) {
      int y0, y1, ay;
      bilinear_axis(Y, A.hs, hr, &y0, &y1, &ay);
      const uint8_t* __restrict__ p0 = A.rgb + (src_img + y0) * A.ws * 3;
      const uint8_t* __restrict__ p1 = A.rgb + (src_img + y1) * A.ws * 3;
      float o[3][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int wx1 = ax[j], wx0 = 2048 - wx1;
        float c[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int top = wx0 * p0[x0[j] + ch] + wx1 * p0[x1[j] + ch];
          const int bot = wx0 * p1[x0[j] + ch] + wx1 * p1[x1[j] + ch];
          c[ch] = (float)(((2048 - ay) * top + ay * bot + (1 << 21)) >> 22);     // the resized uint8
        }
        if (HSV) {
          float r = c[0] / 255.f, g = c[1] / 255.f, b = c[2] / 255.f;
          hsv_jitter(r, g, b, dh, ds, dv);
          o[0][j] = norm_unit(r, A.m0, A.i0);
          o[1][j] = norm_unit(g, A.m1, A.i1);
          o[2][j] = norm_unit(b, A.m2, A.i2);
        } else {
          o[0][j] = norm_u8(c[0], A.scale, A.m0, A.i0);
          o[1][j] = norm_u8(c[1], A.scale, A.m1, A.i1);
          o[2][j] = norm_u8(c[2], A.scale, A.m2, A.i2);
        }
      }
      float* dst = A.out_rgb + (long)img * 3 * hw + (long)y * A.w + x;
      store4<VEC>(dst, o[0], count);
      store4<VEC>(dst + hw, o[1], count);
      store4<VEC>(dst + 2 * hw, o[2], count);
    }
    if (A.depth) {
      const uint16_t* __restrict__ p = A.depth + (src_img + yn) * A.ws;
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = norm_depth(p[xn[j]], A.depth_mean, A.depth_inv_std, A.keep_zero);
      store4<VEC>(A.out_depth + pix, o, count);
    }
#pragma unroll
    for (int l = 0; l < 2; ++l)
      if (A.label[l]) {
        const int size = A.label_size[l];
        copy_labels<VEC>(A.label[l] + (src_img + yn) * A.ws * size, A.out_label[l] + pix * size, size, xn,
                         count);
      }
  }
}

__global__ void augment_orientations_kernel(const float* __restrict__ in, float* __restrict__ out,
                                            const int32_t* __restrict__ params, int n, int m) {
  const float two_pi = 6.2831855f;       // 2 pi rounded to fp32
  const long total = (long)n * m;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    float a = in[i];
    if (params[(i / m) * 8 + 4]) {
      a = two_pi - a;
      a = a - two_pi * floorf(a / two_pi);
      if (a < 0.f) a = a + two_pi;
      if (a >= two_pi) a = a - two_pi;
    }
    out[i] = a;
  }
}
#pragma clang fp contract(fast)

int label_size(int dt) {
  switch (dt) {
    case EMSA_LABEL_I64: return 8;
    case EMSA_LABEL_I32: return 4;
    case EMSA_LABEL_U8: return 1;
    case EMSA_LABEL_I16:
    case EMSA_LABEL_U16: return 2;
    default: return 0;
  }
}

bool sizes_ok(int n, int hs, int ws, int h, int w) {
  return n >= 1 && hs >= 1 && ws >= 1 && h >= 1 && w >= 1 && hs <= kMaxSide && ws <= kMaxSide &&
         h <= kMaxSide && w <= kMaxSide;
}

}  // namespace

extern "C" {

int emsa_augment_params(int32_t* state, int32_t* table, int32_t n, int32_t hs, int32_t ws, int32_t h,
                        int32_t w, int32_t q_min, int32_t q_max, int64_t flip_threshold,
                        float hue_amplitude, float saturation_amplitude, float value_amplitude,
                        void* stream) {
  if (!state || !table) return EMSA_E_ARG;
  if (!sizes_ok(n, hs, ws, h, w) || q_min < 1 || q_max < q_min) return EMSA_E_SHAPE;
  // the crop fits the smallest resize; the largest stays inside the integer range of the apply kernel
  if ((((int64_t)hs * q_min + 512) >> 10) < h || (((int64_t)ws * q_min + 512) >> 10) < w ||
      (((int64_t)hs * q_max + 512) >> 10) > kMaxResized || (((int64_t)ws * q_max + 512) >> 10) > kMaxResized)
    return EMSA_E_SHAPE;
  if (flip_threshold < 0 || flip_threshold > ((int64_t)1 << 32)) return EMSA_E_ARG;
  const float k = 1.f / 16777216.f;
  hipLaunchKernelGGL(augment_params_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream,
                     (uint32_t*)state, table, n, hs, ws, h, w, q_min, q_max,
                     (unsigned long long)flip_threshold, hue_amplitude * k, saturation_amplitude * k,
                     value_amplitude * k);
  return emsa_launch_status();
}

int emsa_augment_apply(const uint8_t* rgb, const uint16_t* depth, const void* label0,
                       int32_t label0_dtype, const void* label1, int32_t label1_dtype,
                       const int32_t* params, int32_t n, int32_t hs, int32_t ws, int32_t h, int32_t w,
                       float* out_rgb, float* out_depth, void* out_label0, void* out_label1,
                       float rgb_scale, const float* mean3, const float* std3, float depth_mean,
                       float depth_std, int32_t keep_zero, int32_t hsv, void* stream) {
  if (!params || (!rgb && !depth && !label0 && !label1)) return EMSA_E_ARG;
  if ((rgb != nullptr) != (out_rgb != nullptr) || (depth != nullptr) != (out_depth != nullptr) ||
      (label0 != nullptr) != (out_label0 != nullptr) || (label1 != nullptr) != (out_label1 != nullptr))
    return EMSA_E_ARG;
  if (rgb && (!mean3 || !std3)) return EMSA_E_ARG;
  if (!sizes_ok(n, hs, ws, h, w) || n > 65535) return EMSA_E_SHAPE;
  if (rgb && (std3[0] == 0.f || std3[1] == 0.f || std3[2] == 0.f)) return EMSA_E_SHAPE;
  if (depth && depth_std == 0.f) return EMSA_E_SHAPE;
  ApplyArgs A = {};
  A.rgb = rgb;
  A.depth = depth;
  A.label[0] = (const uint8_t*)label0;
  A.label[1] = (const uint8_t*)label1;
  A.out_rgb = out_rgb;
  A.out_depth = out_depth;
  A.out_label[0] = (uint8_t*)out_label0;
  A.out_label[1] = (uint8_t*)out_label1;
  A.label_size[0] = label0 ? label_size(label0_dtype) : 0;
  A.label_size[1] = label1 ? label_size(label1_dtype) : 0;
  if ((label0 && !A.label_size[0]) || (label1 && !A.label_size[1])) return EMSA_E_ARG;
  // the packed stores need 16-byte aligned planes (w % 4 == 0 keeps every row aligned)
  const uintptr_t align = (uintptr_t)out_rgb | (uintptr_t)out_depth | (uintptr_t)out_label0 |
                          (uintptr_t)out_label1;
  const bool vec = w % 4 == 0 && align % 16 == 0;
  A.params = params;
  A.n = n;
  A.hs = hs;
  A.ws = ws;
  A.h = h;
  A.w = w;
  if (rgb) {
    A.scale = rgb_scale;
    A.m0 = mean3[0];
    A.m1 = mean3[1];
    A.m2 = mean3[2];
    A.i0 = 1.f / std3[0];
    A.i1 = 1.f / std3[1];
    A.i2 = 1.f / std3[2];
  }
  A.depth_mean = depth_mean;
  A.depth_inv_std = depth ? 1.f / depth_std : 0.f;
  A.keep_zero = keep_zero ? 1 : 0;
  const dim3 grid((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH, n), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (hsv && rgb) {
    if (vec) hipLaunchKernelGGL((augment_apply_kernel<true, true>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((augment_apply_kernel<true, false>), grid, block, 0, st, A);
  } else {
    if (vec) hipLaunchKernelGGL((augment_apply_kernel<false, true>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((augment_apply_kernel<false, false>), grid, block, 0, st, A);
  }
  return emsa_launch_status();
}

int emsa_augment_orientations(const float* orientations, float* out, const int32_t* params, int32_t n,
                              int32_t max_instances, void* stream) {
  if (!orientations || !out || !params) return EMSA_E_ARG;
  if (n < 1 || max_instances < 1) return EMSA_E_SHAPE;
  const long total = (long)n * max_instances;
  long blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(augment_orientations_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                     orientations, out, params, n, max_instances);
  return emsa_launch_status();
}

}  // extern "C"

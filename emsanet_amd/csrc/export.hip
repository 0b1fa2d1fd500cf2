// Inference output packing on device: the ScanNet benchmark and "mapping" formats of the dataset
// inference run (/root/reference/inference_dataset.py:139-552) formed from the post-processed
// prediction where it lies, in HBM, so that only the packed bytes cross to the host.
//  * emsa_export_pack            a table of per-pixel jobs (grid.y = job): label -> uint8 through a
//                                class table, panoptic BGR, sem * 1000 + inst as uint16, class + score
//  * emsa_export_instance_ranks  rank of every instance id that owns pixels, per sample
//  * emsa_export_instance_masks  one 0 / 255 mask plane per ranked instance
// Pure bandwidth: a thread owns 4 consecutive pixels of the flat (n, H, W) output and writes them with
// one 4- / 8- / 12- / 16-byte store; sources of another size are gathered by the nearest rule of
// emsa_nearest_fwd_t.  Rules per entry point: include/emsanet_hip.h.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;          // ~8 workgroups per CU, grid-stride beyond

// the job as the kernel sees it (EmsaExportJob with the host-side decisions taken)
struct PackJob {
  const void* src0;
  const void* src1;
  const void* depth;
  const uint8_t* lut;
  void* dst;
  long divisor;
  float depth_max_f32;        // fp32 depth: masked where depth > depth_max_f32
  int depth_max_u16;          // uint16 depth: masked where depth > depth_max_u16 (= floor(max_depth))
  int kind, src0_dtype, src1_dtype, depth_dtype;
  int lut_size, add;
  int h, w;
  int vec;                    // source has the output's size and 4-element alignment: vector loads
};
struct PackTable {
  PackJob j[EMSA_EXPORT_MAX_JOBS];
};

template <typename T>
__device__ __forceinline__ void load4_as(const void* p, const int idx[4], bool vec, long v[4]) {
  const T* q = (const T*)p;
  if (vec) {
    typedef T V __attribute__((ext_vector_type(4)));
    const V t = *reinterpret_cast<const V*>(q + idx[0]);
    v[0] = (long)t.x; v[1] = (long)t.y; v[2] = (long)t.z; v[3] = (long)t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = idx[k] >= 0 ? (long)q[idx[k]] : 0;
  }
}
__device__ __forceinline__ void load4_label(const void* p, int dtype, const int idx[4], bool vec, long v[4]) {
  switch (dtype) {
    case EMSA_LABEL_I64: load4_as<int64_t>(p, idx, vec, v); break;
    case EMSA_LABEL_I32: load4_as<int32_t>(p, idx, vec, v); break;
    case EMSA_LABEL_U8: load4_as<uint8_t>(p, idx, vec, v); break;
    default: load4_as<uint16_t>(p, idx, vec, v); break;            // EMSA_LABEL_U16 (raw depth)
  }
}
__device__ __forceinline__ void load4_f32(const void* p, const int idx[4], bool vec, float v[4]) {
  const float* q = (const float*)p;
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(q + idx[0]);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = idx[k] >= 0 ? q[idx[k]] : 0.f;
  }
}

// class of `v` through the job's table: lut != NULL -> lut[v]; lut == NULL, lut_size > 0 -> identity on
// [0, lut_size); outside either: 0 and one count.  lut_size == 0: no table, no bound.
__device__ __forceinline__ long map_class(const PackJob& j, long v, uint32_t& bad) {
  if (j.lut_size == 0) return v;
  if (v < 0 || v >= j.lut_size) { ++bad; return 0; }
  return j.lut ? (long)j.lut[v] : v;
}

// torch.clamp(score, 0, 0.999): NaN stays NaN
__device__ __forceinline__ float clamp_score(float s) {
  return s < 0.f ? 0.f : (s > 0.999f ? 0.999f : s);
}

// One group = output pixels [4g, 4g + 4) of the flat (n, H, W) map; `valid` of them exist (the last
// group of a map whose size is no multiple of 4 is stored element by element).
__global__ __launch_bounds__(kThreads) void export_pack_kernel(const PackTable tab, int n_px, int H, int W,
                                                               unsigned long long* __restrict__ counters) {
  const PackJob& j = tab.j[blockIdx.y];
  const int groups = (n_px + 3) >> 2;
  const int hw = H * W, shw = j.h * j.w;
  const bool same = j.h == H && j.w == W;
  const bool row4 = (W & 3) == 0;                       // a group never crosses a row
  uint32_t bad[EMSA_EXPORT_CAUSES] = {0u, 0u, 0u, 0u};
  for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
    const int p0 = g << 2;
    const int valid = n_px - p0 < 4 ? n_px - p0 : 4;
    const bool vec = (j.vec & 1) && valid == 4;
    const bool dvec = (j.vec & 2) && valid == 4;        // bit 1: the depth map is aligned for it
    int idx[4], didx[4];                                // source / depth element per pixel, -1 = none
    if (same) {
#pragma unroll
      for (int k = 0; k < 4; ++k) idx[k] = k < valid ? p0 + k : -1;
    } else if (row4) {
      const int img = p0 / hw, r = p0 - img * hw;
      const int y = r / W, x = r - y * W;
      const int base = img * shw + emsa_nearest_src(y, j.h, H) * j.w;
#pragma unroll
      for (int k = 0; k < 4; ++k) idx[k] = base + emsa_nearest_src(x + k, j.w, W);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + k;
        const int img = p / hw, r = p - img * hw;
        const int y = r / W, x = r - y * W;
        idx[k] = k < valid ? img * shw + emsa_nearest_src(y, j.h, H) * j.w + emsa_nearest_src(x, j.w, W) : -1;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) didx[k] = k < valid ? p0 + k : -1;

    long a[4], b[4] = {0, 0, 0, 0};
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    bool far[4] = {false, false, false, false};
    load4_label(j.src0, j.src0_dtype, idx, vec, a);
    if (j.kind == EMSA_EXPORT_CLASS_SCORE_F32) load4_f32(j.src1, idx, vec, s);
    else if (j.src1) load4_label(j.src1, j.src1_dtype, idx, vec, b);
    if (j.depth) {
      if (j.depth_dtype == EMSA_LABEL_U16) {
        long d[4];
        load4_label(j.depth, EMSA_LABEL_U16, didx, dvec, d);
#pragma unroll
        for (int k = 0; k < 4; ++k) far[k] = (int)d[k] > j.depth_max_u16;
      } else {
        float d[4];
        load4_f32(j.depth, didx, dvec, d);
#pragma unroll
        for (int k = 0; k < 4; ++k) far[k] = d[k] > j.depth_max_f32;
      }
    }

    if (j.kind == EMSA_EXPORT_LABEL_U8) {
      uint32_t word = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= valid) break;
        long c = map_class(j, a[k] + j.add, bad[EMSA_EXPORT_CAUSE_LUT]);
        if (j.lut_size == 0 && (c < 0 || c > 255)) { ++bad[EMSA_EXPORT_CAUSE_LUT]; c = 0; }
        if (far[k]) c = 0;
        word |= (uint32_t)(c & 0xFF) << (8 * k);
      }
      uint8_t* o = (uint8_t*)j.dst + p0;
      if (valid == 4) *reinterpret_cast<uint32_t*>(o) = word;
      else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < valid) o[k] = (uint8_t)(word >> (8 * k));
      }
    } else if (j.kind == EMSA_EXPORT_PANOPTIC_BGR) {
      uint8_t px[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        long sem = a[k], inst = b[k];
        if (j.divisor > 0) {
          if (sem < 0) { ++bad[EMSA_EXPORT_CAUSE_LUT]; sem = 0; }
          if (sem <= 0xFFFFFFFFl) {                               // (64-bit division is a long routine)
            const uint32_t u = (uint32_t)sem, d = (uint32_t)j.divisor;
            inst = (long)(u % d);
            sem = (long)(u / d);
          } else {
            inst = sem % j.divisor;
            sem = sem / j.divisor;
          }
        }
        if (k >= valid) { sem = 0; inst = 0; }
        else sem = map_class(j, sem, bad[EMSA_EXPORT_CAUSE_LUT]);
        if (far[k]) { sem = 0; inst = 0; }
        if (sem < 0 || sem > 255) { ++bad[EMSA_EXPORT_CAUSE_CLASS]; }
        if (inst < 0 || inst > 65535) { ++bad[EMSA_EXPORT_CAUSE_INSTANCE]; }
        px[3 * k + 0] = (uint8_t)(inst & 0xFF);
        px[3 * k + 1] = (uint8_t)((inst >> 8) & 0xFF);
        px[3 * k + 2] = (uint8_t)(sem & 0xFF);
      }
      uint8_t* o = (uint8_t*)j.dst + 3l * p0;
      if (valid == 4) {
        uint32_t wd[3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
          wd[q] = (uint32_t)px[4 * q] | (uint32_t)px[4 * q + 1] << 8 | (uint32_t)px[4 * q + 2] << 16 |
                  (uint32_t)px[4 * q + 3] << 24;
        uint32_t* ow = reinterpret_cast<uint32_t*>(o);          // 12 * g bytes: dword aligned
        ow[0] = wd[0]; ow[1] = wd[1]; ow[2] = wd[2];
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k)
          if (k < 3 * valid) o[k] = px[k];
      }
    } else if (j.kind == EMSA_EXPORT_SEM_INST_U16) {
      uint16_t v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        long sem = 0, inst = b[k];
        if (k < valid) sem = map_class(j, a[k] + j.add, bad[EMSA_EXPORT_CAUSE_LUT]);
        if (far[k] || k >= valid) { sem = 0; inst = 0; }
        const long full = sem * 1000 + inst;
        if (full < 0 || full > 65535) ++bad[EMSA_EXPORT_CAUSE_WRAP];
        v[k] = (uint16_t)(full & 0xFFFF);
      }
      uint16_t* o = (uint16_t*)j.dst + p0;
      if (valid == 4)
        *reinterpret_cast<uint2*>(o) = make_uint2((uint32_t)v[0] | (uint32_t)v[1] << 16,
                                                   (uint32_t)v[2] | (uint32_t)v[3] << 16);
      else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < valid) o[k] = v[k];
      }
    } else {                                                     // EMSA_EXPORT_CLASS_SCORE_F32
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        long c = 0;
        if (k < valid) c = map_class(j, a[k] + j.add, bad[EMSA_EXPORT_CAUSE_LUT]);
        v[k] = (float)c + clamp_score(s[k]);                     // ONE fp32 add
      }
      float* o = (float*)j.dst + p0;
      if (valid == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < valid) o[k] = v[k];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < EMSA_EXPORT_CAUSES; ++c)
    if (bad[c]) atomicAdd(counters + c, (unsigned long long)bad[c]);
}

inline int label_bytes(int dtype) {
  switch (dtype) {
    case EMSA_LABEL_I64: return 8;
    case EMSA_LABEL_I32: return 4;
    case EMSA_LABEL_U8: return 1;
    default: return 0;
  }
}
inline bool aligned(const void* p, int bytes) { return ((uintptr_t)p % (uintptr_t)bytes) == 0; }

// ---- instance ranks ----------------------------------------------------------------------------
// one workgroup: thread = sample (strided), a serial walk over its slots; then thread 0 sums the counts
__global__ __launch_bounds__(kThreads) void export_ranks_kernel(
    const int32_t* __restrict__ area, const int32_t* __restrict__ cls, const uint8_t* __restrict__ lut,
    int lut_size, int n, int slots, int32_t* __restrict__ rank, int32_t* __restrict__ by_rank,
    int32_t* __restrict__ class_by_rank, int32_t* __restrict__ count, int32_t* __restrict__ start,
    unsigned long long* __restrict__ counters) {
  uint32_t bad = 0u;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const long row = (long)i * slots;
    int r = 0;
    rank[row] = -1;                                              // id 0: no instance
    for (int id = 1; id < slots; ++id) {
      const bool present = area[row + id] > 0;
      rank[row + id] = present ? r : -1;
      if (present) {
        long c = (long)cls[row + id] + 1;                        // into the label list with void
        if (lut_size > 0) {
          if (c < 0 || c >= lut_size) { ++bad; c = 0; }
          else if (lut) c = (long)lut[c];
        }
        by_rank[row + r] = id;
        class_by_rank[row + r] = (int32_t)c;
        ++r;
      }
    }
    for (int k = r; k < slots; ++k) { by_rank[row + k] = -1; class_by_rank[row + k] = -1; }
    count[i] = r;
  }
  if (bad) atomicAdd(counters + EMSA_EXPORT_CAUSE_LUT, (unsigned long long)bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t s = 0;
    for (int i = 0; i < n; ++i) { start[i] = s; s += count[i]; }
    start[n] = s;
  }
}

// ---- instance masks ----------------------------------------------------------------------------
// grid (blocks, n): a thread owns 4 consecutive pixels of its sample's (H, W) map (VEC: H * W is a
// multiple of 4, every plane starts dword aligned) or one pixel, reads the id(s) once and writes that
// place in every plane of the sample: 255 in the plane of the id's rank, 0 elsewhere.
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void export_masks_kernel(
    const T* __restrict__ inst, int h, int w, int H, int W, const int32_t* __restrict__ rank, int slots,
    const int32_t* __restrict__ count, const int32_t* __restrict__ start, int total,
    uint8_t* __restrict__ stack) {
  const int img = blockIdx.y;
  const int hw = H * W;
  const int first = start[img];
  int planes = count[img];
  if (first < 0 || planes < 0) return;
  if (planes > total - first) planes = total - first;           // never behind the stack
  if (planes <= 0) return;
  const int32_t* rk = rank + (long)img * slots;
  const T* src = inst + (long)img * h * w;
  uint8_t* out = stack + (long)first * hw;
  constexpr int kPer = VEC ? 4 : 1;
  const int items = hw / kPer;
  for (int g = blockIdx.x * kThreads + threadIdx.x; g < items; g += gridDim.x * kThreads) {
    int r[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int p = g * kPer + k;
      const int y = p / W, x = p - y * W;
      const long id = (long)src[emsa_nearest_src(y, h, H) * w + emsa_nearest_src(x, w, W)];
      r[k] = (id >= 0 && id < slots) ? rk[id] : -1;
    }
    for (int q = 0; q < planes; ++q) {
      if (VEC) {
        uint32_t word = 0u;
#pragma unroll
        for (int k = 0; k < kPer; ++k) word |= (r[k] == q ? 0xFFu : 0u) << (8 * k);
        *reinterpret_cast<uint32_t*>(out + (long)q * hw + 4l * g) = word;
      } else {
        out[(long)q * hw + g] = r[0] == q ? 255 : 0;
      }
    }
  }
}

template <typename T>
int launch_masks(const void* inst, int n, int h, int w, int H, int W, const int32_t* rank, int slots,
                 const int32_t* count, const int32_t* start, int total, uint8_t* stack, hipStream_t st) {
  const long hw = (long)H * W;
  const bool vec = hw % 4 == 0 && aligned(stack, 4);
  long blocks = ((vec ? hw / 4 : hw) + kThreads - 1) / kThreads;
  const long cap = kMaxBlocks / n > 1 ? kMaxBlocks / n : 1;
  blocks = blocks > cap ? cap : (blocks < 1 ? 1 : blocks);
  if (vec)
    hipLaunchKernelGGL((export_masks_kernel<T, true>), dim3((int)blocks, n), dim3(kThreads), 0, st,
                       (const T*)inst, h, w, H, W, rank, slots, count, start, total, stack);
  else
    hipLaunchKernelGGL((export_masks_kernel<T, false>), dim3((int)blocks, n), dim3(kThreads), 0, st,
                       (const T*)inst, h, w, H, W, rank, slots, count, start, total, stack);
  return emsa_launch_status();
}

}  // namespace

extern "C" int emsa_export_pack(const EmsaExportJob* jobs, int32_t n_jobs, int32_t n, int32_t H,
                                int32_t W, int64_t* counters, void* stream) {
  if (!jobs || !counters) return EMSA_E_ARG;
  if (n_jobs < 1 || n_jobs > EMSA_EXPORT_MAX_JOBS || n < 1 || H < 1 || W < 1) return EMSA_E_SHAPE;
  const long n_px = (long)n * H * W;
  if (n_px > 0x7fffffffl - 4) return EMSA_E_SHAPE;               // 32-bit pixel indices
  PackTable tab;
  for (int i = 0; i < n_jobs; ++i) {
    const EmsaExportJob& e = jobs[i];
    PackJob& j = tab.j[i];
    if (!e.src0 || !e.dst || !aligned(e.dst, 16)) return EMSA_E_ARG;
    if (e.kind < EMSA_EXPORT_LABEL_U8 || e.kind > EMSA_EXPORT_CLASS_SCORE_F32) return EMSA_E_ARG;
    if (e.h < 1 || e.w < 1 || (long)n * e.h * e.w > 0x7fffffffl - 4) return EMSA_E_SHAPE;
    const int b0 = label_bytes(e.src0_dtype);
    if (!b0 || !aligned(e.src0, b0)) return EMSA_E_ARG;
    if (e.lut_size < 0 || e.lut_size > 65536 || (e.lut && e.lut_size < 1)) return EMSA_E_ARG;
    const bool two_labels = e.kind == EMSA_EXPORT_SEM_INST_U16 ||
                            (e.kind == EMSA_EXPORT_PANOPTIC_BGR && e.divisor <= 0);
    int b1 = 0;
    if (e.kind == EMSA_EXPORT_CLASS_SCORE_F32) {
      if (!e.src1 || !aligned(e.src1, 4) || e.depth) return EMSA_E_ARG;
      b1 = 4;
    } else if (two_labels) {
      b1 = label_bytes(e.src1_dtype);
      if (!e.src1 || !b1 || !aligned(e.src1, b1)) return EMSA_E_ARG;
    }
    if (e.kind == EMSA_EXPORT_LABEL_U8 && e.lut_size > 256 && !e.lut) return EMSA_E_ARG;
    if (e.kind == EMSA_EXPORT_PANOPTIC_BGR && (e.divisor < 0 || e.divisor > 0x7fffffffll)) return EMSA_E_ARG;
    j.src0 = e.src0;
    j.src1 = (two_labels || e.kind == EMSA_EXPORT_CLASS_SCORE_F32) ? e.src1 : nullptr;
    j.depth = nullptr;
    j.depth_dtype = EMSA_LABEL_U16;
    j.depth_max_f32 = 0.f;
    j.depth_max_u16 = 0;
    int dbytes = 0;
    if (e.depth) {
      if (e.depth_dtype != EMSA_LABEL_U16 && e.depth_dtype != EMSA_EXPORT_DEPTH_F32) return EMSA_E_ARG;
      if (!(e.max_depth == e.max_depth)) return EMSA_E_ARG;       // NaN
      dbytes = e.depth_dtype == EMSA_LABEL_U16 ? 2 : 4;
      if (!aligned(e.depth, dbytes)) return EMSA_E_ARG;
      j.depth = e.depth;
      j.depth_dtype = e.depth_dtype;
      // uint16 d > max_depth (NumPy compares in double: exact) <=> d > floor(max_depth); a float32 map
      // is compared in float32 with max_depth rounded to float32, as NumPy does for a Python scalar
      const double fl = floor(e.max_depth);
      j.depth_max_u16 = fl < -1.0 ? -1 : (fl > 65535.0 ? 65535 : (int)fl);
      j.depth_max_f32 = (float)e.max_depth;
    }
    j.lut = e.lut;
    j.dst = e.dst;
    j.divisor = e.kind == EMSA_EXPORT_PANOPTIC_BGR ? (long)e.divisor : 0;
    j.kind = e.kind;
    j.src0_dtype = e.src0_dtype;
    j.src1_dtype = e.src1_dtype;
    j.lut_size = e.lut_size;
    j.add = e.add;
    j.h = e.h;
    j.w = e.w;
    const bool same = e.h == H && e.w == W;
    int vec = same && aligned(e.src0, 4 * b0) && (!j.src1 || aligned(j.src1, 4 * b1)) ? 1 : 0;
    if (j.depth && aligned(j.depth, 4 * dbytes)) vec |= 2;
    j.vec = vec;
  }
  for (int i = n_jobs; i < EMSA_EXPORT_MAX_JOBS; ++i) tab.j[i] = tab.j[0];
  const long groups = (n_px + 3) / 4;
  long blocks = (groups + kThreads - 1) / kThreads;
  const long cap = kMaxBlocks / n_jobs > 1 ? kMaxBlocks / n_jobs : 1;
  blocks = blocks > cap ? cap : blocks;
  hipLaunchKernelGGL(export_pack_kernel, dim3((int)blocks, n_jobs), dim3(kThreads), 0,
                     (hipStream_t)stream, tab, (int)n_px, (int)H, (int)W,
                     (unsigned long long*)counters);
  return emsa_launch_status();
}

extern "C" int emsa_export_instance_ranks(const int32_t* area, const int32_t* instance_class,
                                          const uint8_t* lut, int32_t lut_size, int32_t n,
                                          int32_t slots, int32_t* rank, int32_t* by_rank,
                                          int32_t* class_by_rank, int32_t* count, int32_t* start,
                                          int64_t* counters, void* stream) {
  if (!area || !instance_class || !rank || !by_rank || !class_by_rank || !count || !start || !counters)
    return EMSA_E_ARG;
  if (lut_size < 0 || lut_size > 65536 || (lut && lut_size < 1)) return EMSA_E_ARG;
  if (n < 1 || n > 65535 || slots < 2 || slots > 65536) return EMSA_E_SHAPE;
  hipLaunchKernelGGL(export_ranks_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, area,
                     instance_class, lut, lut_size, n, slots, rank, by_rank, class_by_rank, count, start,
                     (unsigned long long*)counters);
  return emsa_launch_status();
}

extern "C" int emsa_export_instance_masks(const void* instance, int32_t instance_dtype, int32_t n,
                                          int32_t h, int32_t w, int32_t H, int32_t W,
                                          const int32_t* rank, int32_t slots, const int32_t* count,
                                          const int32_t* start, int32_t total, uint8_t* stack,
                                          void* stream) {
  if (!instance || !rank || !count || !start) return EMSA_E_ARG;
  if (n < 1 || n > 65535 || h < 1 || w < 1 || H < 1 || W < 1 || slots < 2 || total < 0 ||
      (long)H * W > 0x7fffffffl || (long)h * w > 0x7fffffffl)
    return EMSA_E_SHAPE;
  if (total == 0) return EMSA_OK;                                // an empty stack: nothing to write
  if (!stack) return EMSA_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  switch (instance_dtype) {
    case EMSA_LABEL_I64:
      return launch_masks<int64_t>(instance, n, h, w, H, W, rank, slots, count, start, total, stack, st);
    case EMSA_LABEL_I32:
      return launch_masks<int32_t>(instance, n, h, w, H, W, rank, slots, count, start, total, stack, st);
    case EMSA_LABEL_U8:
      return launch_masks<uint8_t>(instance, n, h, w, H, W, rank, slots, count, start, total, stack, st);
    default: return EMSA_E_ARG;
  }
}

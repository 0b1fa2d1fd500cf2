// Training targets on device: the multi-scale semantic / instance / orientation targets the reference
// builds on the CPU in its data-loader workers (/root/reference/emsanet/preprocessing.py:89-104,156-213:
// InstanceClearStuffIDs, MultiscaleSupervisionGenerator, InstanceTargetGenerator,
// OrientationTargetGenerator), from the raw semantic and instance label maps of a batch.  The rules
// are stated in emsanet_amd/targets.py.  Three launches serve every scale (the scale and the image
// are grid dimensions):
//   stats     count / sum_y / sum_x per (scale, image, id): integer atomics in per-workgroup LDS
//             bins, merged with global integer atomics
//   finalize  sums -> centres (round half to even, in integers), a compact centre list per
//             (scale, image), and the accumulators are zero again for the next call
//   render    every output of a pixel in one go; the centres whose window reaches the tile and the
//             Gaussian table sit in LDS
// All arithmetic up to the one fp32 division of the offsets is integer, and the heat map is a
// maximum of table values: no result depends on the execution order.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kStatsPixels = 4096;         // pixels of one stats workgroup: uint32 partial sums hold
                                           // 4096 * 32767 < 2^27
constexpr int kTileW = 64, kTileH = 16;    // render tile; a thread writes kTileH / 4 pixels of a column
constexpr int kMaxDim = 32767;             // a centre is packed (cy << 16) | cx into an int32
constexpr int kMaxInstances = 1024;
constexpr int kMaxSigma = 16;              // table of 2 * 49^2 + 1 floats = 19 KiB of LDS

struct ScaleGeom {
  int32_t s, hs, ws, radius, table_off, table_len, inst;   // inst: instance targets at this scale
};
struct Geom {
  int32_t n_scales, n, h, w, m, n_classes;
  ScaleGeom sc[EMSA_TARGETS_MAX_SCALES];
};
struct Outputs {
  EmsaTargetScale sc[EMSA_TARGETS_MAX_SCALES];
};

// workspace: acc u64[n_scales][n][3][m] | list i32[n_scales][n][m] | centre_of i32[n_scales][n][m]
//            | n_centres i32[n_scales][n]
__host__ __device__ inline size_t ws_acc_bytes(int ns, int n, int m) { return (size_t)ns * n * 3 * m * 8; }
__host__ __device__ inline size_t ws_list_bytes(int ns, int n, int m) { return (size_t)ns * n * m * 4; }
__host__ __device__ inline unsigned long long* ws_acc(void* ws, const Geom& g, int z, int img) {
  return (unsigned long long*)ws + ((size_t)z * g.n + img) * 3 * g.m;
}
__host__ __device__ inline int32_t* ws_list(void* ws, const Geom& g, int z, int img) {
  return (int32_t*)((char*)ws + ws_acc_bytes(g.n_scales, g.n, g.m)) + ((size_t)z * g.n + img) * g.m;
}
__host__ __device__ inline int32_t* ws_centre_of(void* ws, const Geom& g, int z, int img) {
  return ws_list(ws, g, z, img) + (size_t)g.n_scales * g.n * g.m;
}
__host__ __device__ inline int32_t* ws_count(void* ws, const Geom& g, int z, int img) {
  return (int32_t*)((char*)ws + ws_acc_bytes(g.n_scales, g.n, g.m) +
                    2 * ws_list_bytes(g.n_scales, g.n, g.m)) + (size_t)z * g.n + img;
}

__device__ __forceinline__ long load_label(const void* p, int dtype, long i) {
  switch (dtype) {
    case EMSA_LABEL_I64: return (long)((const int64_t*)p)[i];
    case EMSA_LABEL_I32: return (long)((const int32_t*)p)[i];
    case EMSA_LABEL_U8: return (long)((const uint8_t*)p)[i];
    case EMSA_LABEL_I16: return (long)((const int16_t*)p)[i];
    default: return (long)((const uint16_t*)p)[i];
  }
}

// the instance id left after the stuff clearing: 0 for stuff, void and for a pixel with a label or id
// out of range (bit 0 of *bad: id, bit 1: label)
__device__ __forceinline__ int cleared_id(long sem, long id, const uint8_t* __restrict__ is_thing,
                                          int n_classes, int m, int* bad) {
  const bool bad_id = id < 0 || id >= m, bad_sem = sem < 0 || sem >= n_classes;
  *bad = (bad_id ? 1 : 0) | (bad_sem ? 2 : 0);
  if (bad_id || bad_sem || sem == 0 || !is_thing[sem]) return 0;
  return (int)id;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = EMSA_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- statistics ------------------------------------------------------------------------------
// grid (blocks of kStatsPixels pixels, image, scale).  A wave whose 64 pixels carry one id (the inside
// of an instance) adds its three sums once; a mixed wave adds per lane.
__global__ __launch_bounds__(kThreads) void targets_stats_kernel(
    const void* __restrict__ sem, int sem_dt, const void* __restrict__ inst, int inst_dt,
    const uint8_t* __restrict__ is_thing, Geom g, void* __restrict__ ws) {
  extern __shared__ uint32_t bins[];                  // [3][m]: count, sum_y, sum_x
  const int z = blockIdx.z, img = blockIdx.y, tid = threadIdx.x, m = g.m;
  const ScaleGeom sc = g.sc[z];
  const int npx = sc.hs * sc.ws, first = blockIdx.x * kStatsPixels;
  if (!sc.inst || first >= npx) return;
  for (int k = tid; k < 3 * m; k += kThreads) bins[k] = 0u;
  __syncthreads();
  const long base = (long)img * g.h * g.w;
  for (int i0 = first; i0 < npx && i0 < first + kStatsPixels; i0 += kThreads) {
    const int i = i0 + tid;
    int id = 0, y = 0, x = 0;
    if (i < npx) {
      y = i / sc.ws;
      x = i - y * sc.ws;
      const long src = base + (long)(y * sc.s) * g.w + x * sc.s;
      int bad;
      id = cleared_id(load_label(sem, sem_dt, src), load_label(inst, inst_dt, src), is_thing,
                      g.n_classes, m, &bad);
    }
    if (__all(id == __shfl(id, 0))) {
      if (id == 0) continue;
      const uint32_t sy = wave_sum((uint32_t)y), sx = wave_sum((uint32_t)x);
      if ((tid & (EMSA_WAVE - 1)) == 0) {
        atomicAdd(bins + id, (uint32_t)EMSA_WAVE);
        atomicAdd(bins + m + id, sy);
        atomicAdd(bins + 2 * m + id, sx);
      }
    } else if (id) {
      atomicAdd(bins + id, 1u);
      atomicAdd(bins + m + id, (uint32_t)y);
      atomicAdd(bins + 2 * m + id, (uint32_t)x);
    }
  }
  __syncthreads();
  unsigned long long* acc = ws_acc(ws, g, z, img);
  for (int k = tid; k < 3 * m; k += kThreads)
    if (bins[k]) atomicAdd(acc + k, (unsigned long long)bins[k]);   // (sum_y / sum_x are 0 with count 0 only)
}

// ---- finalize --------------------------------------------------------------------------------
__device__ __forceinline__ int round_half_even(unsigned long long sum, unsigned long long count) {
  const unsigned long long q = sum / count, r2 = 2 * (sum - q * count);
  return (int)(q + (r2 > count || (r2 == count && (q & 1ull)) ? 1 : 0));
}

// grid (image, scale).  Thread t owns the ids [t * per, (t + 1) * per): the list is in id order.
__global__ __launch_bounds__(kThreads) void targets_finalize_kernel(Geom g, void* __restrict__ ws) {
  __shared__ int s_off[kThreads + 1];
  const int z = blockIdx.y, img = blockIdx.x, tid = threadIdx.x, m = g.m;
  if (!g.sc[z].inst) return;
  unsigned long long* acc = ws_acc(ws, g, z, img);
  int32_t* list = ws_list(ws, g, z, img);
  int32_t* centre_of = ws_centre_of(ws, g, z, img);
  const int per = (m + kThreads - 1) / kThreads;
  const int lo = tid * per, hi = lo + per < m ? lo + per : m;
  int mine = 0;
  for (int id = lo; id < hi; ++id) mine += acc[id] != 0ull;
  s_off[tid + 1] = mine;
  if (tid == 0) s_off[0] = 0;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t <= kThreads; ++t) s_off[t] += s_off[t - 1];
    *ws_count(ws, g, z, img) = s_off[kThreads];
  }
  __syncthreads();
  int at = s_off[tid];
  for (int id = lo; id < hi; ++id) {
    const unsigned long long count = acc[id];
    int packed = -1;
    if (count) {
      packed = (round_half_even(acc[m + id], count) << 16) | round_half_even(acc[2 * m + id], count);
      list[at++] = packed;
      acc[id] = 0ull;
      acc[m + id] = 0ull;
      acc[2 * m + id] = 0ull;
    }
    centre_of[id] = packed;
  }
}

// ---- render ----------------------------------------------------------------------------------
// grid (tiles of the scale with the most, image, scale); dynamic LDS: int32[m] centres + the table
__global__ __launch_bounds__(kThreads) void targets_render_kernel(
    const void* __restrict__ sem, int sem_dt, const void* __restrict__ inst, int inst_dt,
    const float* __restrict__ orientations, const uint8_t* __restrict__ is_thing,
    const uint8_t* __restrict__ use_orientation, const float* __restrict__ gauss, int normalized,
    Geom g, Outputs out, void* __restrict__ ws, int32_t* __restrict__ flags) {
  extern __shared__ int32_t smem[];
  __shared__ int s_n;
  const int z = blockIdx.z, img = blockIdx.y, tid = threadIdx.x, m = g.m;
  const ScaleGeom sc = g.sc[z];
  const EmsaTargetScale o = out.sc[z];
  const int tiles_x = (sc.ws + kTileW - 1) / kTileW, tiles_y = (sc.hs + kTileH - 1) / kTileH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;
  const int ty0 = ((int)blockIdx.x / tiles_x) * kTileH, tx0 = ((int)blockIdx.x % tiles_x) * kTileW;
  int32_t* s_list = smem;
  float* s_tab = (float*)(smem + m);
  const int R = sc.radius;
  if (tid == 0) s_n = 0;
  __syncthreads();
  if (sc.inst) {
    for (int k = tid; k < sc.table_len; k += kThreads) s_tab[k] = gauss[sc.table_off + k];
    const int32_t* list = ws_list(ws, g, z, img);
    const int n_centres = *ws_count(ws, g, z, img);
    for (int k = tid; k < n_centres; k += kThreads) {
      const int c = list[k], cy = c >> 16, cx = c & 0xFFFF;
      if (cy + R >= ty0 && cy - R < ty0 + kTileH && cx + R >= tx0 && cx - R < tx0 + kTileW)
        s_list[atomicAdd(&s_n, 1)] = c;               // (the order does not matter: a maximum)
    }
  }
  __syncthreads();
  const int n_near = s_n;
  const int32_t* centre_of = ws_centre_of(ws, g, z, img);
  const long base = (long)img * g.h * g.w;
  const int x = tx0 + (tid & (kTileW - 1));
  int bad_any = 0;
  for (int r = 0; r < kTileH / 4; ++r) {
    const int y = ty0 + (tid >> 6) + 4 * r;
    if (y >= sc.hs || x >= sc.ws) continue;
    const long src = base + (long)(y * sc.s) * g.w + x * sc.s;
    const long label = load_label(sem, sem_dt, src);
    int bad;
    const int id = cleared_id(label, inst ? load_label(inst, inst_dt, src) : 0, is_thing, g.n_classes,
                              m, &bad);
    bad_any |= bad;
    const long pix = ((long)img * sc.hs + y) * sc.ws + x;
    if (o.semantic) o.semantic[pix] = label;
    if (!sc.inst) continue;
    float heat = 0.f;
    for (int k = 0; k < n_near; ++k) {
      const int c = s_list[k], dy = y - (c >> 16), dx = x - (c & 0xFFFF);
      if (dy >= -R && dy <= R && dx >= -R && dx <= R) heat = fmaxf(heat, s_tab[dy * dy + dx * dx]);
    }
    o.center[pix] = heat;
    float2 off = make_float2(0.f, 0.f);
    float angle = 0.f;
    uint8_t ofg = 0;
    const int c = id ? centre_of[id] : -1;            // (a pixel with an id was counted: c >= 0)
    if (c >= 0) {
      const float dy = (float)((c >> 16) - y), dx = (float)((c & 0xFFFF) - x);
      off = normalized ? make_float2(dy / (float)sc.hs, dx / (float)sc.ws) : make_float2(dy, dx);
      if (orientations) {
        const float a = orientations[(long)img * m + id];
        if (a == a) {
          angle = a;
          ofg = use_orientation[label] ? 1 : 0;
        }
      }
    }
    *reinterpret_cast<float2*>(o.offset + 2 * pix) = off;
    o.foreground[pix] = c >= 0 ? 1 : 0;
    if (o.orientation) {
      o.orientation[pix] = angle;
      o.orientation_foreground[pix] = ofg;
    }
  }
  if (bad_any & 1) atomicOr(flags + 0, 1);
  if (bad_any & 2) atomicOr(flags + 1, 1);
}

// host: geometry of a call, EMSA_E_SHAPE / EMSA_E_ARG before any launch
int make_geom(int32_t n, int32_t h, int32_t w, int32_t n_classes, int32_t max_instances,
              const EmsaTargetScale* scales, int32_t n_scales, Geom* g) {
  if (!scales) return EMSA_E_ARG;
  if (n < 1 || h < 1 || w < 1 || h > kMaxDim || w > kMaxDim || n_scales < 1 ||
      n_scales > EMSA_TARGETS_MAX_SCALES || max_instances < 2 || max_instances > kMaxInstances ||
      n_classes < 1)
    return EMSA_E_SHAPE;
  g->n_scales = n_scales;
  g->n = n;
  g->h = h;
  g->w = w;
  g->m = max_instances;
  g->n_classes = n_classes;
  int off = 0;
  for (int z = 0; z < n_scales; ++z) {
    const EmsaTargetScale& e = scales[z];
    ScaleGeom& sc = g->sc[z];
    if (e.scale < 1 || h % e.scale || w % e.scale) return EMSA_E_SHAPE;
    sc.s = e.scale;
    sc.hs = h / e.scale;
    sc.ws = w / e.scale;
    sc.inst = e.center != nullptr;
    if (sc.inst) {
      if (e.sigma < 1 || e.sigma > kMaxSigma) return EMSA_E_SHAPE;
      if (!e.offset || !e.foreground || (e.orientation != nullptr) != (e.orientation_foreground != nullptr))
        return EMSA_E_ARG;
    } else if (!e.semantic) {
      return EMSA_E_ARG;                     // a scale without any output
    }
    sc.radius = sc.inst ? 3 * e.sigma + 1 : 0;
    sc.table_off = off;
    sc.table_len = sc.inst ? 2 * sc.radius * sc.radius + 1 : 0;
    off += sc.table_len;
  }
  return EMSA_OK;
}

bool label_dtype_ok(int dt) { return dt >= EMSA_LABEL_I64 && dt <= EMSA_LABEL_U16; }

}  // namespace

extern "C" {

int64_t emsa_targets_workspace_bytes(int32_t n_images, int32_t n_scales, int32_t max_instances) {
  if (n_images < 1 || n_scales < 1 || n_scales > EMSA_TARGETS_MAX_SCALES || max_instances < 2 ||
      max_instances > kMaxInstances)
    return EMSA_E_SHAPE;
  return (int64_t)(ws_acc_bytes(n_scales, n_images, max_instances) +
                   2 * ws_list_bytes(n_scales, n_images, max_instances) +
                   (size_t)n_scales * n_images * 4);
}

int emsa_targets_table_entries(int32_t sigma) {
  if (sigma < 1 || sigma > kMaxSigma) return EMSA_E_SHAPE;
  return 2 * (3 * sigma + 1) * (3 * sigma + 1) + 1;
}

int emsa_targets_stats(const void* semantic, int32_t semantic_dtype, const void* instance,
                       int32_t instance_dtype, const uint8_t* is_thing, int32_t n_classes, int32_t n,
                       int32_t h, int32_t w, const EmsaTargetScale* scales, int32_t n_scales,
                       int32_t max_instances, void* workspace, void* stream) {
  Geom g;
  const int st = make_geom(n, h, w, n_classes, max_instances, scales, n_scales, &g);
  if (st != EMSA_OK) return st;
  if (!semantic || !instance || !is_thing || !workspace || !label_dtype_ok(semantic_dtype) ||
      !label_dtype_ok(instance_dtype))
    return EMSA_E_ARG;
  int blocks = 0;
  for (int z = 0; z < n_scales; ++z)
    if (g.sc[z].inst) {
      const int b = (g.sc[z].hs * g.sc[z].ws + kStatsPixels - 1) / kStatsPixels;
      blocks = b > blocks ? b : blocks;
    }
  if (!blocks) return EMSA_OK;
  hipLaunchKernelGGL(targets_stats_kernel, dim3(blocks, n, n_scales), dim3(kThreads),
                     3 * (size_t)max_instances * sizeof(uint32_t), (hipStream_t)stream, semantic,
                     semantic_dtype, instance, instance_dtype, is_thing, g, workspace);
  return emsa_launch_status();
}

int emsa_targets_finalize(int32_t n, int32_t h, int32_t w, const EmsaTargetScale* scales,
                          int32_t n_scales, int32_t max_instances, void* workspace, void* stream) {
  Geom g;
  const int st = make_geom(n, h, w, 1, max_instances, scales, n_scales, &g);
  if (st != EMSA_OK) return st;
  if (!workspace) return EMSA_E_ARG;
  hipLaunchKernelGGL(targets_finalize_kernel, dim3(n, n_scales), dim3(kThreads), 0,
                     (hipStream_t)stream, g, workspace);
  return emsa_launch_status();
}

int emsa_targets_render(const void* semantic, int32_t semantic_dtype, const void* instance,
                        int32_t instance_dtype, const float* orientations, const uint8_t* is_thing,
                        const uint8_t* use_orientation, int32_t n_classes, int32_t n, int32_t h,
                        int32_t w, const EmsaTargetScale* scales, int32_t n_scales,
                        int32_t max_instances, int32_t normalized_offset, const float* gauss_tables,
                        void* workspace, int32_t* flags, void* stream) {
  Geom g;
  const int st = make_geom(n, h, w, n_classes, max_instances, scales, n_scales, &g);
  if (st != EMSA_OK) return st;
  if (!semantic || !is_thing || !workspace || !flags || !label_dtype_ok(semantic_dtype) ||
      (instance && !label_dtype_ok(instance_dtype)))
    return EMSA_E_ARG;
  Outputs out;
  int tiles = 0, table_max = 0;
  bool any_inst = false;
  for (int z = 0; z < n_scales; ++z) {
    out.sc[z] = scales[z];
    const int t = ((g.sc[z].ws + kTileW - 1) / kTileW) * ((g.sc[z].hs + kTileH - 1) / kTileH);
    tiles = t > tiles ? t : tiles;
    table_max = g.sc[z].table_len > table_max ? g.sc[z].table_len : table_max;
    any_inst |= g.sc[z].inst != 0;
    if (scales[z].orientation && (!orientations || !use_orientation)) return EMSA_E_ARG;
  }
  if (any_inst && (!gauss_tables || !instance)) return EMSA_E_ARG;
  const size_t lds = ((size_t)max_instances + table_max) * 4;
  hipLaunchKernelGGL(targets_render_kernel, dim3(tiles, n, n_scales), dim3(kThreads), lds,
                     (hipStream_t)stream, semantic, semantic_dtype, instance, instance_dtype,
                     orientations, is_thing, use_orientation, gauss_tables, normalized_offset, g, out,
                     workspace, flags);
  return emsa_launch_status();
}

}  // extern "C"

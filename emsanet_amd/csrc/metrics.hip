// Validation metrics on device: the counting behind `valid_semantic_miou` and
// `valid_panoptic_all_deeplab_pq`, the two values the reference checkpoints on
// (/root/reference/main.py:229, emsanet/args.py:1054).  The label maps are already in HBM after the
// eval post-processing; counting them there is one pass over 8 + 8 bytes per pixel.
//  * confusion matrix cm[target][pred] of two label maps (int64 / int32 / uint8)
//  * panoptic quality (Kirillov et al., CVPR 2019) by the DeepLab2 / panopticapi rules: per image
//    the pixel count of every (target segment, predicted segment) pair, then the matching --
//    optionally with the list of matched (predicted id, target id) pairs written out
//  * angular error of per-instance mean orientations against a ground-truth angle table, over the
//    instance slots or over such a match list (`valid_orientation_mae_gt_deg`,
//    `valid_panoptic_mae_deeplab_deg`)
// Every sum is an integer taken with integer atomics: no result depends on the execution order.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;

// ---- confusion matrix ------------------------------------------------------------------------
constexpr int kCmLdsBins = 12288;          // 48 KiB of uint32 bins per workgroup: C <= 110

// grid-stride over the pixels, kUnroll independent loads in flight per thread.  LDS: the workgroup
// counts into private uint32 bins (a workgroup sees < 2^32 pixels: emsa_confusion_matrix bounds n)
// and merges the non-zero ones into the int64 matrix once.  A label outside [0, C) is counted in
// n_invalid and touches no bin.
template <typename TP, typename TT, bool LDS>
__global__ __launch_bounds__(kThreads) void confusion_kernel(
    const TP* __restrict__ pred, const TT* __restrict__ target, long n, int C,
    unsigned long long* __restrict__ cm, unsigned long long* __restrict__ n_invalid) {
  extern __shared__ uint32_t bins[];
  __shared__ uint32_t s_bad;
  const int tid = threadIdx.x, cc = C * C;
  if (LDS)
    for (int k = tid; k < cc; k += kThreads) bins[k] = 0u;
  if (tid == 0) s_bad = 0u;
  __syncthreads();
  uint32_t bad = 0u;
  const long stride = (long)gridDim.x * kThreads;
  for (long i0 = (long)blockIdx.x * kThreads + tid; i0 < n; i0 += kUnroll * stride) {
    long t[kUnroll], p[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const long i = i0 + j * stride;
      const bool in = i < n;
      t[j] = in ? (long)target[i] : -1;
      p[j] = in ? (long)pred[i] : -1;
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (i0 + j * stride >= n) break;
      if (t[j] < 0 || t[j] >= C || p[j] < 0 || p[j] >= C) { ++bad; continue; }
      const int bin = (int)t[j] * C + (int)p[j];
      if (LDS) atomicAdd(bins + bin, 1u);
      else atomicAdd(cm + bin, 1ull);
    }
  }
  if (bad) atomicAdd(&s_bad, bad);
  __syncthreads();
  if (LDS)
    for (int k = tid; k < cc; k += kThreads)
      if (bins[k]) atomicAdd(cm + k, (unsigned long long)bins[k]);
  if (tid == 0 && s_bad) atomicAdd(n_invalid, (unsigned long long)s_bad);
}

template <typename TP, typename TT>
int launch_confusion(const void* pred, const void* target, long n, int C, int64_t* cm,
                     int64_t* n_invalid, hipStream_t st) {
  long blocks = (n + kThreads * 16 - 1) / (kThreads * 16);
  blocks = blocks > 2048 ? 2048 : (blocks < 1 ? 1 : blocks);
  const size_t bins = (size_t)C * C;
  if (bins <= (size_t)kCmLdsBins)
    hipLaunchKernelGGL((confusion_kernel<TP, TT, true>), dim3((int)blocks), dim3(kThreads),
                       bins * sizeof(uint32_t), st, (const TP*)pred, (const TT*)target, n, C,
                       (unsigned long long*)cm, (unsigned long long*)n_invalid);
  else
    hipLaunchKernelGGL((confusion_kernel<TP, TT, false>), dim3((int)blocks), dim3(kThreads), 0, st,
                       (const TP*)pred, (const TT*)target, n, C, (unsigned long long*)cm,
                       (unsigned long long*)n_invalid);
  return emsa_launch_status();
}

template <typename TP>
int dispatch_confusion_target(int target_dtype, const void* pred, const void* target, long n, int C,
                              int64_t* cm, int64_t* n_invalid, hipStream_t st) {
  switch (target_dtype) {
    case EMSA_LABEL_I64: return launch_confusion<TP, int64_t>(pred, target, n, C, cm, n_invalid, st);
    case EMSA_LABEL_I32: return launch_confusion<TP, int32_t>(pred, target, n, C, cm, n_invalid, st);
    case EMSA_LABEL_U8: return launch_confusion<TP, uint8_t>(pred, target, n, C, cm, n_invalid, st);
    default: return EMSA_E_ARG;
  }
}

// ---- panoptic targets ------------------------------------------------------------------------
// id = sem * divisor + (is_thing[sem] ? inst : 0); void (sem == 0) and labels outside the table: 0
template <typename TS, typename TI>
__global__ __launch_bounds__(kThreads) void panoptic_targets_kernel(
    const TS* __restrict__ sem, const TI* __restrict__ inst, const uint8_t* __restrict__ is_thing,
    int n_classes, long divisor, long n, int64_t* __restrict__ out) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const long s = (long)sem[i];
    long id = 0;
    if (s > 0 && s < n_classes) id = s * divisor + (is_thing[s] ? (long)inst[i] : 0);
    out[i] = id;
  }
}

template <typename TS, typename TI>
int launch_targets(const void* sem, const void* inst, const uint8_t* is_thing, int n_classes,
                   long divisor, long n, int64_t* out, hipStream_t st) {
  long blocks = (n + kThreads * 4 - 1) / (kThreads * 4);
  blocks = blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks);
  hipLaunchKernelGGL((panoptic_targets_kernel<TS, TI>), dim3((int)blocks), dim3(kThreads), 0, st,
                     (const TS*)sem, (const TI*)inst, is_thing, n_classes, divisor, n, out);
  return emsa_launch_status();
}

template <typename TS>
int dispatch_targets_inst(int inst_dtype, const void* sem, const void* inst, const uint8_t* is_thing,
                          int n_classes, long divisor, long n, int64_t* out, hipStream_t st) {
  switch (inst_dtype) {
    case EMSA_LABEL_I64: return launch_targets<TS, int64_t>(sem, inst, is_thing, n_classes, divisor, n, out, st);
    case EMSA_LABEL_I32: return launch_targets<TS, int32_t>(sem, inst, is_thing, n_classes, divisor, n, out, st);
    case EMSA_LABEL_U8: return launch_targets<TS, uint8_t>(sem, inst, is_thing, n_classes, divisor, n, out, st);
    default: return EMSA_E_ARG;
  }
}

// ---- panoptic pair counting --------------------------------------------------------------------
// Workspace of one image (T = max_segments):
//   keys_t[T], keys_p[T]  uint64  open-addressing tables id + 1 -> slot (0 = free), linear probing
//   pair[T][T]            int32   pixels of (target slot, predicted slot)
// The slot of a segment is its position in the table, so it needs no second pass and no waiting:
// a position is claimed by one 64-bit compare-and-swap and never changes afterwards.  Which segment
// gets which slot depends on who comes first; everything derived from the matrix (areas = row /
// column sums, overlaps) is a sum over slots and does not.
constexpr int kMaxSegments = 1024;         // T * T + 1 must fit the uint32 pair key
constexpr int kPairHash = 2048;            // per-workgroup LDS (pair -> count) table
constexpr int kPairProbes = 16;
constexpr int kFlagOverflow = 0, kFlagInvalid = 1;

__host__ __device__ inline size_t pan_image_bytes(int T) {
  const size_t b = (size_t)2 * T * sizeof(unsigned long long) + (size_t)T * T * sizeof(int32_t);
  return (b + 15) & ~(size_t)15;             // the next image's 64-bit keys stay aligned
}

__device__ __forceinline__ uint32_t id_hash(unsigned long long key1) {
  return emsa_lowbias32((uint32_t)key1 ^ ((uint32_t)(key1 >> 32) * 0x85EBCA6Bu));
}

// slot of segment `key1` (= id + 1): looked up in the workgroup's LDS mirror of the image's table,
// claimed in the global table on a miss.  -1: the table is full (more than T segments).
__device__ __forceinline__ int segment_slot(unsigned long long key1,
                                            volatile unsigned long long* mirror,
                                            unsigned long long* table, int T) {
  int pos = (int)(id_hash(key1) % (uint32_t)T);
  for (int probe = 0; probe < T; ++probe) {
    unsigned long long k = mirror[pos];
    if (k == 0ull) {
      k = atomicCAS(table + pos, 0ull, key1);
      if (k == 0ull) k = key1;
      mirror[pos] = k;                       // (whoever writes a position writes the same key)
    }
    if (k == key1) return pos;
    pos = pos + 1 == T ? 0 : pos + 1;
  }
  return -1;
}

__device__ __forceinline__ void pair_add(uint32_t pair1, int count, volatile uint32_t* hkey,
                                         uint32_t* hkey_rw, int* hcount, int32_t* pair) {
  uint32_t pos = emsa_lowbias32(pair1) & (kPairHash - 1);
  for (int probe = 0; probe < kPairProbes; ++probe) {
    uint32_t k = hkey[pos];
    if (k == 0u) {
      k = atomicCAS(hkey_rw + pos, 0u, pair1);
      if (k == 0u) k = pair1;
    }
    if (k == pair1) { atomicAdd(hcount + pos, count); return; }
    pos = (pos + 1) & (kPairHash - 1);
  }
  atomicAdd(pair + (pair1 - 1u), count);     // LDS table crowded: straight to the matrix
}

// grid = (blocks per image, images).  A thread folds runs of equal (target, pred) ids before it
// looks anything up; counts go to the LDS pair table and from there once to the matrix.
__global__ __launch_bounds__(kThreads) void panoptic_pairs_kernel(
    const int64_t* __restrict__ pred, const int64_t* __restrict__ target, long hw, int T,
    unsigned char* __restrict__ workspace, int32_t* __restrict__ flags) {
  __shared__ unsigned long long mirror_t[kMaxSegments], mirror_p[kMaxSegments];
  __shared__ uint32_t hkey[kPairHash];
  __shared__ int hcount[kPairHash];
  const int tid = threadIdx.x;
  const long img = blockIdx.y;
  unsigned char* ws = workspace + img * pan_image_bytes(T);
  unsigned long long* keys_t = (unsigned long long*)ws;
  unsigned long long* keys_p = keys_t + T;
  int32_t* pair = (int32_t*)(keys_p + T);
  for (int k = tid; k < T; k += kThreads) { mirror_t[k] = 0ull; mirror_p[k] = 0ull; }
  for (int k = tid; k < kPairHash; k += kThreads) { hkey[k] = 0u; hcount[k] = 0; }
  __syncthreads();
  const int64_t* tg = target + img * hw;
  const int64_t* pr = pred + img * hw;
  long run_t = -1, run_p = -1;
  int run = 0, flag = 0;                       // bit k: flags[k] to be raised
  auto flush = [&]() {
    if (run == 0) return;
    if (run_t < 0 || run_p < 0) { flag |= 1 << kFlagInvalid; return; }
    const int st = segment_slot((unsigned long long)run_t + 1ull, mirror_t, keys_t, T);
    const int sp = segment_slot((unsigned long long)run_p + 1ull, mirror_p, keys_p, T);
    if (st < 0 || sp < 0) { flag |= 1 << kFlagOverflow; return; }
    pair_add((uint32_t)(st * T + sp) + 1u, run, hkey, hkey, hcount, pair);
  };
  const long stride = (long)gridDim.x * kThreads;
  for (long q0 = (long)blockIdx.x * kThreads + tid; q0 < hw; q0 += kUnroll * stride) {
    long t[kUnroll], p[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const long q = q0 + j * stride;
      const bool in = q < hw;
      t[j] = in ? (long)tg[q] : 0;
      p[j] = in ? (long)pr[q] : 0;
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (q0 + j * stride >= hw) break;
      if (run && t[j] == run_t && p[j] == run_p) { ++run; continue; }
      flush();
      run_t = t[j]; run_p = p[j]; run = 1;
    }
  }
  flush();
  if (flag & (1 << kFlagOverflow)) atomicOr(flags + kFlagOverflow, 1);
  if (flag & (1 << kFlagInvalid)) atomicOr(flags + kFlagInvalid, 1);
  __syncthreads();
  for (int k = tid; k < kPairHash; k += kThreads)
    if (hkey[k]) atomicAdd(pair + (hkey[k] - 1u), hcount[k]);
}

// ---- panoptic matching -------------------------------------------------------------------------
// round(inter / uni * 2^40) for 0 < inter <= uni < 2^31, in integers (two 20-bit long-division steps)
__device__ __forceinline__ unsigned long long iou_fixed40(unsigned long long inter,
                                                          unsigned long long uni) {
  const unsigned long long a = inter << 20, q1 = a / uni, r1 = a - q1 * uni;
  const unsigned long long b = r1 << 20, q2 = b / uni, r2 = b - q2 * uni;
  return (q1 << 20) + q2 + (2ull * r2 >= uni ? 1ull : 0ull);
}

// one workgroup per image; thread = predicted slot, loop = target slots (coalesced matrix rows).
// EXPORT: every match is also written as (predicted id, target id) into the image's list
// matches[img][T][2]; a slot of the list is claimed by an LDS counter (first come first: the order
// inside the list is unspecified), the counter ends up in n_matches[img].  A target matches at most
// one prediction (IoU > 1/2), so an image has at most T matches.
template <bool EXPORT>
__global__ __launch_bounds__(kThreads) void panoptic_match_kernel(
    const unsigned char* __restrict__ workspace, int T, int num_categories, int ignored,
    long max_inst, unsigned long long* __restrict__ tp, unsigned long long* __restrict__ fn,
    unsigned long long* __restrict__ fp, unsigned long long* __restrict__ iou_sum,
    int32_t* __restrict__ flags, int64_t* __restrict__ matches, int32_t* __restrict__ n_matches) {
  // category of a slot: -1 free, -2 outside [0, num_categories)
  __shared__ int cat_t[kMaxSegments], cat_p[kMaxSegments];
  __shared__ int area_t[kMaxSegments], area_p[kMaxSegments], void_p[kMaxSegments];
  __shared__ int hit_t[kMaxSegments], hit_p[kMaxSegments];
  __shared__ int s_matches;
  const int tid = threadIdx.x;
  if (EXPORT && tid == 0) s_matches = 0;       // (visible after the first barrier below)
  const unsigned char* ws = workspace + (long)blockIdx.x * pan_image_bytes(T);
  const unsigned long long* keys_t = (const unsigned long long*)ws;
  const unsigned long long* keys_p = keys_t + T;
  const int32_t* pair = (const int32_t*)(keys_p + T);
  bool bad = false;
  for (int k = tid; k < T; k += kThreads) {
    const unsigned long long kt = keys_t[k], kp = keys_p[k];
    const unsigned long long ct = kt ? (kt - 1ull) / (unsigned long long)max_inst : 0ull;
    const unsigned long long cp = kp ? (kp - 1ull) / (unsigned long long)max_inst : 0ull;
    cat_t[k] = !kt ? -1 : (ct < (unsigned long long)num_categories ? (int)ct : -2);
    cat_p[k] = !kp ? -1 : (cp < (unsigned long long)num_categories ? (int)cp : -2);
    bad = bad || cat_t[k] == -2 || cat_p[k] == -2;
    area_t[k] = 0; hit_t[k] = 0; hit_p[k] = 0;
  }
  if (bad) atomicOr(flags + kFlagInvalid, 1);
  __syncthreads();
  // areas = row / column sums; void_p = overlap with target segments of the ignored category
  for (int sp = tid; sp < T; sp += kThreads) {
    int ap = 0, vp = 0;
    if (cat_p[sp] != -1)
      for (int st = 0; st < T; ++st) {
        if (cat_t[st] == -1) continue;
        const int v = pair[(long)st * T + sp];
        if (!v) continue;
        ap += v;
        if (cat_t[st] == ignored) vp += v;
        atomicAdd(area_t + st, v);
      }
    area_p[sp] = ap;
    void_p[sp] = vp;
  }
  __syncthreads();
  for (int sp = tid; sp < T; sp += kThreads) {
    const int c = cat_p[sp];
    if (c < 0 || c == ignored) continue;
    for (int st = 0; st < T; ++st) {
      if (cat_t[st] != c) continue;
      const long inter = pair[(long)st * T + sp];
      if (!inter) continue;
      const long uni = (long)area_t[st] + area_p[sp] - inter - void_p[sp];
      if (2 * inter > uni) {
        hit_t[st] = 1;
        hit_p[sp] = 1;
        atomicAdd(tp + c, 1ull);
        atomicAdd(iou_sum + c, iou_fixed40((unsigned long long)inter, (unsigned long long)uni));
        if (EXPORT) {
          const int slot = atomicAdd(&s_matches, 1);
          if (slot < T) {
            int64_t* m = matches + ((long)blockIdx.x * T + slot) * 2;
            m[0] = (int64_t)(keys_p[sp] - 1ull);
            m[1] = (int64_t)(keys_t[st] - 1ull);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < T; k += kThreads) {
    const int ct = cat_t[k], cp = cat_p[k];
    if (ct >= 0 && ct != ignored && !hit_t[k]) atomicAdd(fn + ct, 1ull);
    if (cp >= 0 && cp != ignored && !hit_p[k] && !(2l * void_p[k] > (long)area_p[k]))
      atomicAdd(fp + cp, 1ull);
  }
  if (EXPORT && tid == 0) n_matches[blockIdx.x] = s_matches < T ? s_matches : T;
}

// ---- angular error -----------------------------------------------------------------------------
// One thread per instance slot (identity mode: slot j against ground-truth id j) or per entry of a
// match list (matched mode: predicted id % divisor against target id % divisor).  The angle of an
// instance is atan2 of its two fixed-point sums in double; the error is rounded once to 2^-40 rad and
// added as an integer, so the sum does not depend on the order.
constexpr double kTwoPi = 6.283185307179586;
constexpr double kAngleOne = 1099511627776.0;      // 2^40

template <bool MATCHED>
__global__ __launch_bounds__(kThreads) void angular_error_kernel(
    const long long* __restrict__ vec, const int32_t* __restrict__ count,
    const uint8_t* __restrict__ keep, int slots, const float* __restrict__ gt, int gt_slots,
    const int64_t* __restrict__ matches, const int32_t* __restrict__ n_matches, int T, long divisor,
    unsigned long long* __restrict__ acc, int32_t* __restrict__ flag) {
  __shared__ unsigned long long s_err;
  __shared__ unsigned int s_cnt;
  const int tid = threadIdx.x;
  if (tid == 0) { s_err = 0ull; s_cnt = 0u; }
  __syncthreads();
  const long img = blockIdx.y;
  const int k = blockIdx.x * kThreads + tid;
  long ps = -1, gs = -1;                       // predicted slot, ground-truth id
  if (MATCHED) {
    int nm = n_matches[img];
    nm = nm < T ? nm : T;
    if (k < nm) {
      const int64_t* m = matches + (img * T + k) * 2;
      const long pi = (long)(m[0] % divisor), gi = (long)(m[1] % divisor);
      if (m[0] >= 0 && m[1] >= 0 && pi > 0 && gi > 0) { ps = pi; gs = gi; }   // (0: a stuff segment)
    }
  } else if (k >= 1 && k < slots) {
    ps = k; gs = k;
  }
  if (ps > 0) {
    const bool ps_ok = ps < slots;
    if (!ps_ok) {
      atomicOr(flag, 1);                       // (matched mode: a predicted instance beyond the sums)
    } else if (count[img * slots + ps] > 0 && (!keep || keep[img * slots + ps])) {
      if (gs >= gt_slots) {
        atomicOr(flag, 1);
      } else {
        const float g = gt[img * gt_slots + gs];
        if (g == g) {                          // NaN: this instance carries no orientation
          const double s = (double)vec[(img * slots + ps) * 2];
          const double c = (double)vec[(img * slots + ps) * 2 + 1];
          double th = atan2(s, c);
          if (th < 0.0) th += kTwoPi;
          const double d = fmod(fabs(th - (double)g), kTwoPi);
          const double err = fmin(d, kTwoPi - d);
          atomicAdd(&s_err, (unsigned long long)llrint(err * kAngleOne));
          atomicAdd(&s_cnt, 1u);
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0 && s_cnt) {
    atomicAdd(acc, s_err);
    atomicAdd(acc + 1, (unsigned long long)s_cnt);
  }
}

}  // namespace

extern "C" int emsa_confusion_matrix(const void* pred, int32_t pred_dtype, const void* target,
                                     int32_t target_dtype, int64_t n, int32_t n_classes,
                                     int64_t* cm, int64_t* n_invalid, void* stream) {
  if (!pred || !target || !cm || !n_invalid) return EMSA_E_ARG;
  if (n < 1 || n > (1ll << 40) || n_classes < 1 || n_classes > 46340) return EMSA_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const long N = (long)n;
  switch (pred_dtype) {
    case EMSA_LABEL_I64:
      return dispatch_confusion_target<int64_t>(target_dtype, pred, target, N, n_classes, cm, n_invalid, st);
    case EMSA_LABEL_I32:
      return dispatch_confusion_target<int32_t>(target_dtype, pred, target, N, n_classes, cm, n_invalid, st);
    case EMSA_LABEL_U8:
      return dispatch_confusion_target<uint8_t>(target_dtype, pred, target, N, n_classes, cm, n_invalid, st);
    default: return EMSA_E_ARG;
  }
}

extern "C" int emsa_panoptic_targets(const void* semantic, int32_t semantic_dtype,
                                     const void* instance, int32_t instance_dtype,
                                     const uint8_t* is_thing, int32_t n_classes,
                                     int64_t label_divisor, int64_t n, int64_t* out, void* stream) {
  if (!semantic || !instance || !is_thing || !out) return EMSA_E_ARG;
  if (n < 1 || n_classes < 1 || label_divisor < 1) return EMSA_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  switch (semantic_dtype) {
    case EMSA_LABEL_I64:
      return dispatch_targets_inst<int64_t>(instance_dtype, semantic, instance, is_thing, n_classes,
                                            (long)label_divisor, (long)n, out, st);
    case EMSA_LABEL_I32:
      return dispatch_targets_inst<int32_t>(instance_dtype, semantic, instance, is_thing, n_classes,
                                            (long)label_divisor, (long)n, out, st);
    case EMSA_LABEL_U8:
      return dispatch_targets_inst<uint8_t>(instance_dtype, semantic, instance, is_thing, n_classes,
                                            (long)label_divisor, (long)n, out, st);
    default: return EMSA_E_ARG;
  }
}

extern "C" int64_t emsa_panoptic_workspace_bytes(int32_t n_images, int32_t max_segments) {
  if (n_images < 1 || max_segments < 1 || max_segments > kMaxSegments) return 0;
  return (int64_t)n_images * (int64_t)pan_image_bytes(max_segments);
}

extern "C" int emsa_panoptic_pairs(const int64_t* pred, const int64_t* target, int32_t n_images,
                                   int64_t hw, int32_t max_segments, void* workspace,
                                   int32_t* flags, void* stream) {
  if (!pred || !target || !workspace || !flags) return EMSA_E_ARG;
  if (n_images < 1 || n_images > 65535 || hw < 1 || hw > 0x7fffffffll || max_segments < 1 ||
      max_segments > kMaxSegments)
    return EMSA_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  emsa_zero_async(workspace, (size_t)emsa_panoptic_workspace_bytes(n_images, max_segments), st);
  long blocks = (hw + kThreads * 16 - 1) / (kThreads * 16);
  blocks = blocks > 64 ? 64 : blocks;
  hipLaunchKernelGGL(panoptic_pairs_kernel, dim3((int)blocks, n_images), dim3(kThreads), 0, st, pred,
                     target, (long)hw, max_segments, (unsigned char*)workspace, flags);
  return emsa_launch_status();
}

extern "C" int emsa_panoptic_match(const void* workspace, int32_t n_images, int32_t max_segments,
                                   int32_t num_categories, int32_t ignored_label,
                                   int64_t max_instances_per_category, int64_t* tp, int64_t* fn,
                                   int64_t* fp, int64_t* iou_sum, int32_t* flags, void* stream) {
  if (!workspace || !tp || !fn || !fp || !iou_sum || !flags) return EMSA_E_ARG;
  if (n_images < 1 || max_segments < 1 || max_segments > kMaxSegments || num_categories < 1 ||
      max_instances_per_category < 1)
    return EMSA_E_SHAPE;
  hipLaunchKernelGGL(panoptic_match_kernel<false>, dim3(n_images), dim3(kThreads), 0,
                     (hipStream_t)stream, (const unsigned char*)workspace, max_segments,
                     num_categories, ignored_label, (long)max_instances_per_category,
                     (unsigned long long*)tp, (unsigned long long*)fn, (unsigned long long*)fp,
                     (unsigned long long*)iou_sum, flags, (int64_t*)nullptr, (int32_t*)nullptr);
  return emsa_launch_status();
}

extern "C" int emsa_panoptic_match_pairs(const void* workspace, int32_t n_images,
                                         int32_t max_segments, int32_t num_categories,
                                         int32_t ignored_label, int64_t max_instances_per_category,
                                         int64_t* tp, int64_t* fn, int64_t* fp, int64_t* iou_sum,
                                         int64_t* matches, int32_t* n_matches, int32_t* flags,
                                         void* stream) {
  if (!workspace || !tp || !fn || !fp || !iou_sum || !matches || !n_matches || !flags)
    return EMSA_E_ARG;
  if (n_images < 1 || max_segments < 1 || max_segments > kMaxSegments || num_categories < 1 ||
      max_instances_per_category < 1)
    return EMSA_E_SHAPE;
  hipLaunchKernelGGL(panoptic_match_kernel<true>, dim3(n_images), dim3(kThreads), 0,
                     (hipStream_t)stream, (const unsigned char*)workspace, max_segments,
                     num_categories, ignored_label, (long)max_instances_per_category,
                     (unsigned long long*)tp, (unsigned long long*)fn, (unsigned long long*)fp,
                     (unsigned long long*)iou_sum, flags, matches, n_matches);
  return emsa_launch_status();
}

extern "C" int emsa_angular_error(const int64_t* vec_sum, const int32_t* count, const uint8_t* keep,
                                  int32_t n, int32_t slots, const float* gt_angles,
                                  int32_t gt_slots, const int64_t* matches,
                                  const int32_t* n_matches, int32_t max_segments,
                                  int64_t label_divisor, int64_t* acc, int32_t* flag, void* stream) {
  if (!vec_sum || !count || !gt_angles || !acc || !flag) return EMSA_E_ARG;
  if ((matches == nullptr) != (n_matches == nullptr)) return EMSA_E_ARG;
  if (n < 1 || n > 65535 || slots < 2 || gt_slots < 2) return EMSA_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (matches) {
    if (max_segments < 1 || max_segments > kMaxSegments || label_divisor < 1) return EMSA_E_SHAPE;
    hipLaunchKernelGGL(angular_error_kernel<true>, dim3((max_segments + kThreads - 1) / kThreads, n),
                       dim3(kThreads), 0, st, (const long long*)vec_sum, count, keep, slots,
                       gt_angles, gt_slots, matches, n_matches, max_segments, (long)label_divisor,
                       (unsigned long long*)acc, flag);
  } else {
    hipLaunchKernelGGL(angular_error_kernel<false>, dim3((slots + kThreads - 1) / kThreads, n),
                       dim3(kThreads), 0, st, (const long long*)vec_sum, count, keep, slots,
                       gt_angles, gt_slots, (const int64_t*)nullptr, (const int32_t*)nullptr, 0, 1l,
                       (unsigned long long*)acc, flag);
  }
  return emsa_launch_status();
}

// The half-resolution stage between the two 7x7 stem convolutions and layer1, fp32, C = 64, training
// mode, as four passes over memory:
//
//   y_rgb, y_depth (conv outputs) --BN+ReLU--> a_rgb, a_depth --SE-add--> f --max pool--> P_f
//                                                       a_depth ------------max pool--> P_d
//
//   forward  1  stem_squeeze_kernel      gap_m = mean relu(y_m * scale_m + shift_m)   (reads y twice)
//            2  stem_pool_fwd_kernel     P_f, idx_f, P_d, idx_d from the 18 taps of y_rgb / y_depth
//   backward 1  stem_bwd_reduce_kernel   SE ds and the pieces of the BatchNorm sums per image
//            2  stem_bwd_apply_kernel    dy_rgb, dy_depth
//
// a = relu(y * scale + shift), its mask and xhat are recomputed from y where they are needed: the
// kernels are HBM bound and the vector work is free.  Every piece of arithmetic that also exists in
// pointwise.hip is spelled the same way (bn_math.h; the SE product as se_scale_add_fwd_kernel is
// compiled: fma(a_rgb, s_rgb, a_depth * s_depth)), so that forward pass 2 is bit-equal to
// se_scale_add + maxpool_fwd x2 and the squeeze to channel_mean(bn_act(y)).
//
// The BatchNorm sums of the backward pass are linear in the per-image constants s[n,c] and
// dgap[n,c] / HW, which are only known after the SE MLP backward: pass 1 therefore accumulates, per
// image and channel,  ds = sum dout a,  A0 = sum mask dout,  A1 = sum mask dout xhat,  M0 = sum mask,
// M1 = sum mask xhat  (depth also D0 = sum mask dd, D1 = sum mask dd xhat), and
// stem_bwd_finalize_kernel forms   dbeta = sum_n s A0 + dgap/HW M0 (+ D0),   dgamma likewise.
// No atomics: per-thread fp32 sums, lanes merged in a fixed order, everything above in fp64.
#include <cstdlib>

#include "common.h"
#include "bn_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kC = 64;                        // channels of the stage
constexpr int kCvn = kC / 4;                  // float4 per pixel
constexpr int kLanes = kThreads / kCvn;       // pixels (quads) a workgroup handles at a time
constexpr int kSums = 12;                     // per image and channel, see Q_*
constexpr int kMaxBlocks = 256 * 8;
// order of the sums: rgb {ds, A0, A1, M0, M1}, depth {ds, A0, A1, M0, M1, D0, D1}
enum { Q_DS = 0, Q_A0 = 1, Q_A1 = 2, Q_M0 = 3, Q_M1 = 4, Q_DEPTH = 5, Q_D0 = 10, Q_D1 = 11 };

__device__ __forceinline__ void ld4v(const float* p, float (&v)[4]) {
  const float4 f = emsa_ld4(p);
  v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
}
__device__ __forceinline__ void cvt4(const float4& f, float (&v)[4]) {
  v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
}

// per-channel vectors of the two BatchNorms (index 0 = rgb, 1 = depth)
struct StemAffine {
  const float* scale[2];
  const float* shift[2];
};
struct StemStats {
  const float* mean[2];
  const float* invstd[2];
};

// ------------------------------------------------------------------------------------------
// forward pass 1: the two SE squeezes from y.  Workgroups, pixel partition and summation order are
// those of channel_dot_kernel<float, false> in its paired form (emsa_se_pair_fwd_t): ws =
// [2][n][splits][c], bit-equal to the sums over the materialised activation.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void stem_squeeze_kernel(
    const float* __restrict__ y_rgb, const float* __restrict__ y_depth, const StemAffine aff,
    float* __restrict__ ws, long hw, int splits, int nblk) {
  __shared__ __attribute__((aligned(16))) float cred[kLanes * kC];
  const bool second = (int)blockIdx.x >= nblk;
  const int blk = second ? blockIdx.x - nblk : blockIdx.x;
  const float* __restrict__ y = second ? y_depth : y_rgb;
  const int img = blk / splits, sp = blk % splits;
  const long chunk = (hw + splits - 1) / splits;
  const long p0 = img * hw + sp * chunk, p1 = min(img * hw + (sp + 1) * chunk, (img + 1) * hw);
  const int cv = threadIdx.x % kCvn, rl = threadIdx.x / kCvn;
  float sc[4], sh[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
  ld4v((second ? aff.scale[1] : aff.scale[0]) + cv * 4, sc);
  ld4v((second ? aff.shift[1] : aff.shift[0]) + cv * 4, sh);
  auto term = [&](const float4& r) {
    float v[4];
    cvt4(r, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += fmaxf(bn_affine(v[k], sc[k], sh[k]), 0.f);
  };
  long p = p0 + rl;
  for (; p + 3 * kLanes < p1; p += 4 * kLanes) {
    float4 r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = emsa_ld4(y + ((p + u * kLanes) * kCvn + cv) * 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) term(r[u]);
  }
  for (; p < p1; p += kLanes) term(emsa_ld4(y + (p * kCvn + cv) * 4));
#pragma unroll
  for (int k = 0; k < 4; ++k) cred[rl * kC + cv * 4 + k] = acc[k];
  __syncthreads();
  for (int ch = threadIdx.x; ch < kC; ch += kThreads) {
    float t = 0.f;
    for (int k = 0; k < kLanes; ++k) t += cred[k * kC + ch];
    ws[(long)blockIdx.x * kC + ch] = t;
  }
}

// ------------------------------------------------------------------------------------------
// forward pass 2: one thread = one pooled pixel x 4 channels (maxpool_fwd_kernel's enumeration, tap
// order, strict `>` and first-in-range-tap rule); all 18 taps are loaded first, at clamped
// coordinates.
// ------------------------------------------------------------------------------------------
template <typename I>
__global__ __launch_bounds__(kThreads) void stem_pool_fwd_kernel(
    const float* __restrict__ y_rgb, const float* __restrict__ y_depth, const StemAffine aff,
    const float* __restrict__ s_rgb, const float* __restrict__ s_depth, float* __restrict__ pf,
    int8_t* __restrict__ idx_f, float* __restrict__ pd, int8_t* __restrict__ idx_d, int n, int h,
    int w) {
  const int oh_n = (h + 1) / 2, ow_n = (w + 1) / 2;
  const I total = (I)n * oh_n * ow_n * kCvn;
  // (the grid stride is a multiple of kCvn: a thread keeps its channel vector)
  const int c4 = threadIdx.x % kCvn;
  float scr[4], shr[4], scd[4], shd[4];
  ld4v(aff.scale[0] + c4 * 4, scr);
  ld4v(aff.shift[0] + c4 * 4, shr);
  ld4v(aff.scale[1] + c4 * 4, scd);
  ld4v(aff.shift[1] + c4 * 4, shd);
  for (I i = blockIdx.x * (I)kThreads + threadIdx.x; i < total; i += (I)gridDim.x * kThreads) {
    I r = i / (I)kCvn;
    const int ow = (int)(r % (I)ow_n); r /= (I)ow_n;
    const int oh = (int)(r % (I)oh_n);
    const int img = (int)(r / (I)oh_n);
    float4 tr[9], td[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ih = min(max(oh * 2 - 1 + kh, 0), h - 1), iw = min(max(ow * 2 - 1 + kw, 0), w - 1);
        const size_t o = (size_t)(((((I)img * h + ih) * w + iw) * kCvn + c4) * 4);
        tr[kh * 3 + kw] = emsa_ld4(y_rgb + o);
        td[kh * 3 + kw] = emsa_ld4(y_depth + o);
      }
    float sr[4], sd[4];
    ld4v(s_rgb + ((size_t)img * kCvn + c4) * 4, sr);
    ld4v(s_depth + ((size_t)img * kCvn + c4) * 4, sd);
    float bf[4], bd[4];
    int kf[4] = {0, 0, 0, 0}, kd[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) bf[k] = bd[k] = -INFINITY;
    bool first = true;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ih = oh * 2 - 1 + kh, iw = ow * 2 - 1 + kw, t = kh * 3 + kw;
        const bool in = ih >= 0 && ih < h && iw >= 0 && iw < w;
        float vr[4], vd[4];
        cvt4(tr[t], vr);
        cvt4(td[t], vd);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float ar = fmaxf(bn_affine(vr[k], scr[k], shr[k]), 0.f);
          const float ad = fmaxf(bn_affine(vd[k], scd[k], shd[k]), 0.f);
          const float f = __builtin_fmaf(ar, sr[k], bn_mul(ad, sd[k]));
          if (in && (first || f > bf[k])) { bf[k] = f; kf[k] = t; }
          if (in && (first || ad > bd[k])) { bd[k] = ad; kd[k] = t; }
        }
        first = first && !in;
      }
    emsa_st4(pf + (size_t)i * 4, make_float4(bf[0], bf[1], bf[2], bf[3]));
    emsa_st4(pd + (size_t)i * 4, make_float4(bd[0], bd[1], bd[2], bd[3]));
    *reinterpret_cast<char4*>(idx_f + (size_t)i * 4) = make_char4(kf[0], kf[1], kf[2], kf[3]);
    *reinterpret_cast<char4*>(idx_d + (size_t)i * 4) = make_char4(kd[0], kd[1], kd[2], kd[3]);
  }
}

// ------------------------------------------------------------------------------------------
// backward: one thread = a 2x2 quad of /2 pixels x 4 channels (maxpool_bwd_kernel's enumeration).
// The quad (2qh.., 2qw..) lies under the four windows (qh..qh+1, qw..qw+1); a window or a pixel
// outside the map is loaded at clamped coordinates and masked out afterwards, so all 24 loads of a
// quad are issued before the first is used.
// ------------------------------------------------------------------------------------------
struct QuadIn {
  float4 gf[4], gd[4];        // window gradients of P_f / P_d
  uint32_t kf[4], kd[4];      // their argmax taps (4 x int8)
  float4 yr[4], yd[4];        // the quad's pixels of y_rgb / y_depth
};

template <typename I>
__device__ __forceinline__ void quad_issue(QuadIn& q, const float* __restrict__ gf,
                                           const int8_t* __restrict__ idx_f,
                                           const float* __restrict__ gd,
                                           const int8_t* __restrict__ idx_d,
                                           const float* __restrict__ y_rgb,
                                           const float* __restrict__ y_depth, int img, int qh, int qw,
                                           int c4, int h, int w, int oh_n, int ow_n) {
#pragma unroll
  for (int dh = 0; dh < 2; ++dh)
#pragma unroll
    for (int dw = 0; dw < 2; ++dw) {
      const int oh = min(qh + dh, oh_n - 1), ow = min(qw + dw, ow_n - 1);
      const size_t o = (size_t)(((((I)img * oh_n + oh) * ow_n + ow) * kCvn + c4) * 4);
      q.gf[dh * 2 + dw] = emsa_ld4(gf + o);
      q.gd[dh * 2 + dw] = emsa_ld4(gd + o);
      q.kf[dh * 2 + dw] = *reinterpret_cast<const uint32_t*>(idx_f + o);
      q.kd[dh * 2 + dw] = *reinterpret_cast<const uint32_t*>(idx_d + o);
    }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ih = min(2 * qh + a, h - 1), iw = min(2 * qw + b, w - 1);
      const size_t o = (size_t)(((((I)img * h + ih) * w + iw) * kCvn + c4) * 4);
      q.yr[a * 2 + b] = emsa_ld4(y_rgb + o);
      q.yd[a * 2 + b] = emsa_ld4(y_depth + o);
    }
}

// max pool backward of both pooled gradients onto the quad: dout / dd [pixel a * 2 + b][channel]
// (windows in maxpool_bwd_kernel's order)
__device__ __forceinline__ void quad_unpool(const QuadIn& q, int qh, int qw, int oh_n, int ow_n,
                                            float (&dout)[4][4], float (&dd)[4][4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int k = 0; k < 4; ++k) dout[p][k] = dd[p][k] = 0.f;
#pragma unroll
  for (int dh = 0; dh < 2; ++dh)
#pragma unroll
    for (int dw = 0; dw < 2; ++dw) {
      const bool valid = qh + dh < oh_n && qw + dw < ow_n;
      float g[4], e[4];
      cvt4(q.gf[dh * 2 + dw], g);
      cvt4(q.gd[dh * 2 + dw], e);
      const uint32_t rf = q.kf[dh * 2 + dw], rd = q.kd[dh * 2 + dw];
      // quad pixel (a, b) = input (2qh + a, 2qw + b): kh = a - 2 dh + 1, kw = b - 2 dw + 1
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int kh = a - 2 * dh + 1;
        if (kh < 0 || kh > 2) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int kw = b - 2 * dw + 1;
          if (kw < 0 || kw > 2) continue;
          const uint32_t t = (uint32_t)(kh * 3 + kw);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            dout[a * 2 + b][k] += (valid && ((rf >> (8 * k)) & 0xFFu) == t) ? g[k] : 0.f;
            dd[a * 2 + b][k] += (valid && ((rd >> (8 * k)) & 0xFFu) == t) ? e[k] : 0.f;
          }
        }
      }
    }
}

// quads per image and the chunk of them a workgroup (image, split) walks
__device__ __forceinline__ void quad_range(int oh_n, int ow_n, int splits, int sp, int& q0, int& q1) {
  const int nq = oh_n * ow_n, chunk = (nq + splits - 1) / splits;
  q0 = sp * chunk;
  q1 = min(nq, q0 + chunk);
}

// backward pass 1: ws[n][splits][kSums][c]
template <typename I>
__global__ __launch_bounds__(kThreads, 2) void stem_bwd_reduce_kernel(
    const float* __restrict__ gf, const int8_t* __restrict__ idx_f, const float* __restrict__ gd,
    const int8_t* __restrict__ idx_d, const float* __restrict__ y_rgb,
    const float* __restrict__ y_depth, const StemAffine aff, const StemStats st,
    float* __restrict__ ws, int h, int w, int splits) {
  __shared__ __attribute__((aligned(16))) float cred[kSums * kLanes * kC];
  const int oh_n = (h + 1) / 2, ow_n = (w + 1) / 2;
  const int img = blockIdx.x / splits, sp = blockIdx.x % splits;
  int q0, q1;
  quad_range(oh_n, ow_n, splits, sp, q0, q1);
  const int c4 = threadIdx.x % kCvn, rl = threadIdx.x / kCvn;
  float sc[2][4], sh[2][4], mu[2][4], is[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    ld4v(aff.scale[m] + c4 * 4, sc[m]);
    ld4v(aff.shift[m] + c4 * 4, sh[m]);
    ld4v(st.mean[m] + c4 * 4, mu[m]);
    ld4v(st.invstd[m] + c4 * 4, is[m]);
  }
  float acc[kSums][4];
#pragma unroll
  for (int s = 0; s < kSums; ++s)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[s][k] = 0.f;
  for (int qi = q0 + rl; qi < q1; qi += kLanes) {
    const int qh = qi / ow_n, qw = qi - qh * ow_n;
    QuadIn q;
    quad_issue<I>(q, gf, idx_f, gd, idx_d, y_rgb, y_depth, img, qh, qw, c4, h, w, oh_n, ow_n);
    float dout[4][4], dd[4][4];
    quad_unpool(q, qh, qw, oh_n, ow_n, dout, dd);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool pv = 2 * qh + (p >> 1) < h && 2 * qw + (p & 1) < w;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        float y[4];
        cvt4(m ? q.yd[p] : q.yr[p], y);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float z = bn_affine(y[k], sc[m][k], sh[m][k]);
          const bool on = pv && z > 0.f;
          const float g = on ? dout[p][k] : 0.f;
          const float xh = bn_mul(bn_add(y[k], -mu[m][k]), is[m][k]);
          acc[m * Q_DEPTH + Q_DS][k] = __builtin_fmaf(dout[p][k], fmaxf(z, 0.f), acc[m * Q_DEPTH + Q_DS][k]);
          acc[m * Q_DEPTH + Q_A0][k] = bn_add(acc[m * Q_DEPTH + Q_A0][k], g);
          acc[m * Q_DEPTH + Q_A1][k] = bn_acc_xhat(acc[m * Q_DEPTH + Q_A1][k], g, y[k], mu[m][k], is[m][k]);
          acc[m * Q_DEPTH + Q_M0][k] += on ? 1.f : 0.f;
          acc[m * Q_DEPTH + Q_M1][k] += on ? xh : 0.f;
          if (m == 1) {
            const float e = on ? dd[p][k] : 0.f;
            acc[Q_D0][k] = bn_add(acc[Q_D0][k], e);
            acc[Q_D1][k] = bn_acc_xhat(acc[Q_D1][k], e, y[k], mu[m][k], is[m][k]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kSums; ++s)
#pragma unroll
    for (int k = 0; k < 4; ++k) cred[(s * kLanes + rl) * kC + c4 * 4 + k] = acc[s][k];
  __syncthreads();
  for (int o = threadIdx.x; o < kSums * kC; o += kThreads) {
    const int s = o / kC, ch = o % kC;
    float t = 0.f;
    for (int k = 0; k < kLanes; ++k) t += cred[(s * kLanes + k) * kC + ch];
    ws[((long)blockIdx.x * kSums + s) * kC + ch] = t;
  }
}

// second level of the merge, fp64: sums[n][kSums][c] over the splits in order; the two SE ds rows
// also as fp32 [2][n][c] for emsa_se_mlp_bwd.  grid = (n, kSums * c / 256)
__global__ void stem_bwd_merge_kernel(const float* __restrict__ ws, int splits, int n,
                                      double* __restrict__ sums, float* __restrict__ ds) {
  const int img = blockIdx.x, o = blockIdx.y * blockDim.x + threadIdx.x;
  if (o >= kSums * kC) return;
  double a = 0.0;
#pragma unroll 4
  for (int sp = 0; sp < splits; ++sp) a += (double)ws[((long)img * splits + sp) * kSums * kC + o];
  sums[(long)img * kSums * kC + o] = a;
  const int s = o / kC, ch = o % kC;
  if (s == Q_DS) ds[(long)img * kC + ch] = (float)a;
  if (s == Q_DEPTH + Q_DS) ds[((long)n + img) * kC + ch] = (float)a;
}

// dbeta / dgamma of both BatchNorms from the per-image sums, fp64: one thread per (stream, channel)
struct StemGradOut {
  float* dgamma[2];
  float* dbeta[2];
};
__global__ void stem_bwd_finalize_kernel(const double* __restrict__ sums,
                                         const float* __restrict__ s_rgb,
                                         const float* __restrict__ s_depth,
                                         const float* __restrict__ dgap_rgb,
                                         const float* __restrict__ dgap_depth, const StemGradOut out,
                                         int n, double inv_hw) {
  const int m = threadIdx.x / kC, ch = threadIdx.x % kC;
  const float* __restrict__ s = m ? s_depth : s_rgb;
  const float* __restrict__ dgap = m ? dgap_depth : dgap_rgb;
  double db = 0.0, dg = 0.0;
  for (int img = 0; img < n; ++img) {
    const double* __restrict__ r = sums + ((long)img * kSums + m * Q_DEPTH) * kC + ch;
    const double sv = (double)s[(long)img * kC + ch], dv = (double)dgap[(long)img * kC + ch] * inv_hw;
    db += sv * r[Q_A0 * kC] + dv * r[Q_M0 * kC];
    dg += sv * r[Q_A1 * kC] + dv * r[Q_M1 * kC];
    if (m == 1) {
      db += sums[((long)img * kSums + Q_D0) * kC + ch];
      dg += sums[((long)img * kSums + Q_D1) * kC + ch];
    }
  }
  (m ? out.dbeta[1] : out.dbeta[0])[ch] = (float)db;
  (m ? out.dgamma[1] : out.dgamma[0])[ch] = (float)dg;
}

// backward pass 2: dy_rgb, dy_depth.  Same workgroups and quads as pass 1.
struct StemApplyVec {
  const float* gamma[2];
  const float* s[2];          // [n][c]
  const float* dgap[2];       // [n][c]
  const float* dgamma[2];
  const float* dbeta[2];
};
template <typename I>
__global__ __launch_bounds__(kThreads, 2) void stem_bwd_apply_kernel(
    const float* __restrict__ gf, const int8_t* __restrict__ idx_f, const float* __restrict__ gd,
    const int8_t* __restrict__ idx_d, const float* __restrict__ y_rgb,
    const float* __restrict__ y_depth, const StemAffine aff, const StemStats st,
    const StemApplyVec v, float* __restrict__ dy_rgb, float* __restrict__ dy_depth, int h, int w,
    int splits, float inv_hw, float inv_count) {
  const int oh_n = (h + 1) / 2, ow_n = (w + 1) / 2;
  const int img = blockIdx.x / splits, sp = blockIdx.x % splits;
  int q0, q1;
  quad_range(oh_n, ow_n, splits, sp, q0, q1);
  const int c4 = threadIdx.x % kCvn, rl = threadIdx.x / kCvn;
  float sc[2][4], sh[2][4], mu[2][4], is[2][4], gi[2][4], db[2][4], dg[2][4], sv[2][4], dv[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    float ga[4], dgp[4];
    ld4v(aff.scale[m] + c4 * 4, sc[m]);
    ld4v(aff.shift[m] + c4 * 4, sh[m]);
    ld4v(st.mean[m] + c4 * 4, mu[m]);
    ld4v(st.invstd[m] + c4 * 4, is[m]);
    ld4v(v.gamma[m] + c4 * 4, ga);
    ld4v(v.dbeta[m] + c4 * 4, db[m]);
    ld4v(v.dgamma[m] + c4 * 4, dg[m]);
    ld4v(v.s[m] + ((size_t)img * kCvn + c4) * 4, sv[m]);
    ld4v(v.dgap[m] + ((size_t)img * kCvn + c4) * 4, dgp);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gi[m][k] = bn_mul(ga[k], is[m][k]);
      dv[m][k] = bn_mul(dgp[k], inv_hw);
    }
  }
  for (int qi = q0 + rl; qi < q1; qi += kLanes) {
    const int qh = qi / ow_n, qw = qi - qh * ow_n;
    QuadIn q;
    quad_issue<I>(q, gf, idx_f, gd, idx_d, y_rgb, y_depth, img, qh, qw, c4, h, w, oh_n, ow_n);
    float dout[4][4], dd[4][4];
    quad_unpool(q, qh, qw, oh_n, ow_n, dout, dd);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int ih = 2 * qh + (p >> 1), iw = 2 * qw + (p & 1);
      if (ih >= h || iw >= w) continue;
      const size_t o = (size_t)(((((I)img * h + ih) * w + iw) * kCvn + c4) * 4);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        float y[4], r[4];
        cvt4(m ? q.yd[p] : q.yr[p], y);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float da = __builtin_fmaf(dout[p][k], sv[m][k], dv[m][k]);
          if (m == 1) da = bn_add(da, dd[p][k]);
          const float dz = bn_affine(y[k], sc[m][k], sh[m][k]) > 0.f ? da : 0.f;
          r[k] = bn_dx_train(dz, y[k], mu[m][k], is[m][k], gi[m][k], db[m][k], dg[m][k], inv_count);
        }
        emsa_st4((m ? dy_depth : dy_rgb) + o, make_float4(r[0], r[1], r[2], r[3]));
      }
    }
  }
}

// 32-bit element indices when the largest tensor of a launch has < 2^31 elements (EMSA_IDX32=0:
// 64-bit everywhere, A/B runs)
bool idx32_ok(long max_elements) {
  static const bool on = [] {
    const char* e = getenv("EMSA_IDX32");
    return !e || atoi(e) != 0;
  }();
  return on && max_elements > 0 && max_elements < (1L << 31);
}

// fp32 NHWC maps of exactly 64 channels, at least one pixel, image count and map size within int
bool shape_ok(int n, long h, long w, int c) {
  return c == kC && n >= 1 && h >= 1 && w >= 1 && h < (1 << 24) && w < (1 << 24) &&
         (long)n * ((h + 1) / 2) * ((w + 1) / 2) < (1L << 31) / kCvn;
}

// splits of the backward passes: ~256 quads per workgroup, at most 64 per image
int bwd_splits(int h, int w) {
  const long nq = (long)((h + 1) / 2) * ((w + 1) / 2);
  long s = (nq + 255) / 256;
  return (int)(s < 1 ? 1 : s > 64 ? 64 : s);
}

}  // namespace

extern "C" int emsa_stem_stage_squeeze(const float* y_rgb, const float* y_depth,
                                       const float* scale_rgb, const float* shift_rgb,
                                       const float* scale_depth, const float* shift_depth,
                                       float* ws, int32_t n, int64_t hw, int32_t c, void* stream) {
  if (!y_rgb || !y_depth || !scale_rgb || !shift_rgb || !scale_depth || !shift_depth || !ws)
    return EMSA_E_ARG;
  if (c != kC || n < 1 || hw < 1) return EMSA_E_SHAPE;
  // (the partition of emsa_channel_mean / emsa_se_pair_fwd_t, whose second stage reads ws)
  const int splits = emsa_channel_ws_floats(n, hw, c) / (n * c);
  if (splits < 1 || (long)2 * n * splits >= (1L << 31)) return EMSA_E_SHAPE;
  const StemAffine aff = {{scale_rgb, scale_depth}, {shift_rgb, shift_depth}};
  hipLaunchKernelGGL(stem_squeeze_kernel, dim3(2 * n * splits), dim3(kThreads), 0,
                     (hipStream_t)stream, y_rgb, y_depth, aff, ws, (long)hw, splits, n * splits);
  return emsa_launch_status();
}

extern "C" int emsa_stem_stage_fwd(const float* y_rgb, const float* y_depth, const float* scale_rgb,
                                   const float* shift_rgb, const float* scale_depth,
                                   const float* shift_depth, const float* s_rgb,
                                   const float* s_depth, float* pf, int8_t* idx_f, float* pd,
                                   int8_t* idx_d, int32_t n, int32_t h, int32_t w, int32_t c,
                                   void* stream) {
  if (!y_rgb || !y_depth || !scale_rgb || !shift_rgb || !scale_depth || !shift_depth || !s_rgb ||
      !s_depth || !pf || !idx_f || !pd || !idx_d)
    return EMSA_E_ARG;
  if (!shape_ok(n, h, w, c)) return EMSA_E_SHAPE;
  const StemAffine aff = {{scale_rgb, scale_depth}, {shift_rgb, shift_depth}};
  const long total = (long)n * ((h + 1) / 2) * ((w + 1) / 2) * kCvn;
  long blocks = (total + kThreads - 1) / kThreads;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  const dim3 grid((int)blocks), block(kThreads);
  if (idx32_ok((long)n * h * w * c))
    hipLaunchKernelGGL(stem_pool_fwd_kernel<uint32_t>, grid, block, 0, (hipStream_t)stream, y_rgb,
                       y_depth, aff, s_rgb, s_depth, pf, idx_f, pd, idx_d, n, h, w);
  else
    hipLaunchKernelGGL(stem_pool_fwd_kernel<long>, grid, block, 0, (hipStream_t)stream, y_rgb,
                       y_depth, aff, s_rgb, s_depth, pf, idx_f, pd, idx_d, n, h, w);
  return emsa_launch_status();
}

extern "C" int emsa_stem_stage_bwd_splits(int32_t h, int32_t w) {
  return h >= 1 && w >= 1 ? bwd_splits(h, w) : EMSA_E_SHAPE;
}

extern "C" int emsa_stem_stage_bwd_reduce(const float* gf, const int8_t* idx_f, const float* gd,
                                          const int8_t* idx_d, const float* y_rgb,
                                          const float* y_depth, const float* scale_rgb,
                                          const float* shift_rgb, const float* scale_depth,
                                          const float* shift_depth, const float* mean_rgb,
                                          const float* invstd_rgb, const float* mean_depth,
                                          const float* invstd_depth, float* ws, double* sums,
                                          float* ds, int32_t n, int32_t h, int32_t w, int32_t c,
                                          void* stream) {
  if (!gf || !idx_f || !gd || !idx_d || !y_rgb || !y_depth || !scale_rgb || !shift_rgb ||
      !scale_depth || !shift_depth || !mean_rgb || !invstd_rgb || !mean_depth || !invstd_depth ||
      !ws || !sums || !ds)
    return EMSA_E_ARG;
  if (!shape_ok(n, h, w, c)) return EMSA_E_SHAPE;
  const int splits = bwd_splits(h, w);
  const StemAffine aff = {{scale_rgb, scale_depth}, {shift_rgb, shift_depth}};
  const StemStats st = {{mean_rgb, mean_depth}, {invstd_rgb, invstd_depth}};
  hipStream_t s = (hipStream_t)stream;
  if (idx32_ok((long)n * h * w * c))
    hipLaunchKernelGGL(stem_bwd_reduce_kernel<uint32_t>, dim3(n * splits), dim3(kThreads), 0, s, gf,
                       idx_f, gd, idx_d, y_rgb, y_depth, aff, st, ws, h, w, splits);
  else
    hipLaunchKernelGGL(stem_bwd_reduce_kernel<long>, dim3(n * splits), dim3(kThreads), 0, s, gf,
                       idx_f, gd, idx_d, y_rgb, y_depth, aff, st, ws, h, w, splits);
  hipLaunchKernelGGL(stem_bwd_merge_kernel, dim3(n, (kSums * kC + 255) / 256), dim3(256), 0, s, ws,
                     splits, n, sums, ds);
  return emsa_launch_status();
}

extern "C" int emsa_stem_stage_bwd_finalize(const double* sums, const float* s_rgb,
                                            const float* s_depth, const float* dgap_rgb,
                                            const float* dgap_depth, float* dgamma_rgb,
                                            float* dbeta_rgb, float* dgamma_depth,
                                            float* dbeta_depth, int32_t n, int64_t hw, int32_t c,
                                            void* stream) {
  if (!sums || !s_rgb || !s_depth || !dgap_rgb || !dgap_depth || !dgamma_rgb || !dbeta_rgb ||
      !dgamma_depth || !dbeta_depth)
    return EMSA_E_ARG;
  if (c != kC || n < 1 || hw < 1) return EMSA_E_SHAPE;
  const StemGradOut out = {{dgamma_rgb, dgamma_depth}, {dbeta_rgb, dbeta_depth}};
  hipLaunchKernelGGL(stem_bwd_finalize_kernel, dim3(1), dim3(2 * kC), 0, (hipStream_t)stream, sums,
                     s_rgb, s_depth, dgap_rgb, dgap_depth, out, n, 1.0 / (double)hw);
  return emsa_launch_status();
}

extern "C" int emsa_stem_stage_bwd_apply(
    const float* gf, const int8_t* idx_f, const float* gd, const int8_t* idx_d, const float* y_rgb,
    const float* y_depth, const float* scale_rgb, const float* shift_rgb, const float* scale_depth,
    const float* shift_depth, const float* mean_rgb, const float* invstd_rgb,
    const float* mean_depth, const float* invstd_depth, const float* gamma_rgb,
    const float* gamma_depth, const float* s_rgb, const float* s_depth, const float* dgap_rgb,
    const float* dgap_depth, const float* dgamma_rgb, const float* dbeta_rgb,
    const float* dgamma_depth, const float* dbeta_depth, float* dy_rgb, float* dy_depth, int32_t n,
    int32_t h, int32_t w, int32_t c, void* stream) {
  if (!gf || !idx_f || !gd || !idx_d || !y_rgb || !y_depth || !scale_rgb || !shift_rgb ||
      !scale_depth || !shift_depth || !mean_rgb || !invstd_rgb || !mean_depth || !invstd_depth ||
      !gamma_rgb || !gamma_depth || !s_rgb || !s_depth || !dgap_rgb || !dgap_depth || !dgamma_rgb ||
      !dbeta_rgb || !dgamma_depth || !dbeta_depth || !dy_rgb || !dy_depth)
    return EMSA_E_ARG;
  if (!shape_ok(n, h, w, c)) return EMSA_E_SHAPE;
  const int splits = bwd_splits(h, w);
  const StemAffine aff = {{scale_rgb, scale_depth}, {shift_rgb, shift_depth}};
  const StemStats st = {{mean_rgb, mean_depth}, {invstd_rgb, invstd_depth}};
  const StemApplyVec v = {{gamma_rgb, gamma_depth}, {s_rgb, s_depth}, {dgap_rgb, dgap_depth},
                          {dgamma_rgb, dgamma_depth}, {dbeta_rgb, dbeta_depth}};
  const float inv_hw = 1.0f / (float)((long)h * w), inv_count = 1.0f / (float)((long)n * h * w);
  hipStream_t s = (hipStream_t)stream;
  if (idx32_ok((long)n * h * w * c))
    hipLaunchKernelGGL(stem_bwd_apply_kernel<uint32_t>, dim3(n * splits), dim3(kThreads), 0, s, gf,
                       idx_f, gd, idx_d, y_rgb, y_depth, aff, st, v, dy_rgb, dy_depth, h, w, splits,
                       inv_hw, inv_count);
  else
    hipLaunchKernelGGL(stem_bwd_apply_kernel<long>, dim3(n * splits), dim3(kThreads), 0, s, gf,
                       idx_f, gd, idx_d, y_rgb, y_depth, aff, st, v, dy_rgb, dy_depth, h, w, splits,
                       inv_hw, inv_count);
  return emsa_launch_status();
}

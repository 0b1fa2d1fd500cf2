// The optimizer updates over one flat bucket, as device functions shared by pointwise.hip (the
// plain entry points emsa_sgd_nesterov / emsa_adam_*) and loss_scale.hip (the forms that read a
// loss scaler's device state).  ONE body per optimizer, templated on LS: the scaled form differs
// from the plain one in two places only -- it returns at once when the scaler says skip, and it
// multiplies the gradient by grad_scale * inv_scale where the plain form multiplies by grad_scale.
// grad_scale * inv_scale is formed ONCE per thread, in front of the element loop, so that the
// product with the gradient is the same single multiplication in both forms: for a power-of-two
// loss scale S, (S g) * (grad_scale / S) rounds exactly as g * grad_scale does, and the scaled
// step on S g equals the plain step on g bit for bit (tests/test_loss_scale_gpu.py).
#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------
// SGD with Nesterov momentum and weight decay over one flat bucket: the update of
// torch.optim.SGD(momentum, weight_decay, nesterov=True) the reference trains with
// (/root/reference/emsanet/optimizer.py:29-36):
//   d = g * grad_scale + wd * p;  buf = first ? d : mu * buf + d;  p -= lr * (d + mu * buf)
// one pass: reads p, g, buf, writes p, buf (5 streams instead of the ~12 of a foreach SGD).
// ------------------------------------------------------------------------------------------
// hp (optional): the hyper-parameters {lr, momentum, weight_decay, grad_scale, first_step} in DEVICE
// memory -- a training step captured in a hipGraph reads the schedule's current values at replay
// time instead of the values baked into the launch
//
// LS and the first-step flag: the flag stays host-managed (FusedSGD._first) and has no device twin.
// A skipped first step leaves the momentum buffers at their initial zeros, and the next step, run
// with first = 0, forms mu * 0 + d = d -- the first-step rule.
template <bool LS>
__device__ __forceinline__ void sgd_nesterov_body(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ m, long n4, long n, float lr,
                                                  float mu, float wd, float gs, int first,
                                                  const float* __restrict__ hp,
                                                  const EmsaLossScale* __restrict__ ls) {
  if (hp) {
    lr = hp[0]; mu = hp[1]; wd = hp[2]; gs = hp[3];
    first = hp[4] != 0.f;
  }
  if constexpr (LS) {
    if (ls->skip) return;           // parameters and momentum untouched, bit for bit
    gs = gs * ls->inv_scale;
  }
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    const float4 pv = emsa_ld4(p + i * 4), gv = emsa_ld4(g + i * 4);
    float4 d = make_float4(gv.x * gs + wd * pv.x, gv.y * gs + wd * pv.y, gv.z * gs + wd * pv.z,
                           gv.w * gs + wd * pv.w);
    float4 b = d;
    if (!first) {
      const float4 mv = emsa_ld4(m + i * 4);
      b = make_float4(mu * mv.x + d.x, mu * mv.y + d.y, mu * mv.z + d.z, mu * mv.w + d.w);
    }
    emsa_st4(m + i * 4, b);
    emsa_st4(p + i * 4, make_float4(pv.x - lr * (d.x + mu * b.x), pv.y - lr * (d.y + mu * b.y),
                                    pv.z - lr * (d.z + mu * b.z), pv.w - lr * (d.w + mu * b.w)));
  }
  // tail (n not a multiple of 4)
  const long t = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (t < n) {
    const float pv = p[t], d = g[t] * gs + wd * pv;
    const float b = first ? d : mu * m[t] + d;
    m[t] = b;
    p[t] = pv - lr * (d + mu * b);
  }
}

// ------------------------------------------------------------------------------------------
// Adam / AdamW / RAdam over one flat bucket: the other three optimizers the reference's factory
// builds (/root/reference/emsanet/optimizer.py:37-57: betas (0.9, 0.999), torch's eps 1e-8, weight
// decay as L2 for adam / radam and decoupled for adamw).  The arithmetic follows torch.optim's
// single-tensor paths:
//   g' = g * grad_scale (+ wd * p for adam / radam);   adamw: p *= 1 - lr * wd
//   m += (g' - m) * (1 - b1);   v = b2 * v + (1 - b2) * g'^2
//   adam / adamw:  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
//   radam:         p -= (m / bc1) * lr * (rho_t > 5 ? sqrt(bc2) / (sqrt(v) + eps) * rect : 1)
// hyper (double[8], host-owned): {lr, b1, b2, eps, wd, grad_scale, mode (0 adam, 1 adamw, 2 radam)}
// state (double[8], DEVICE-owned): {t, lr / bc1, bc1, sqrt(bc2), rect, rho_t > 5} -- advanced by a
// one-thread kernel in front of the bucket launches, so that a step captured in a hipGraph counts
// its own replays; the step-dependent scalars are formed in double like torch's Python floats.
// One pass: reads p, g, m, v, writes p, m, v.
// LS: a skipped step advances nothing -- not the step count either, or the bias corrections of the
// steps that follow would belong to a later step than the moments they correct.
// ------------------------------------------------------------------------------------------
template <bool LS>
__device__ __forceinline__ void adam_advance_body(const double* __restrict__ hp, double* __restrict__ st,
                                                  const EmsaLossScale* __restrict__ ls) {
  if constexpr (LS) {
    if (ls->skip) return;
  }
  const double b1 = hp[1], b2 = hp[2];
  const double t = st[0] + 1.0;
  const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
  const double rho_inf = 2.0 / (1.0 - b2) - 1.0;
  const double rho_t = rho_inf - 2.0 * t * pow(b2, t) / bc2;
  double rect = 0.0;
  if (rho_t > 5.0)
    rect = sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t));
  st[0] = t;
  st[1] = hp[0] / bc1;
  st[2] = bc1;
  st[3] = sqrt(bc2);
  st[4] = rect;
  st[5] = rho_t > 5.0 ? 1.0 : 0.0;
}

// omb1 / omb2: 1 - b1 and 1 - b2, formed in double and rounded once, as torch rounds the Python floats
// `1 - beta1` / `1 - beta2` it passes to lerp_ / addcmul_.  Formed in fp32, 1.f - 0.999f is
// 0.99998713e-3: a relative error of 1.3e-5 in the new term of the second moment, 6e-6 in the update.
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float lr, float omb1,
                                         float b2, float omb2, float eps, float wd, float gs, int mode,
                                         float step_size, float bc1, float bc2_sqrt, float rect,
                                         bool use_rect) {
  float gg = g * gs;
  if (mode == 1) p = p * (1.f - lr * wd);
  else if (wd != 0.f) gg = gg + wd * p;
  m = m + (gg - m) * omb1;
  v = b2 * v + omb2 * gg * gg;
  if (mode != 2) {
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
  } else {
    const float mh = m / bc1;
    p = use_rect ? p - mh * lr * (bc2_sqrt / (sqrtf(v) + eps)) * rect : p - mh * lr;
  }
}

template <bool LS>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g,
                                          float* __restrict__ m, float* __restrict__ v, long n4, long n,
                                          const double* __restrict__ hp, const double* __restrict__ st,
                                          const EmsaLossScale* __restrict__ ls) {
#pragma clang fp contract(off)
  const float lr = (float)hp[0], b2 = (float)hp[2], eps = (float)hp[3];
  const float omb1 = (float)(1.0 - hp[1]), omb2 = (float)(1.0 - hp[2]);
  const float wd = (float)hp[4];
  float gs = (float)hp[5];
  if constexpr (LS) {
    if (ls->skip) return;           // parameters and both moments untouched, bit for bit
    gs = gs * ls->inv_scale;
  }
  const int mode = (int)hp[6];
  const float step_size = (float)st[1], bc1 = (float)st[2], bc2_sqrt = (float)st[3];
  const float rect = (float)st[4];
  const bool use_rect = st[5] != 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    float4 pv = emsa_ld4(p + i * 4), mv = emsa_ld4(m + i * 4), vv = emsa_ld4(v + i * 4);
    const float4 gv = emsa_ld4(g + i * 4);
    adam_one(pv.x, gv.x, mv.x, vv.x, lr, omb1, b2, omb2, eps, wd, gs, mode, step_size, bc1, bc2_sqrt, rect, use_rect);
    adam_one(pv.y, gv.y, mv.y, vv.y, lr, omb1, b2, omb2, eps, wd, gs, mode, step_size, bc1, bc2_sqrt, rect, use_rect);
    adam_one(pv.z, gv.z, mv.z, vv.z, lr, omb1, b2, omb2, eps, wd, gs, mode, step_size, bc1, bc2_sqrt, rect, use_rect);
    adam_one(pv.w, gv.w, mv.w, vv.w, lr, omb1, b2, omb2, eps, wd, gs, mode, step_size, bc1, bc2_sqrt, rect, use_rect);
    emsa_st4(m + i * 4, mv);
    emsa_st4(v + i * 4, vv);
    emsa_st4(p + i * 4, pv);
  }
  const long t = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (t < n) {
    float pv = p[t], mv = m[t], vv = v[t];
    adam_one(pv, g[t], mv, vv, lr, omb1, b2, omb2, eps, wd, gs, mode, step_size, bc1, bc2_sqrt, rect, use_rect);
    m[t] = mv; v[t] = vv; p[t] = pv;
  }
}

}  // namespace

// Dynamic loss scaling on the DEVICE (fp16 storage training): the non-finite scan over the flat
// gradient buckets, the one-thread update of the scaler state (the rule of torch.amp.GradScaler)
// and the optimizer updates that read that state.  Every entry point takes a stream, launches its
// kernel there and nothing else, allocates nothing and reads nothing back: the whole sequence is
// captured with the training step (a hipGraph replays the decision to skip with everything else).
//
// Order inside one step (optim.LossScaler.step):
//   backward pass, seeded with state.scale as the cotangent of the loss  -> gradients = S * g
//   emsa_nonfinite_scan per bucket          -> state.found |= any inf / NaN
//   emsa_loss_scale_update                  -> skip, inv_scale = 1 / S, scale for the NEXT step
//   emsa_sgd_nesterov_ls / emsa_adam_*_ls   -> nothing if skip, else the step on g * inv_scale
// The decision needs every bucket before any parameter moves, so the scan is a pass of its own
// (one extra read of the gradient bytes) and cannot ride in the update kernel of the same bucket.
#include "common.h"
#include "optim_step.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScanVecPerThread = 8;      // float4 loads per thread and grid-stride round
constexpr int kScanMaxBlocks = 2048;

// all exponent bits set: +-inf and every NaN (quiet, signalling, any payload)
__device__ __forceinline__ uint32_t nonfinite_bits(uint32_t u) {
  return (u & 0x7F800000u) == 0x7F800000u ? 1u : 0u;
}

// Read-only scan of n floats starting at g (4-byte aligned).  `head` (0..3) elements bring the
// address to a 16-byte boundary, n4 float4 follow, the rest is the tail; head and tail are
// checked by the first threads of workgroup 0.  A workgroup that saw a non-finite value stores 1
// into *found: every writer stores the same constant, no atomic and no ordering is needed, and
// nobody ever stores 0 here (emsa_loss_scale_update clears the flag once per step).
__global__ __launch_bounds__(kThreads) void nonfinite_scan_kernel(const float* __restrict__ g, long head,
                                                                   long n4, long n,
                                                                   int32_t* __restrict__ found) {
  uint32_t bad = 0u;
  const uint4* __restrict__ body = reinterpret_cast<const uint4*>(g + head);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    const uint4 v = body[i];
    bad |= nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
  }
  if (blockIdx.x == 0) {
    const uint32_t* __restrict__ u = reinterpret_cast<const uint32_t*>(g);
    const long t = threadIdx.x;
    if (t < head) bad |= nonfinite_bits(u[t]);
    const long tail0 = head + n4 * 4;
    if (tail0 + t < n) bad |= nonfinite_bits(u[tail0 + t]);      // (n - tail0 <= 3)
  }
  if (__syncthreads_or((int)bad) && threadIdx.x == 0) *found = 1;
}

// torch.amp.GradScaler's update (aten: _amp_update_scale_) plus the bookkeeping the update kernels
// need.  Two values are kept apart: `scale`, which the NEXT backward pass reads, and `inv_scale`,
// the reciprocal of the scale THIS step's gradients were produced with, which this step's update
// kernels read.
__global__ void loss_scale_update_kernel(EmsaLossScale* __restrict__ s, float growth, float backoff,
                                         int32_t interval) {
  const float used = s->scale;
  // (formed in double and rounded once: exact for the powers of two the default factors produce)
  s->inv_scale = (float)(1.0 / (double)used);
  s->steps += 1;
  if (s->found) {
    s->scale = used * backoff;
    s->growth_tracker = 0;
    s->skip = 1;
    s->skipped += 1;
  } else {
    s->skip = 0;
    int32_t t = s->growth_tracker + 1;
    if (t == interval) {
      const float grown = used * growth;
      if (!nonfinite_bits(__float_as_uint(grown))) s->scale = grown;   // else: growth not applied
      t = 0;
    }
    s->growth_tracker = t;
  }
  s->found = 0;
}

__global__ void sgd_nesterov_ls_kernel(float* __restrict__ p, const float* __restrict__ g,
                                       float* __restrict__ m, long n4, long n, float lr, float mu,
                                       float wd, float gs, int first, const float* __restrict__ hp,
                                       const EmsaLossScale* __restrict__ ls) {
  sgd_nesterov_body<true>(p, g, m, n4, n, lr, mu, wd, gs, first, hp, ls);
}

__global__ void adam_advance_ls_kernel(const double* __restrict__ hp, double* __restrict__ st,
                                       const EmsaLossScale* __restrict__ ls) {
  adam_advance_body<true>(hp, st, ls);
}

__global__ void adam_ls_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                               float* __restrict__ v, long n4, long n, const double* __restrict__ hp,
                               const double* __restrict__ st, const EmsaLossScale* __restrict__ ls) {
  adam_body<true>(p, g, m, v, n4, n, hp, st, ls);
}

// grid of the bucket updates: the one pointwise.hip uses for the plain forms (grid-stride loops)
inline int update_grid(long n4) {
  long b = ((n4 > 0 ? n4 : 1) + kThreads - 1) / kThreads;
  if (b > 2048) b = 2048;
  return (int)b;
}

}  // namespace

extern "C" int emsa_nonfinite_scan(const float* grad, int64_t n, EmsaLossScale* state, void* stream) {
  if (!grad || !state) return EMSA_E_ARG;
  if (n < 1) return EMSA_OK;
  const uintptr_t a = (uintptr_t)grad;
  if ((a & 3) || (((uintptr_t)state) & 3)) return EMSA_E_SHAPE;
  long head = (long)(((16 - (a & 15)) & 15) / 4);
  if (head > (long)n) head = (long)n;
  const long n4 = ((long)n - head) / 4;
  // the grid follows the byte count: one thread per kScanVecPerThread float4 (128 bytes), capped
  long blocks = (n4 + (long)kThreads * kScanVecPerThread - 1) / ((long)kThreads * kScanVecPerThread);
  if (blocks < 1) blocks = 1;
  if (blocks > kScanMaxBlocks) blocks = kScanMaxBlocks;
  hipLaunchKernelGGL(nonfinite_scan_kernel, dim3((int)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                     grad, head, n4, (long)n, &state->found);
  return emsa_launch_status();
}

extern "C" int emsa_loss_scale_update(EmsaLossScale* state, float growth_factor, float backoff_factor,
                                      int32_t growth_interval, void* stream) {
  if (!state) return EMSA_E_ARG;
  if (!(growth_factor > 1.f) || !(backoff_factor > 0.f && backoff_factor < 1.f) || growth_interval < 1)
    return EMSA_E_ARG;
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state,
                     growth_factor, backoff_factor, growth_interval);
  return emsa_launch_status();
}

extern "C" int emsa_sgd_nesterov_ls(float* param, const float* grad, float* momentum_buf, int64_t n,
                                    float lr, float momentum, float weight_decay, float grad_scale,
                                    int32_t first_step, const float* hyper, const EmsaLossScale* state,
                                    void* stream) {
  if (!param || !grad || !momentum_buf || !state) return EMSA_E_ARG;
  if (n < 1) return EMSA_OK;
  if ((((uintptr_t)param) | ((uintptr_t)grad) | ((uintptr_t)momentum_buf)) & 15) return EMSA_E_SHAPE;
  const long n4 = (long)n / 4;
  hipLaunchKernelGGL(sgd_nesterov_ls_kernel, dim3(update_grid(n4)), dim3(kThreads), 0,
                     (hipStream_t)stream, param, grad, momentum_buf, n4, (long)n, lr, momentum,
                     weight_decay, grad_scale, first_step ? 1 : 0, hyper, state);
  return emsa_launch_status();
}

extern "C" int emsa_adam_advance_ls(const double* hyper, double* adam_state, const EmsaLossScale* state,
                                    void* stream) {
  if (!hyper || !adam_state || !state) return EMSA_E_ARG;
  hipLaunchKernelGGL(adam_advance_ls_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, hyper,
                     adam_state, state);
  return emsa_launch_status();
}

extern "C" int emsa_adam_step_ls(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                 int64_t n, const double* hyper, const double* adam_state,
                                 const EmsaLossScale* state, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !hyper || !adam_state || !state) return EMSA_E_ARG;
  if (n < 1) return EMSA_OK;
  if ((((uintptr_t)param) | ((uintptr_t)grad) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 15)
    return EMSA_E_SHAPE;
  const long n4 = (long)n / 4;
  hipLaunchKernelGGL(adam_ls_kernel, dim3(update_grid(n4)), dim3(kThreads), 0, (hipStream_t)stream,
                     param, grad, exp_avg, exp_avg_sq, n4, (long)n, hyper, adam_state, state);
  return emsa_launch_status();
}

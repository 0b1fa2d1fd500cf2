// The arithmetic of the BatchNorm passes, shared by pointwise.hip and stem_stage.hip.
#pragma once
#include <hip/hip_runtime.h>

// ---- the arithmetic of the BatchNorm passes, spelled out ----------------------------------------
// One fma / mul / add per step, none left to the compiler's contraction heuristics: the general and
// the fast form of a pass (below) must round alike, and what clang fuses depends on the code around
// an expression (a product hoisted out of a loop is no longer fused into the sum behind it).
__device__ __forceinline__ float bn_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float bn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
// y = x * scale + shift
__device__ __forceinline__ float bn_affine(float x, float sc, float sh) { return __builtin_fmaf(x, sc, sh); }
// one term of sum g * xhat:  acc + (g * (x - mean)) * invstd
__device__ __forceinline__ float bn_acc_xhat(float acc, float g, float x, float mu, float is) {
  return __builtin_fmaf(bn_mul(g, bn_add(x, -mu)), is, acc);
}
// dx = gamma * invstd * (g - sum_g / N - xhat * sum_gxhat / N), gi = gamma * invstd (bn_mul)
__device__ __forceinline__ float bn_dx_train(float g, float x, float mu, float is, float gi, float db,
                                             float dg, float inv_count) {
  const float xh = bn_mul(bn_add(x, -mu), is);
  const float t = __builtin_fmaf(-db, inv_count, g);
  return bn_mul(gi, __builtin_fmaf(-bn_mul(xh, dg), inv_count, t));
}

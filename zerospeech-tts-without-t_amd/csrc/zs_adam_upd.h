// zs_adam_upd.h -- the clip + Adam update of one element (zs_adam_clip, include/zs_amd.h), shared by every kernel that applies it:
// adam_kernel and adam_pack_kernel (zs_elem.hip) and voice_adam_kernel (zs_voice.hip) compile this one expression, so that their
// results agree bit for bit.
#pragma once
#include "zs_common.h"

// The update of one element: ONE function for every kernel, so that all compile the same expression.
struct AdamCoef { float coef, step_size, bc2_sqrt, beta1, beta2, eps; };
__device__ __forceinline__ AdamCoef adam_coef(const ZsAdam& p, const float* sumsq) {
  const float gs = p.grad_scale != 0.f ? p.grad_scale : 1.f;      // 1/world: g holds the SUM over the data-parallel ranks
  float coef = gs;
  if (p.max_norm > 0.f && sumsq) {
    const float norm = sqrtf(*sumsq) * gs;
    coef = gs * fminf(p.max_norm / (norm + 1e-6f), 1.f);         // clip_grad_norm_
  }
  float bc1 = p.bc1, bc2 = p.bc2;
  if (p.step_ptr) {                                              // hipGraph replay: the step count lives on the device
    const float t = (float)(*p.step_ptr);
    bc1 = 1.f - powf(p.beta1, t);
    bc2 = 1.f - powf(p.beta2, t);
  }
  return AdamCoef{coef, p.lr / bc1, sqrtf(bc2), p.beta1, p.beta2, p.eps};
}
// Which products fuse with which sums is written out (and the compiler's own contraction is off inside): left to the compiler
// it depends on the code around the call -- the 16-byte loop fused as below, the one-element loop fused nothing in m and v --
// and a tile of zs_adam_pack must give the bits the flat loop of zs_adam_clip gives.  These are the fusions of that 16-byte
// loop, the only one a flat parameter buffer (16-byte aligned, a multiple of 4 elements) ever ran.
__device__ __forceinline__ void adam_upd(const AdamCoef& c, float& w, float& g, float& m, float& v) {
#pragma clang fp contract(off)
  const float d = __builtin_fmaf(g, c.coef, -m);                 // g - m of the scaled gradient, one rounding
  g = g * c.coef;
  m = __builtin_fmaf(d, 1.f - c.beta1, m);                       // exp_avg.lerp_(grad, 1 - beta1)
  v = __builtin_fmaf(g * g, 1.f - c.beta2, v * c.beta2);         // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  w = __builtin_fmaf(-c.step_size, m / denom, w);
}

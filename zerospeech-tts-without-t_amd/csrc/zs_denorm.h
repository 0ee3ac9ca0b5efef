// zs_denorm.h -- normalised magnitude -> amplitude (convert.py:56-58).  The one place this expression is written: gl_denorm_kernel,
// gen_scatter_kernel (zs_vocoder.hip) and xfade_gather_kernel (zs_xfade.hip) all call it, so all produce the same bits for the same
// input.  Which of its operations fuse is part of those bits, so the function states its own contraction mode -- the compiler's
// default, under which zs_vocoder.hip has always compiled it -- and a file that turns contraction off around it (zs_xfade.hip)
// does not change it.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float gl_denorm(float x) {
#pragma clang fp contract(fast)
  const float m = fminf(fmaxf(x, 0.f), 1.f) * 100.f - 100.f + 20.f;         // convert.py:57
  return powf(10.0f, m * 0.05f);                                             // convert.py:58
}

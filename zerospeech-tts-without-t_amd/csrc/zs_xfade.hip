// zs_xfade.hip -- zs_xfade_gather: the vocoder's padded input [rows][out_ld] out of decode windows that overlap.  Every output row is
// a copy of one source row or the cross-fade of two (include/zs_amd.h has the definition; convert._xfade_tables plans the tables).
// A gather of whole rows, bound by memory: one wave per output row, the grid strides over the rows.  Rows are 513 floats, so a row
// starts on a 4-byte boundary only and its phase against 16 bytes differs from row to row, and between an output row and its source
// rows.  The wave cuts the OUTPUT row: single elements up to its first 16-byte boundary, 16-byte stores over the aligned middle,
// single elements behind it.  The source rows are read at the same column offsets in 16-byte pieces at their own 4-byte alignment
// (a global load of four dwords needs dword alignment only), the two rows of a blended frame in the same pass.
// No LDS, no atomics; every element is written by one lane, so a launch is bitwise reproducible.
#include "zs_common.h"
#include "zs_denorm.h"

// the blend is two products and one sum, a rounding each: nothing in this file may be fused into a multiply-add (gl_denorm states
// its own mode, zs_denorm.h)
#pragma clang fp contract(off)

namespace {

constexpr int XF_WAVES = 4;                                // waves (rows in flight) per 256-thread workgroup
constexpr int XF_MAX_BLOCKS = 256 * 8;                     // 8 workgroups per CU: 32 waves, what a CU holds

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));     // four floats at 4-byte alignment

__device__ __forceinline__ f32x4 xf_load4(const float* p) {
  const f32x4_a4 v = *reinterpret_cast<const f32x4_a4*>(p);
  return f32x4{v.x, v.y, v.z, v.w};
}

template <bool DENORM> __device__ __forceinline__ float xf_out(float v) { return DENORM ? gl_denorm(v) : v; }

// KIND 0: no source (the row holds D(0)); 1: a copy of s0; 2: w0 * s0 + w1 * s1
// A row without a source holds D(zero), with `zero` a 0.f the compiler cannot see through (the kernel forms it from an argument): D
// of a literal 0.f would be folded at compile time by the host's pow, which is not bound to give the bits the device's powf gives
// zs_gl_denormalize and zs_gen_scatter for the same input (it did not: one ulp).
template <int KIND, bool DENORM>
__device__ __forceinline__ float xf_val(const float* s0, const float* s1, float w0, float w1, int f, float zero) {
  if (KIND == 0) return xf_out<DENORM>(zero);
  if (KIND == 1) return xf_out<DENORM>(s0[f]);
  const float a = w0 * s0[f];
  const float b = w1 * s1[f];
  return xf_out<DENORM>(a + b);
}

template <int KIND, bool DENORM>
__device__ __forceinline__ void xf_row(float* o, const float* s0, const float* s1, float w0, float w1, int cols, int lane, float zero) {
  int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(o) >> 2) & 3u)) & 3u);    // elements before the first 16-byte boundary
  if (head > cols) head = cols;
  const int nvec = (cols - head) >> 2;
  const int tail0 = head + 4 * nvec;                       // the first of the at most 3 elements behind the aligned middle
  for (int v = lane; v < nvec; v += 64) {
    const int f = head + 4 * v;
    f32x4 r;
    if (KIND == 0) {
      const float z = xf_out<DENORM>(zero);
      r = f32x4{z, z, z, z};
    } else if (KIND == 1) {
      const f32x4 x = xf_load4(s0 + f);
      r = f32x4{xf_out<DENORM>(x.x), xf_out<DENORM>(x.y), xf_out<DENORM>(x.z), xf_out<DENORM>(x.w)};
    } else {
      const f32x4 x = xf_load4(s0 + f), y = xf_load4(s1 + f);
      const f32x4 a = x * w0;
      const f32x4 b = y * w1;
      const f32x4 s = a + b;
      r = f32x4{xf_out<DENORM>(s.x), xf_out<DENORM>(s.y), xf_out<DENORM>(s.z), xf_out<DENORM>(s.w)};
    }
    *reinterpret_cast<f32x4*>(o + f) = r;
  }
  // the two ends: lanes 0 .. head - 1 the elements before the middle, the next lanes those behind it (at most 3 + 3)
  const int ntail = cols - tail0;
  if (lane < head) o[lane] = xf_val<KIND, DENORM>(s0, s1, w0, w1, lane, zero);
  else if (lane - head < ntail) o[tail0 + lane - head] = xf_val<KIND, DENORM>(s0, s1, w0, w1, tail0 + lane - head, zero);
}

template <bool DENORM>
__global__ void __launch_bounds__(64 * XF_WAVES) xfade_gather_kernel(const ZsXfadeGather p) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * XF_WAVES;
  const float zero = (float)(p.cols >> 31);                // 0.f: cols >= 0 (checked at the entry point)
  for (int64_t r = (int64_t)blockIdx.x * XF_WAVES + (threadIdx.x >> 6); r < p.rows; r += step) {     // r is uniform over the wave
    const int64_t a = p.i0[r], b = p.i1[r];
    float* o = p.out + r * p.out_ld;
    if (a < 0 || a >= p.src_rows || b < -1 || b >= p.src_rows) {          // no source, or a bad table entry: nothing is read
      xf_row<0, DENORM>(o, nullptr, nullptr, 0.f, 0.f, p.cols, lane, zero);
    } else if (b < 0) {
      xf_row<1, DENORM>(o, p.src + a * p.ld_src, nullptr, 0.f, 0.f, p.cols, lane, zero);
    } else {
      xf_row<2, DENORM>(o, p.src + a * p.ld_src, p.src + b * p.ld_src, p.w0[r], p.w1[r], p.cols, lane, zero);
    }
  }
}

}  // namespace

extern "C" int zs_xfade_gather(const ZsXfadeGather* p, void* stream) {
  ZS_REQUIRE(p, "zs_xfade_gather: null argument");
  ZS_REQUIRE(p->rows >= 0 && p->src_rows >= 0 && p->ld_src >= 0 && p->out_ld >= 0 && p->cols >= 0, "zs_xfade_gather: negative size");
  ZS_REQUIRE(p->cols <= p->ld_src && p->cols <= p->out_ld, "zs_xfade_gather: cols must be <= ld_src and <= out_ld");
  ZS_REQUIRE(p->rows < ((int64_t)1 << 31), "zs_xfade_gather: rows must be < 2^31");
  if (p->rows == 0) return ZS_OK;
  ZS_REQUIRE(p->src && p->i0 && p->i1 && p->w0 && p->w1 && p->out, "zs_xfade_gather: null operand");
  int64_t nb = (p->rows + XF_WAVES - 1) / XF_WAVES;
  if (nb > XF_MAX_BLOCKS) nb = XF_MAX_BLOCKS;
  if (p->denorm)
    hipLaunchKernelGGL(xfade_gather_kernel<true>, dim3((unsigned)nb), dim3(64 * XF_WAVES), 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL(xfade_gather_kernel<false>, dim3((unsigned)nb), dim3(64 * XF_WAVES), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_xfade_gather");
}

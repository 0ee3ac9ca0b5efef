// zs_quant.h -- what the quantiser files (zs_vq.hip, zs_vq_train.hip, zs_rvq.hip, zs_rvq_train.hip, zs_rvq_drop.hip) share: the guarded
// row accesses of their memory-bound kernels, the hash of the device draws and the host arithmetic of a launch over teams.  Each was a
// copy per file under a prefix of its own (rq_, rt_, rd_, vt_, vq_, vr_); the definitions the kernels are tested against bit for bit
// now have one text.
// Not folded, and why:
//   vq_load4 (zs_vq.hip)                 q_load4 with an `ok` operand and an early return for c >= E in front of the vector branch: the
//                                        staging loop of vq_tile_products is built around both.
//   vt_load, vt_load_code (zs_vq_train.hip)   8-column forms with the same early return, used by vq_commit_kernel and vq_st_bwd_kernel,
//                                        which take the difference in double and are different arithmetic anyway.
//   the store of r in rvq_residual_kernel (zs_rvq.hip)   q_store4's text written out: through q_store4 the compiler allots the kernel's
//                                        registers differently (64 SGPRs and 30 VGPRs for 62 and 32), and this change moves no
//                                        kernel's instruction stream.
//   RtVec (zs_rvq_train.hip)             one user is left, so it stays beside it.
#pragma once
#include "zs_common.h"

// the definitions are stated operation by operation (a rounding each): nothing below this line, in this header or in the file that
// includes it, may be fused into a multiply-add.  The pragma holds to the end of the translation unit; zs_vq.hip, whose scores and
// norms contract, says so behind the include.
#pragma clang fp contract(off)

namespace {

inline bool misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

// ---- a launch over teams -----------------------------------------------------------------------------------------------------------
// A row is owned by a team of 2^t <= 64 lanes of one wave, one piece per lane and round: the least such team that covers `groups` pieces.
inline int team_lanes(int groups) {
  int tl = 1;
  while (tl < groups && tl < 64) tl <<= 1;
  return tl;
}
// workgroups of nt threads whose teams of tl lanes take n rows, at most `cap`: the rows beyond are strided over
inline unsigned team_wgs(int64_t n, int tl, int nt, int64_t cap) {
  const int64_t per_wg = nt / tl;
  const int64_t wgs = (n + per_wg - 1) / per_wg;
  return (unsigned)(wgs > cap ? cap : wgs);
}

// ---- four columns of a row -----------------------------------------------------------------------------------------------------------
// four columns c .. c + 3 of a row as fp32; those at or above E read nothing and are zero
template <typename S> __device__ __forceinline__ void q_load4(const S* row, int c, int E, bool vec, float (&v)[4]);
template <> __device__ __forceinline__ void q_load4<float>(const float* row, int c, int E, bool vec, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (vec && c + 4 <= E) {
    const float4 a = *reinterpret_cast<const float4*>(row + c);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c + i < E) v[i] = row[c + i];
}
template <> __device__ __forceinline__ void q_load4<bf16_t>(const bf16_t* row, int c, int E, bool vec, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (vec && c + 4 <= E) {
    const uint2 a = *reinterpret_cast<const uint2*>(row + c);
    v[0] = __uint_as_float(a.x << 16); v[1] = __uint_as_float(a.x & 0xffff0000u);
    v[2] = __uint_as_float(a.y << 16); v[3] = __uint_as_float(a.y & 0xffff0000u);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c + i < E) v[i] = bf2f(row[c + i]);
}
// the columns below E of c .. c + 3 of an fp32 row
__device__ __forceinline__ void q_store4(float* row, int c, int E, bool vec, const float (&v)[4]) {
  if (vec && c + 4 <= E) {
    *reinterpret_cast<float4*>(row + c) = make_float4(v[0], v[1], v[2], v[3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c + i < E) row[c + i] = v[i];
}

// ---- one 16-byte piece ---------------------------------------------------------------------------------------------------------------
// PER columns c .. c + PER - 1 (4 or 8) of a codeword row; those at or above E read nothing and are zero
template <int PER> __device__ __forceinline__ void q_load_code(const float* row, int c, int E, bool vec, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (vec && c + PER <= E) {
    const float4 a = *reinterpret_cast<const float4*>(row + c);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    if (PER == 8) {
      const float4 b = *reinterpret_cast<const float4*>(row + c + 4);
      v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (c + i < E) v[i] = row[c + i];
}
// one whole 16-byte piece of an operand of T (4 or 8 columns of v)
template <typename T> __device__ __forceinline__ void q_store_piece(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void q_store_piece<float>(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void q_store_piece<bf16_t>(bf16_t* p, const float (&v)[8]) { store8<bf16_t>(p, v); }

// ---- the hash of the device draws (zs_vq_restart, zs_rvq_drop_draw): splitmix64's finaliser -------------------------------------------
__device__ __forceinline__ uint64_t q_mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

}  // namespace

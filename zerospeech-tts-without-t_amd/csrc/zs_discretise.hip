// zs_discretise.hip -- the encoder discretisers other than MBV (model/model.py:93-110, 457-472): Gumbel-softmax
// straight-through for enc_mode 'one_hot' (one softmax group of E per row) and 'binary' (E groups of E per row, summed
// over the groups and clamped to [0, 1]), and leaky_relu for 'continues'.  The MBV discretiser stays in zs_elem.hip.
//
// Work mapping.  A row of the encoder output is one (sample, frame).  Its softmax groups need a max and a sum over the
// group, so the softmax modes run ONE WAVE PER ROW (4 waves per 256-thread block, grid-stride over rows):
//  - one_hot: the group is the whole row of E (2 .. 1024).  Lane l holds columns l, l + 64, ... (NPL = ceil(E/64), a power
//    of two chosen on the host, so the per-lane values stay in registers with no dynamic indexing); the max, the sum and
//    the first-index argmax are 64-lane butterflies (__shfl_xor, width 64).  A group wider than 64 columns is just more
//    registers per lane, the reduction is the same.
//  - binary: E <= 64, so one group fits one wave with lane j holding column j of every group.  The wave walks the E groups
//    of its row in increasing i; each group's loads are E contiguous floats (coalesced) and lane j accumulates
//    s_j = sum_i out_{i,j} in its own register -- in increasing i as the reference's .sum(2) does, with no cross-lane
//    traffic.  (The values summed are exactly 0.0 or 1.0 -- (hard - y) + y rounds to the hard value -- so s_j is exact.)
//  The alternative, one lane per group, would make lane i read a stride-E column walk of its own and still need a
//  cross-lane sum for s_j.  Lanes past E idle for small E; these kernels touch rows x n_lin floats, small beside the step.
//  - continues: elementwise, one thread per (row, column), as the MBV kernel.
// Nothing here allocates or synchronises: the kernels are captured inside the train_ae step's hipGraph, and the noise
// seed can come from device memory (seed_ptr) so that every replay draws new noise.
#include <math.h>

#include "zs_common.h"

namespace {

constexpr int WPB = 4;                          // waves per block
constexpr uint32_t GUMBEL_TAG = 0x67756d00u;    // RNG stream of these kernels ("gum"); MBV draws from 0x6d627600

template <typename T> __device__ __forceinline__ float ldT(const void* p, int64_t i) { return Elem<T>::ld((const T*)p + i); }
template <typename T> __device__ __forceinline__ void stT(void* p, int64_t i, float v) { Elem<T>::st((T*)p + i, v); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// argmax over the wave: the larger value wins, equal values -> the smaller column (torch's first index on ties)
__device__ __forceinline__ int wave_argmax(float v, int idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  return idx;
}

template <typename T> __device__ __forceinline__ float ld_logit(const ZsGumbelStFwd& p, int64_t i) {
  return p.logits_f32 ? ((const float*)p.logits)[i] : ldT<T>(p.logits, i);
}

__device__ __forceinline__ float gumbel_noise(const ZsGumbelStFwd& p, uint64_t seed, int64_t ni) {
  if (p.noise_kind == 0) return p.noise[ni];
  const float u = p.noise_kind == 1 ? p.noise[ni] : zs_uniform(seed, GUMBEL_TAG, (uint64_t)ni);
  return -logf(-logf(u + 1e-20f) + 1e-20f);                     // model/model.py:95-98
}

template <typename T, int NPL>
__global__ __launch_bounds__(64 * WPB) void gumbel_st_fwd_kernel(const ZsGumbelStFwd p) {
  const int lane = threadIdx.x & 63;
  const int E = p.E;
  const bool binary = p.mode == ZS_ENC_BINARY;
  const int groups = binary ? E : 1;
  const int64_t n_lin = (int64_t)groups * E;
  const uint64_t seed = p.seed + (p.seed_ptr ? *p.seed_ptr : 0ull);
  for (int64_t r = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); r < p.rows; r += (int64_t)gridDim.x * WPB) {
    float s[NPL];                                               // one_hot: out_j; binary: s_j = sum_i out_{i,j}
#pragma unroll
    for (int k = 0; k < NPL; ++k) s[k] = 0.f;
    for (int i = 0; i < groups; ++i) {
      const int64_t nb = r * n_lin + (int64_t)i * E;            // noise / y index of column (i, 0)
      const int64_t lb = r * p.ld + (int64_t)i * E;
      float v[NPL];
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        const int j = lane + 64 * k;
        v[k] = -INFINITY;
        if (j < E) {
          v[k] = __fdiv_rn(__fadd_rn(ld_logit<T>(p, lb + j), gumbel_noise(p, seed, nb + j)), p.tau);   // (l + g) / tau
          mx = fmaxf(mx, v[k]);
        }
      }
      mx = wave_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < NPL; ++k)
        if (lane + 64 * k < E) { v[k] = expf(v[k] - mx); sum += v[k]; }
      sum = wave_sum(sum);
      float best = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < NPL; ++k)
        if (lane + 64 * k < E) {
          v[k] = __fdiv_rn(v[k], sum);                          // y = softmax(a)
          if (v[k] > best) { best = v[k]; bi = lane + 64 * k; }
        }
      bi = wave_argmax(best, bi);
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        const int j = lane + 64 * k;
        if (j < E) {
          const float hard = (j == bi) ? 1.f : 0.f;
          s[k] = __fadd_rn(s[k], __fadd_rn(__fsub_rn(hard, v[k]), v[k]));      // (y_hard - y).detach() + y
          if (p.y) p.y[nb + j] = v[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int j = lane + 64 * k;
      const float enc = binary ? fminf(fmaxf(s[k], 0.f), 1.f) : s[k];          // torch.clamp(min=0, max=1)
      if (j < E) {
        if (p.bits_f32) p.bits_f32[r * E + j] = enc;
        if (binary && p.s) p.s[r * E + j] = s[k];
      }
      if (p.bits && j < p.bits_fill_cols) stT<T>(p.bits, r * p.ld_bits + j, j < E ? enc : 0.f);
    }
    if (p.bits)
      for (int c = lane + 64 * NPL; c < p.bits_fill_cols; c += 64) stT<T>(p.bits, r * p.ld_bits + c, 0.f);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void continues_fwd_kernel(const ZsGumbelStFwd p) {
  const int64_t total = p.rows * p.bits_fill_cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / p.bits_fill_cols;
    const int e = (int)(i - r * p.bits_fill_cols);
    float v = 0.f;
    if (e < p.E) {
      const float l = ld_logit<T>(p, r * p.ld + e);
      v = l > 0.f ? l : l * p.slope;                            // F.leaky_relu(out, ns), model/model.py:458-459
      if (p.bits_f32) p.bits_f32[r * p.E + e] = v;
    }
    if (p.bits) stT<T>(p.bits, r * p.ld_bits + e, v);
  }
}

template <typename T, int NPL>
__global__ __launch_bounds__(64 * WPB) void gumbel_st_bwd_kernel(const ZsGumbelStBwd p) {
  const int lane = threadIdx.x & 63;
  const int E = p.E;
  const bool binary = p.mode == ZS_ENC_BINARY;
  const int groups = binary ? E : 1;
  const int64_t n_lin = (int64_t)groups * E;
  for (int64_t r = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); r < p.rows; r += (int64_t)gridDim.x * WPB) {
    float g[NPL];                                               // gradient w.r.t. out_{i,j}: the same for every group i
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int j = lane + 64 * k;
      g[k] = 0.f;
      if (j < E) {
        g[k] = ldT<T>(p.dbits, r * p.ld_dbits + j);
        if (binary) {
          const float s = p.s[r * E + j];
          if (!(s >= 0.f && s <= 1.f)) g[k] = 0.f;            // clamp backward: the inclusive mask of torch.clamp
        }
      }
    }
    for (int i = 0; i < groups; ++i) {
      const int64_t yb = r * p.ld_y + (int64_t)i * E;
      float y[NPL];
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        y[k] = lane + 64 * k < E ? p.y[yb + lane + 64 * k] : 0.f;
        dot += g[k] * y[k];
      }
      dot = wave_sum(dot);
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        const int j = lane + 64 * k;
        if (j < E) stT<T>(p.dlogits, r * p.ld + (int64_t)i * E + j, __fdiv_rn(y[k] * (g[k] - dot), p.tau));   // softmax bwd, / tau
      }
    }
    for (int64_t c = n_lin + lane; c < p.fill_cols; c += 64) stT<T>(p.dlogits, r * p.ld + c, 0.f);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void continues_bwd_kernel(const ZsGumbelStBwd p) {
  const int64_t total = p.rows * p.fill_cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / p.fill_cols;
    const int e = (int)(i - r * p.fill_cols);
    float v = 0.f;
    if (e < p.E) {
      const float d = ldT<T>(p.dbits, r * p.ld_dbits + e);
      v = p.y[r * p.ld_y + e] > 0.f ? d : d * p.slope;
    }
    stT<T>(p.dlogits, r * p.ld + e, v);
  }
}

inline unsigned row_blocks(int64_t rows) {
  int64_t b = (rows + WPB - 1) / WPB;
  return (unsigned)(b > 4096 ? 4096 : b);
}

inline unsigned elem_blocks(int64_t total) {
  int64_t b = (total + 255) / 256;
  if (b > 2048) b = 2048;
  return (unsigned)(b < 1 ? 1 : b);
}

inline int npl_for(int E) {
  int n = 1;
  while (64 * n < E) n *= 2;
  return n;
}

#define ZS_NPL_LAUNCH(KERNEL, T, npl, grid, stream, arg)                                                              \
  switch (npl) {                                                                                                      \
    case 1: hipLaunchKernelGGL((KERNEL<T, 1>), grid, dim3(64 * WPB), 0, (hipStream_t)(stream), arg); break;           \
    case 2: hipLaunchKernelGGL((KERNEL<T, 2>), grid, dim3(64 * WPB), 0, (hipStream_t)(stream), arg); break;           \
    case 4: hipLaunchKernelGGL((KERNEL<T, 4>), grid, dim3(64 * WPB), 0, (hipStream_t)(stream), arg); break;           \
    case 8: hipLaunchKernelGGL((KERNEL<T, 8>), grid, dim3(64 * WPB), 0, (hipStream_t)(stream), arg); break;           \
    default: hipLaunchKernelGGL((KERNEL<T, 16>), grid, dim3(64 * WPB), 0, (hipStream_t)(stream), arg); break;         \
  }

int check_mode(int32_t mode, int32_t E, const char* what) {
  ZS_REQUIRE(mode == ZS_ENC_ONE_HOT || mode == ZS_ENC_BINARY || mode == ZS_ENC_CONTINUES, "%s: bad mode %d", what, mode);
  ZS_REQUIRE(E >= 2, "%s: E must be >= 2", what);
  ZS_REQUIRE(mode != ZS_ENC_ONE_HOT || E <= 1024, "%s: one_hot supports E <= 1024 (got %d)", what, E);
  ZS_REQUIRE(mode != ZS_ENC_BINARY || E <= 64, "%s: binary supports E <= 64 (got %d)", what, E);
  return ZS_OK;
}

}  // namespace

extern "C" int zs_gumbel_st_fwd(const ZsGumbelStFwd* p, void* stream) {
  ZS_REQUIRE(p && p->logits && p->rows > 0, "zs_gumbel_st_fwd: bad args");
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_gumbel_st_fwd: bad dtype");
  int rc = check_mode(p->mode, p->E, "zs_gumbel_st_fwd");
  if (rc) return rc;
  const int64_t n_lin = p->mode == ZS_ENC_BINARY ? (int64_t)p->E * p->E : p->E;
  ZS_REQUIRE(p->ld >= n_lin, "zs_gumbel_st_fwd: ld %lld < %lld logit columns", (long long)p->ld, (long long)n_lin);
  ZS_REQUIRE(p->bits || p->bits_f32, "zs_gumbel_st_fwd: no output");
  ZsGumbelStFwd q = *p;
  if (!q.bits || q.bits_fill_cols < q.E) q.bits_fill_cols = q.E;
  ZS_REQUIRE(!q.bits || q.ld_bits >= q.bits_fill_cols, "zs_gumbel_st_fwd: ld_bits < bits_fill_cols");
  if (p->mode == ZS_ENC_CONTINUES) {
    ZS_REQUIRE(!p->noise, "zs_gumbel_st_fwd: continues takes no noise");
    const unsigned nb = elem_blocks(q.rows * q.bits_fill_cols);
    if (p->dtype == ZS_F32) hipLaunchKernelGGL(continues_fwd_kernel<float>, dim3(nb), dim3(256), 0, (hipStream_t)stream, q);
    else hipLaunchKernelGGL(continues_fwd_kernel<bf16_t>, dim3(nb), dim3(256), 0, (hipStream_t)stream, q);
    return zs_check_launch("zs_gumbel_st_fwd");
  }
  ZS_REQUIRE(p->tau > 0.f, "zs_gumbel_st_fwd: tau must be > 0");
  ZS_REQUIRE(p->noise_kind >= 0 && p->noise_kind <= 2, "zs_gumbel_st_fwd: bad noise_kind");
  ZS_REQUIRE(p->noise_kind == 2 || p->noise, "zs_gumbel_st_fwd: noise missing");
  const int npl = npl_for(p->E);
  const dim3 grid(row_blocks(q.rows));
  if (p->dtype == ZS_F32) { ZS_NPL_LAUNCH(gumbel_st_fwd_kernel, float, npl, grid, stream, q) }
  else { ZS_NPL_LAUNCH(gumbel_st_fwd_kernel, bf16_t, npl, grid, stream, q) }
  return zs_check_launch("zs_gumbel_st_fwd");
}

extern "C" int zs_gumbel_st_bwd(const ZsGumbelStBwd* p, void* stream) {
  ZS_REQUIRE(p && p->dbits && p->y && p->dlogits && p->rows > 0, "zs_gumbel_st_bwd: bad args");
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_gumbel_st_bwd: bad dtype");
  int rc = check_mode(p->mode, p->E, "zs_gumbel_st_bwd");
  if (rc) return rc;
  const int64_t n_lin = p->mode == ZS_ENC_BINARY ? (int64_t)p->E * p->E : p->E;
  ZS_REQUIRE(p->fill_cols >= n_lin && p->ld >= p->fill_cols, "zs_gumbel_st_bwd: need n_lin <= fill_cols <= ld");
  ZS_REQUIRE(p->ld_y >= n_lin, "zs_gumbel_st_bwd: ld_y < n_lin");
  ZS_REQUIRE(p->mode != ZS_ENC_BINARY || p->s, "zs_gumbel_st_bwd: binary needs s");
  if (p->mode == ZS_ENC_CONTINUES) {
    const unsigned nb = elem_blocks(p->rows * p->fill_cols);
    if (p->dtype == ZS_F32) hipLaunchKernelGGL(continues_bwd_kernel<float>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(continues_bwd_kernel<bf16_t>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p);
    return zs_check_launch("zs_gumbel_st_bwd");
  }
  ZS_REQUIRE(p->tau > 0.f, "zs_gumbel_st_bwd: tau must be > 0");
  const int npl = npl_for(p->E);
  const dim3 grid(row_blocks(p->rows));
  if (p->dtype == ZS_F32) { ZS_NPL_LAUNCH(gumbel_st_bwd_kernel, float, npl, grid, stream, *p) }
  else { ZS_NPL_LAUNCH(gumbel_st_bwd_kernel, bf16_t, npl, grid, stream, *p) }
  return zs_check_launch("zs_gumbel_st_bwd");
}

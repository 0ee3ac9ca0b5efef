// zs_rvq_drop.hip -- quantiser dropout for training through the residual codebook (include/zs_amd_rvq_drop.h): the stage
// count of every sample drawn on the device (zs_rvq_drop_draw), zs_rvq_commit where only the rows of samples that still use the stage
// take part (zs_rvq_commit_drop) and zs_rvq_gather with a stage count per fragment (zs_rvq_gather_frag).  All three are memory-bound;
// the search, the sums, the average, the restart, the loss and the backward are the unchanged entry points.  Nothing here adds floats
// atomically, so a step is bitwise reproducible.
//   rvq_drop_draw_kernel     one workgroup: lane t draws the samples t, t + 256, ..; the S integer counts go through the waves' shuffles.
//   rvq_commit_drop_kernel   rvq_commit_kernel's layout and operation order (zs_rvq_train.hip).  Whether a row takes part is a property
//                            of its fragment, so of the whole team: the trip counts and the shuffles do not depend on it.
//   rvq_gather_frag_kernel   rvq_gather_kernel's layout (zs_rvq.hip): one lane per 16-byte piece; a fragment's count is read once per
//                            fragment and is the same for every lane of the workgroup.
#include "zs_common.h"
#include "../../include/zs_amd_rvq_drop.h"

// the definitions are stated operation by operation (a rounding each): nothing in this file may be fused into a multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int RD_NT = 256;

// four columns c .. c + 3 of a row as fp32; those at or above E read nothing and are zero
template <typename S> __device__ __forceinline__ void rd_load4(const S* row, int c, int E, bool vec, float (&v)[4]);
template <> __device__ __forceinline__ void rd_load4<float>(const float* row, int c, int E, bool vec, float (&v)[4]) {
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
template <> __device__ __forceinline__ void rd_load4<bf16_t>(const bf16_t* row, int c, int E, bool vec, float (&v)[4]) {
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
__device__ __forceinline__ void rd_store4(float* row, int c, int E, bool vec, const float (&v)[4]) {
  if (vec && c + 4 <= E) {
    *reinterpret_cast<float4*>(row + c) = make_float4(v[0], v[1], v[2], v[3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c + i < E) row[c + i] = v[i];
}

struct RdVec { int x, code, r, xf, a; };                          // which operands take 16-byte (x bf16: 8-byte) accesses

// ---- draw --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rd_mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__global__ void __launch_bounds__(RD_NT) rvq_drop_draw_kernel(const ZsRvqDropDraw p) {
  __shared__ int s_cnt[RD_NT / 64][ZS_RVQ_MAX_S];
  const int tid = threadIdx.x;
  const uint64_t base = p.seed + (p.seed_ptr ? *p.seed_ptr : 0ull) + (uint64_t)ZS_RVQ_DROP_SALT;
  int cnt[ZS_RVQ_MAX_S];
#pragma unroll
  for (int s = 0; s < ZS_RVQ_MAX_S; ++s) cnt[s] = 0;
  for (int b = tid; b < p.n_frag; b += RD_NT) {
    const uint64_t u = rd_mix64(base + (uint64_t)b * 0x9E3779B97F4A7C15ull);
    const bool drop = (u >> 40) < (uint64_t)p.thr;
    const int su = drop ? 1 + (int)((u & 0xFFFFFFFFull) % (uint64_t)p.S) : p.S;
    p.s_use[b] = su;
#pragma unroll
    for (int s = 0; s < ZS_RVQ_MAX_S; ++s) cnt[s] += su > s;
  }
#pragma unroll
  for (int s = 0; s < ZS_RVQ_MAX_S; ++s) {                         // every lane of every wave: whole waves at the shuffles
    int v = cnt[s];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6][s] = v;
  }
  __syncthreads();
  if (tid < p.S) p.active[tid] = p.rows_per_frag * (((s_cnt[0][tid] + s_cnt[1][tid]) + s_cnt[2][tid]) + s_cnt[3][tid]);
}

// ---- commit ------------------------------------------------------------------------------------------------------------------------
template <typename S> __global__ void __launch_bounds__(RD_NT)
rvq_commit_drop_kernel(const ZsRvqCommitDrop p, const int tl, const int groups, const RdVec vec) {
  __shared__ double s_part[RD_NT / 64];
  const int tid = threadIdx.x, tlane = tid & (tl - 1);
  const int64_t n_teams = (int64_t)gridDim.x * (RD_NT / tl);
  const int64_t team = (int64_t)blockIdx.x * (RD_NT / tl) + tid / tl;
  const int64_t rounds = (p.n + n_teams - 1) / n_teams;            // the same for every lane: the shuffles below see whole waves
  const S* x = static_cast<const S*>(p.x);
  double acc = 0.0;
  int bad = 0, over = 0;
  for (int64_t rd = 0; rd < rounds; ++rd) {
    const int64_t row = team + rd * n_teams;
    const bool live = row < p.n;
    // the fragment's count decides for the whole team (a row has one fragment): the loop below has the team's trip count either way
    const bool act = live && p.stage < p.s_use[(int)row / p.rows_per_frag];
    const int k = act ? p.idx[row] : 0;
    const bool ok = act && k >= 0 && k < p.K;                       // else never an index: the row passes unsubtracted
    int big = 0;
    if (live) {
      const S* xr = x + row * p.ld_x;
      const float* cr = p.code + (int64_t)(ok ? k : 0) * p.ld_code;
      float* rr = p.r + row * p.ld_r;
      float* ar = p.a + row * p.ld_a;
      for (int g = tlane; g < groups; g += tl) {
        const int c = 4 * g;
        float xv[4], rv[4], av[4] = {0.f, 0.f, 0.f, 0.f};
        rd_load4<S>(xr, c, p.E, vec.x != 0, xv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          big |= act && !(fabsf(xv[j]) < (float)ZS_VQ_MAX_ABS);     // (NaN: not below; the columns at or above E are zero)
          rv[j] = xv[j];
        }
        if (ok) {
          float cv[4];
          rd_load4<float>(cr, c, p.E, vec.code != 0, cv);
          if (!p.first) rd_load4<float>(ar, c, p.E, vec.a != 0, av);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            rv[j] = xv[j] - cv[j];                                  // one IEEE subtraction
            if (c + j < p.E) acc += (double)rv[j] * (double)rv[j];  // the stored value
            av[j] = p.first ? rv[j] : av[j] + rv[j];                // one fp32 add
          }
        }
        rd_store4(rr, c, p.E, vec.r != 0, rv);                      // (a row that takes no part: the fp32 value of x)
        if (p.x_f32) rd_store4(p.x_f32 + row * p.ld_xf, c, p.E, vec.xf != 0, xv);
        if (ok || (act && p.first)) rd_store4(ar, c, p.E, vec.a != 0, av);   // (a bad row: zero at the first stage, as it is behind it)
      }
    }
    for (int o = 1; o < tl; o <<= 1) big |= __shfl_xor(big, o, 64);  // over the team; every lane of the wave is here
    if (live && tlane == 0) {
      bad += act && !ok;
      over += big;
      p.idx_acc[row] = (ok && !big) ? k : -1;
    }
  }
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) s_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) p.partial[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
  if (blockIdx.x == 0)
    for (int w = (int)gridDim.x + tid; w < ZS_VQ_COMMIT_PARTS; w += RD_NT) p.partial[w] = 0.0;
  if (bad) atomicAdd(p.bad, bad);
  if (over) atomicAdd(p.over, over);
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void rd_store_piece(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void rd_store_piece<float>(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void rd_store_piece<bf16_t>(bf16_t* p, const float (&v)[8]) { store8<bf16_t>(p, v); }

// PER columns c .. c + PER - 1 of a codeword row; those at or above E read nothing and are zero
template <int PER> __device__ __forceinline__ void rd_load_code(const float* row, int c, int E, bool vec, float (&v)[8]) {
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

template <typename T> __global__ void __launch_bounds__(RD_NT) rvq_gather_frag_kernel(const ZsRvqGatherFrag p, const int cvec) {
  constexpr int PER = 16 / (int)sizeof(T);                        // columns of a 16-byte piece
  const int groups = (int)(p.ld_dst / PER);
  const int64_t per_frag = (int64_t)p.T * groups;
  const int64_t tid = (int64_t)blockIdx.x * RD_NT + threadIdx.x, nthr = (int64_t)gridDim.x * RD_NT;
  int bad = 0;
  for (int64_t f = blockIdx.y; f < p.n_frag; f += gridDim.y) {
    const int64_t start = p.start[f];
    const int len = p.len[f];
    const int su = p.s_use[f];
    const bool ok = len >= 0 && len <= p.T && start >= 0 && start <= p.n_idx - len;          // else: a zero fragment, nothing read
    const bool counted = su >= 1 && su <= p.S;                      // else: zero rows, a bad frame each, no index read
    T* dst = static_cast<T*>(p.dst) + f * p.T * p.ld_dst;
    for (int64_t i = tid; i < per_frag; i += nthr) {
      const int t = (int)(i / groups), g = (int)(i - (int64_t)t * groups);
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (ok && t < len) {
        int k[ZS_RVQ_MAX_S];
        bool in = counted;
#pragma unroll
        for (int s = 0; s < ZS_RVQ_MAX_S; ++s) {
          k[s] = (counted && s < su) ? p.idx[(int64_t)s * p.ld_idx + start + t] : 0;
          in = in && k[s] >= 0 && k[s] < p.K;
        }
        if (!in) {
          bad += g == 0;                                          // once per row, however many of its indices are out of range
        } else if (PER * g < p.E) {
          rd_load_code<PER>(p.code + (int64_t)k[0] * p.ld_code, PER * g, p.E, cvec != 0, v);
#pragma unroll
          for (int s = 1; s < ZS_RVQ_MAX_S; ++s)
            if (s < su) {
              float w[8];
              rd_load_code<PER>(p.code + (int64_t)s * p.plane_code + (int64_t)k[s] * p.ld_code, PER * g, p.E, cvec != 0, w);
#pragma unroll
              for (int j = 0; j < PER; ++j) v[j] = v[j] + w[j];   // in increasing stage, a rounding each
            }
        }
      }
      rd_store_piece<T>(dst + (int64_t)t * p.ld_dst + PER * g, v);
    }
  }
  if (bad) atomicAdd(p.bad, bad);
}

inline bool misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

}  // namespace

extern "C" int zs_rvq_drop_draw(const ZsRvqDropDraw* p, void* stream) {
  ZS_REQUIRE(p, "zs_rvq_drop_draw: null argument");
  ZS_REQUIRE(p->S >= 1 && p->S <= ZS_RVQ_MAX_S, "zs_rvq_drop_draw: S must be in [1, %d] (got %d)", ZS_RVQ_MAX_S, p->S);
  ZS_REQUIRE(p->thr >= 1 && p->thr <= ZS_RVQ_DROP_THR_ONE, "zs_rvq_drop_draw: thr must be in [1, %d] (got %d)", ZS_RVQ_DROP_THR_ONE, p->thr);
  ZS_REQUIRE(p->n_frag >= 1 && p->n_frag <= ZS_UNITS_MAX_FRAG && p->rows_per_frag >= 1 &&
                 (int64_t)p->n_frag * p->rows_per_frag <= 0x7fffffff,
             "zs_rvq_drop_draw: n_frag must be in [1, %d], rows_per_frag >= 1 and their product below 2^31 (got %d, %d)", ZS_UNITS_MAX_FRAG,
             p->n_frag, p->rows_per_frag);
  ZS_REQUIRE(p->s_use && p->active, "zs_rvq_drop_draw: null operand");
  ZS_REQUIRE(!misaligned(p->s_use, 4) && !misaligned(p->active, 4) && !misaligned(p->seed_ptr, 8),
             "zs_rvq_drop_draw: an operand is not aligned to its element");
  hipLaunchKernelGGL(rvq_drop_draw_kernel, dim3(1), dim3(RD_NT), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_rvq_drop_draw");
}

extern "C" int zs_rvq_commit_drop(const ZsRvqCommitDrop* p, void* stream) {
  ZS_REQUIRE(p, "zs_rvq_commit_drop: null argument");
  const char* why = nullptr;
  if (p->E < 1 || p->E > ZS_CODE_MAX_E) why = "E must be in [1, 1024]";
  if (!why && (p->n < 0 || p->n > 0x7fffffff)) why = "n must be in [0, 2^31)";
  if (!why && (p->K < 1 || p->K > ZS_CODE_MAX_K)) why = "K must be in [1, 65536]";
  if (!why && (p->ld_x < p->E || p->ld_code < p->E || p->ld_r < p->E || p->ld_a < p->E || (p->x_f32 && p->ld_xf < p->E)))
    why = "a leading dimension is below E";
  ZS_REQUIRE(!why, "zs_rvq_commit_drop: %s (n %lld, K %d, E %d, ld_x %lld, ld_code %lld, ld_r %lld, ld_xf %lld, ld_a %lld)", why,
             (long long)p->n, p->K, p->E, (long long)p->ld_x, (long long)p->ld_code, (long long)p->ld_r, (long long)p->ld_xf, (long long)p->ld_a);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_rvq_commit_drop: bad dtype");
  ZS_REQUIRE(p->rows_per_frag >= 1 && p->stage >= 0 && p->stage < ZS_RVQ_MAX_S && (p->first != 0) == (p->stage == 0),
             "zs_rvq_commit_drop: rows_per_frag must be >= 1, stage in [0, %d) and first set at stage 0 alone (got %d, stage %d, first %d)",
             ZS_RVQ_MAX_S, p->rows_per_frag, p->stage, p->first);
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->x && p->idx && p->code && p->r && p->idx_acc && p->a && p->partial && p->bad && p->over && p->s_use,
             "zs_rvq_commit_drop: null operand");
  const bool f32 = p->src_f32 || p->dtype == ZS_F32;
  ZS_REQUIRE(!misaligned(p->x, f32 ? 4 : 2) && !misaligned(p->idx, 4) && !misaligned(p->code, 4) && !misaligned(p->r, 4) &&
                 !misaligned(p->x_f32, 4) && !misaligned(p->idx_acc, 4) && !misaligned(p->a, 4) && !misaligned(p->partial, 8) &&
                 !misaligned(p->bad, 4) && !misaligned(p->over, 4) && !misaligned(p->s_use, 4),
             "zs_rvq_commit_drop: an operand is not aligned to its element");
  const void* xv = p->x;
  ZS_REQUIRE(p->r != xv && p->a != xv && p->x_f32 != xv && p->r != p->a && p->r != p->x_f32 && p->a != p->x_f32,
             "zs_rvq_commit_drop: r, x_f32 and a must not be x or each other");
  ZS_REQUIRE(p->idx_acc != p->idx && p->idx_acc != p->s_use, "zs_rvq_commit_drop: idx_acc must not be idx or s_use");
  RdVec vec;
  vec.x = !misaligned(p->x, f32 ? 16 : 8) && p->ld_x % 4 == 0;
  vec.code = !misaligned(p->code, 16) && p->ld_code % 4 == 0;
  vec.r = !misaligned(p->r, 16) && p->ld_r % 4 == 0;
  vec.xf = p->x_f32 && !misaligned(p->x_f32, 16) && p->ld_xf % 4 == 0;
  vec.a = !misaligned(p->a, 16) && p->ld_a % 4 == 0;
  const int groups = (p->E + 3) / 4;
  int tl = 1;
  while (tl < groups && tl < 64) tl <<= 1;
  const int64_t per_wg = RD_NT / tl;
  int64_t wgs = (p->n + per_wg - 1) / per_wg;
  wgs = wgs > ZS_VQ_COMMIT_PARTS ? ZS_VQ_COMMIT_PARTS : wgs;       // the rows beyond are strided over
  const hipStream_t st = (hipStream_t)stream;
  if (f32)
    hipLaunchKernelGGL(rvq_commit_drop_kernel<float>, dim3((unsigned)wgs), dim3(RD_NT), 0, st, *p, tl, groups, vec);
  else
    hipLaunchKernelGGL(rvq_commit_drop_kernel<bf16_t>, dim3((unsigned)wgs), dim3(RD_NT), 0, st, *p, tl, groups, vec);
  return zs_check_launch("zs_rvq_commit_drop");
}

extern "C" int zs_rvq_gather_frag(const ZsRvqGatherFrag* p, void* stream) {
  ZS_REQUIRE(p, "zs_rvq_gather_frag: null argument");
  ZS_REQUIRE(p->n_frag >= 0 && p->n_frag <= ZS_UNITS_MAX_FRAG, "zs_rvq_gather_frag: n_frag must be in [0, %d] (got %d)", ZS_UNITS_MAX_FRAG,
             p->n_frag);
  const char* why = nullptr;
  if (p->K < 1 || p->K > ZS_CODE_MAX_K) why = "K must be in [1, 65536]";
  else if (p->E < 1 || p->E > ZS_CODE_MAX_E) why = "E must be in [1, 1024]";
  else if (p->n_idx < 0 || p->n_idx > 0x7fffffff) why = "n must be in [0, 2^31)";
  else if (p->ld_dst < p->E || p->ld_code < p->E) why = "a leading dimension is below E";
  ZS_REQUIRE(!why, "zs_rvq_gather_frag: %s (n_idx %lld, K %d, E %d, ld_dst %lld, ld_code %lld)", why, (long long)p->n_idx, p->K, p->E,
             (long long)p->ld_dst, (long long)p->ld_code);
  ZS_REQUIRE(p->S >= 1 && p->S <= ZS_RVQ_MAX_S, "zs_rvq_gather_frag: S must be in [1, %d] (got %d)", ZS_RVQ_MAX_S, p->S);
  ZS_REQUIRE(p->ld_idx >= p->n_idx, "zs_rvq_gather_frag: the index planes are ld_idx = %lld apart and hold n_idx = %lld entries",
             (long long)p->ld_idx, (long long)p->n_idx);
  ZS_REQUIRE(p->plane_code >= (int64_t)(p->K - 1) * p->ld_code + p->E,
             "zs_rvq_gather_frag: the codebooks are plane_code = %lld apart, K = %d rows of ld_code = %lld need %lld", (long long)p->plane_code,
             p->K, (long long)p->ld_code, (long long)((int64_t)(p->K - 1) * p->ld_code + p->E));
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_rvq_gather_frag: bad dtype");
  ZS_REQUIRE(p->T > 0 && p->ld_dst % 8 == 0, "zs_rvq_gather_frag: T must be > 0 and ld_dst a multiple of 8");
  if (p->n_frag == 0) return ZS_OK;
  ZS_REQUIRE(p->dst && p->start && p->len && p->code && p->bad && p->s_use && (p->idx || p->n_idx == 0), "zs_rvq_gather_frag: null operand");
  ZS_REQUIRE(!misaligned(p->dst, 16) && !misaligned(p->code, 4) && !misaligned(p->idx, 4) && !misaligned(p->bad, 4) &&
                 !misaligned(p->start, 8) && !misaligned(p->len, 4) && !misaligned(p->s_use, 4),
             "zs_rvq_gather_frag: an operand is misaligned (dst: 16 bytes)");
  const int cvec = !misaligned(p->code, 16) && p->ld_code % 4 == 0 && p->plane_code % 4 == 0;
  const int per = p->dtype == ZS_F32 ? 4 : 8;
  int64_t bx = ((int64_t)p->T * (p->ld_dst / per) + RD_NT - 1) / RD_NT;
  bx = bx > 64 ? 64 : bx;
  const dim3 grid((unsigned)bx, (unsigned)(p->n_frag < 65535 ? p->n_frag : 65535));
  if (p->dtype == ZS_F32)
    hipLaunchKernelGGL(rvq_gather_frag_kernel<float>, grid, dim3(RD_NT), 0, (hipStream_t)stream, *p, cvec);
  else
    hipLaunchKernelGGL(rvq_gather_frag_kernel<bf16_t>, grid, dim3(RD_NT), 0, (hipStream_t)stream, *p, cvec);
  return zs_check_launch("zs_rvq_gather_frag");
}

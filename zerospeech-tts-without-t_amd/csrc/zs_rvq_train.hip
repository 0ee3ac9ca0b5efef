// zs_rvq_train.hip -- training a 'continues' model through its residual codebook (include/zs_amd.h): what a stage of the
// straight-through quantiser leaves over, with everything the step wants of it in the same pass (zs_rvq_commit), the commitment loss of
// the S stages from its partial sums (zs_rvq_loss) and the gradient (zs_rvq_st_bwd).  All three are memory-bound; the search, the
// fixed-point sums, the codebook's average and the restart of every stage are zs_vq_assign, zs_vq_accum, zs_vq_ema and zs_vq_restart,
// unchanged.  Nothing here adds floats atomically, so a step is bitwise reproducible.
//   rvq_commit_kernel   rvq_residual_kernel's layout: a row is owned by a team of 2^t <= 64 lanes of one wave, four columns per lane
//                       and round.  A lane reads its piece of x, of the one codeword row and (behind the first stage) of a, and
//                       writes its piece of r, of a and of the fp32 copy: every operand crosses the memory system once.  The row's
//                       magnitude check is an OR over the team by shuffles, as in vq_commit_kernel, and so is the tree of the doubles.
//   rvq_loss_kernel     one workgroup: the [S][ZS_VQ_COMMIT_PARTS] partials in a fixed order.
//   rvq_st_bwd_kernel   one lane per 16-byte piece of dz, grid-stride.
#include "zs_common.h"

// the definitions are stated operation by operation (a rounding each): nothing in this file may be fused into a multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int RT_NT = 256;

// four columns c .. c + 3 of a row as fp32; those at or above E read nothing and are zero
template <typename S> __device__ __forceinline__ void rt_load4(const S* row, int c, int E, bool vec, float (&v)[4]);
template <> __device__ __forceinline__ void rt_load4<float>(const float* row, int c, int E, bool vec, float (&v)[4]) {
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
template <> __device__ __forceinline__ void rt_load4<bf16_t>(const bf16_t* row, int c, int E, bool vec, float (&v)[4]) {
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
__device__ __forceinline__ void rt_store4(float* row, int c, int E, bool vec, const float (&v)[4]) {
  if (vec && c + 4 <= E) {
    *reinterpret_cast<float4*>(row + c) = make_float4(v[0], v[1], v[2], v[3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c + i < E) row[c + i] = v[i];
}

struct RtVec { int x, code, r, xf, a; };                          // which operands take 16-byte (x bf16: 8-byte) accesses

// ---- commit ------------------------------------------------------------------------------------------------------------------------
template <typename S> __global__ void __launch_bounds__(RT_NT)
rvq_commit_kernel(const ZsRvqCommit p, const int tl, const int groups, const RtVec vec) {
  __shared__ double s_part[RT_NT / 64];
  const int tid = threadIdx.x, tlane = tid & (tl - 1);
  const int64_t n_teams = (int64_t)gridDim.x * (RT_NT / tl);
  const int64_t team = (int64_t)blockIdx.x * (RT_NT / tl) + tid / tl;
  const int64_t rounds = (p.n + n_teams - 1) / n_teams;            // the same for every lane: the shuffles below see whole waves
  const S* x = static_cast<const S*>(p.x);
  double acc = 0.0;
  int bad = 0, over = 0;
  for (int64_t rd = 0; rd < rounds; ++rd) {
    const int64_t row = team + rd * n_teams;
    const bool live = row < p.n;
    const int k = live ? p.idx[row] : 0;
    const bool ok = live && k >= 0 && k < p.K;                      // else never an index: the row passes unsubtracted
    int big = 0;
    if (live) {
      const S* xr = x + row * p.ld_x;
      const float* cr = p.code + (int64_t)(ok ? k : 0) * p.ld_code;
      float* rr = p.r + row * p.ld_r;
      float* ar = p.a + row * p.ld_a;
      for (int g = tlane; g < groups; g += tl) {
        const int c = 4 * g;
        float xv[4], rv[4], av[4] = {0.f, 0.f, 0.f, 0.f};
        rt_load4<S>(xr, c, p.E, vec.x != 0, xv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          big |= !(fabsf(xv[j]) < (float)ZS_VQ_MAX_ABS);            // (NaN: not below; the columns at or above E are zero)
          rv[j] = xv[j];
        }
        if (ok) {
          float cv[4];
          rt_load4<float>(cr, c, p.E, vec.code != 0, cv);
          if (!p.first) rt_load4<float>(ar, c, p.E, vec.a != 0, av);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            rv[j] = xv[j] - cv[j];                                  // one IEEE subtraction
            if (c + j < p.E) acc += (double)rv[j] * (double)rv[j];  // the stored value
            av[j] = p.first ? rv[j] : av[j] + rv[j];                // one fp32 add
          }
        }
        rt_store4(rr, c, p.E, vec.r != 0, rv);
        if (p.x_f32) rt_store4(p.x_f32 + row * p.ld_xf, c, p.E, vec.xf != 0, xv);
        if (ok || p.first) rt_store4(ar, c, p.E, vec.a != 0, av);   // (a bad row: zero at the first stage, as it is behind it)
      }
    }
    for (int o = 1; o < tl; o <<= 1) big |= __shfl_xor(big, o, 64);  // over the team
    if (live && tlane == 0) {
      bad += !ok;
      over += big;
      p.idx_acc[row] = (ok && !big) ? k : -1;
    }
  }
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) s_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) p.partial[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
  if (blockIdx.x == 0)
    for (int w = (int)gridDim.x + tid; w < ZS_VQ_COMMIT_PARTS; w += RT_NT) p.partial[w] = 0.0;
  if (bad) atomicAdd(p.bad, bad);
  if (over) atomicAdd(p.over, over);
}

// ---- loss --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RT_NT) rvq_loss_kernel(const ZsRvqLoss p) {
  __shared__ double s_part[ZS_RVQ_MAX_S][RT_NT / 64];
  const int tid = threadIdx.x;
  for (int s = 0; s < p.S; ++s) {
    const double* part = p.partial + (int64_t)s * ZS_VQ_COMMIT_PARTS;
    double v = 0.0;
    for (int i = tid; i < ZS_VQ_COMMIT_PARTS; i += RT_NT) v += part[i];
    v = wave_sum_d(v);
    if ((tid & 63) == 0) s_part[s][tid >> 6] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int s = 0; s < p.S; ++s) {
      const double d = ((s_part[s][0] + s_part[s][1]) + s_part[s][2]) + s_part[s][3];
      p.loss[1 + s] = (float)(p.scale * d);
      total = s == 0 ? d : total + d;
    }
    p.loss[0] = (float)(p.scale * total);
  }
}

// ---- straight-through backward ---------------------------------------------------------------------------------------------------------
// one whole 16-byte piece of an operand of T (4 or 8 columns)
template <typename T> __device__ __forceinline__ void rt_load_piece(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void rt_load_piece<float>(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = v[5] = v[6] = v[7] = 0.f;
}
template <> __device__ __forceinline__ void rt_load_piece<bf16_t>(const bf16_t* p, float (&v)[8]) { load8<bf16_t>(p, v); }

template <typename T> __global__ void __launch_bounds__(RT_NT) rvq_st_bwd_kernel(const ZsRvqStBwd p, const int groups, const int avec) {
  constexpr int PER = 16 / (int)sizeof(T);
  const int64_t total = p.n * groups;
  const int64_t nthr = (int64_t)gridDim.x * RT_NT;
  const T* dq = static_cast<const T*>(p.dq);
  T* dz = static_cast<T*>(p.dz);
  for (int64_t i = (int64_t)blockIdx.x * RT_NT + threadIdx.x; i < total; i += nthr) {
    const int64_t row = i / groups;
    const int c = PER * (int)(i - row * groups);
    float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < p.E) {
      float dv[8], lo[4], hi[4] = {0.f, 0.f, 0.f, 0.f};
      rt_load_piece<T>(dq + row * p.ld_dq + c, dv);               // (dq is 16-byte aligned at a pitch of whole pieces)
      const float* ar = p.a + row * p.ld_a;
      rt_load4<float>(ar, c, p.E, avec != 0, lo);
      if (PER == 8) rt_load4<float>(ar, c + 4, p.E, avec != 0, hi);
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const float t = p.g * (j < 4 ? lo[j & 3] : hi[j & 3]);      // two fp32 operations, a rounding each (contract off)
        out[j] = c + j < p.E ? dv[j] + t : 0.f;
      }
    }
    if (PER == 4)
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(dz) + row * p.ld_dz + c) = make_float4(out[0], out[1], out[2], out[3]);
    else
      store8<T>(dz + row * p.ld_dz + c, out);
  }
}

inline bool misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

const char* rt_shape(int E, int64_t n) {
  if (E < 1 || E > ZS_CODE_MAX_E) return "E must be in [1, 1024]";
  if (n < 0 || n > 0x7fffffff) return "n must be in [0, 2^31)";
  return nullptr;
}

}  // namespace

extern "C" int zs_rvq_commit(const ZsRvqCommit* p, void* stream) {
  ZS_REQUIRE(p, "zs_rvq_commit: null argument");
  const char* why = rt_shape(p->E, p->n);
  if (!why && (p->K < 1 || p->K > ZS_CODE_MAX_K)) why = "K must be in [1, 65536]";
  if (!why && (p->ld_x < p->E || p->ld_code < p->E || p->ld_r < p->E || p->ld_a < p->E || (p->x_f32 && p->ld_xf < p->E)))
    why = "a leading dimension is below E";
  ZS_REQUIRE(!why, "zs_rvq_commit: %s (n %lld, K %d, E %d, ld_x %lld, ld_code %lld, ld_r %lld, ld_xf %lld, ld_a %lld)", why, (long long)p->n,
             p->K, p->E, (long long)p->ld_x, (long long)p->ld_code, (long long)p->ld_r, (long long)p->ld_xf, (long long)p->ld_a);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_rvq_commit: bad dtype");
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->x && p->idx && p->code && p->r && p->idx_acc && p->a && p->partial && p->bad && p->over, "zs_rvq_commit: null operand");
  const bool f32 = p->src_f32 || p->dtype == ZS_F32;
  ZS_REQUIRE(!misaligned(p->x, f32 ? 4 : 2) && !misaligned(p->idx, 4) && !misaligned(p->code, 4) && !misaligned(p->r, 4) &&
                 !misaligned(p->x_f32, 4) && !misaligned(p->idx_acc, 4) && !misaligned(p->a, 4) && !misaligned(p->partial, 8) &&
                 !misaligned(p->bad, 4) && !misaligned(p->over, 4), "zs_rvq_commit: an operand is not aligned to its element");
  const void* xv = p->x;
  ZS_REQUIRE(p->r != xv && p->a != xv && p->x_f32 != xv && p->r != p->a && p->r != p->x_f32 && p->a != p->x_f32,
             "zs_rvq_commit: r, x_f32 and a must not be x or each other");
  ZS_REQUIRE(p->idx_acc != p->idx, "zs_rvq_commit: idx_acc must not be idx");
  RtVec vec;
  vec.x = !misaligned(p->x, f32 ? 16 : 8) && p->ld_x % 4 == 0;
  vec.code = !misaligned(p->code, 16) && p->ld_code % 4 == 0;
  vec.r = !misaligned(p->r, 16) && p->ld_r % 4 == 0;
  vec.xf = p->x_f32 && !misaligned(p->x_f32, 16) && p->ld_xf % 4 == 0;
  vec.a = !misaligned(p->a, 16) && p->ld_a % 4 == 0;
  const int groups = (p->E + 3) / 4;
  int tl = 1;
  while (tl < groups && tl < 64) tl <<= 1;
  const int64_t per_wg = RT_NT / tl;
  int64_t wgs = (p->n + per_wg - 1) / per_wg;
  wgs = wgs > ZS_VQ_COMMIT_PARTS ? ZS_VQ_COMMIT_PARTS : wgs;       // the rows beyond are strided over
  const hipStream_t st = (hipStream_t)stream;
  if (f32)
    hipLaunchKernelGGL(rvq_commit_kernel<float>, dim3((unsigned)wgs), dim3(RT_NT), 0, st, *p, tl, groups, vec);
  else
    hipLaunchKernelGGL(rvq_commit_kernel<bf16_t>, dim3((unsigned)wgs), dim3(RT_NT), 0, st, *p, tl, groups, vec);
  return zs_check_launch("zs_rvq_commit");
}

extern "C" int zs_rvq_loss(const ZsRvqLoss* p, void* stream) {
  ZS_REQUIRE(p, "zs_rvq_loss: null argument");
  ZS_REQUIRE(p->S >= 1 && p->S <= ZS_RVQ_MAX_S, "zs_rvq_loss: S must be in [1, %d] (got %d)", ZS_RVQ_MAX_S, p->S);
  ZS_REQUIRE(p->partial && p->loss, "zs_rvq_loss: null operand");
  ZS_REQUIRE(!misaligned(p->partial, 8) && !misaligned(p->loss, 4), "zs_rvq_loss: an operand is not aligned to its element");
  hipLaunchKernelGGL(rvq_loss_kernel, dim3(1), dim3(RT_NT), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_rvq_loss");
}

extern "C" int zs_rvq_st_bwd(const ZsRvqStBwd* p, void* stream) {
  ZS_REQUIRE(p, "zs_rvq_st_bwd: null argument");
  const char* why = rt_shape(p->E, p->n);
  if (!why && (p->ld_dq < p->E || p->ld_dz < p->E || p->ld_a < p->E)) why = "a leading dimension is below E";
  ZS_REQUIRE(!why, "zs_rvq_st_bwd: %s (n %lld, E %d, ld_dq %lld, ld_a %lld, ld_dz %lld)", why, (long long)p->n, p->E, (long long)p->ld_dq,
             (long long)p->ld_a, (long long)p->ld_dz);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_rvq_st_bwd: bad dtype");
  ZS_REQUIRE(p->ld_dq % 8 == 0 && p->ld_dz % 8 == 0, "zs_rvq_st_bwd: ld_dq and ld_dz must be multiples of 8 (got %lld, %lld)",
             (long long)p->ld_dq, (long long)p->ld_dz);
  ZS_REQUIRE(!p->dq || p->dq != p->dz || p->ld_dq == p->ld_dz, "zs_rvq_st_bwd: in place (dz == dq) needs ld_dz == ld_dq");
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->dq && p->a && p->dz, "zs_rvq_st_bwd: null operand");
  ZS_REQUIRE(!misaligned(p->dq, 16) && !misaligned(p->dz, 16) && !misaligned(p->a, 4), "zs_rvq_st_bwd: an operand is misaligned (dq, dz: 16 bytes)");
  ZS_REQUIRE(static_cast<const void*>(p->a) != p->dq && static_cast<const void*>(p->a) != p->dz, "zs_rvq_st_bwd: a must not be dq or dz");
  const int per = p->dtype == ZS_F32 ? 4 : 8;
  const int groups = (int)(p->ld_dz / per);
  const int avec = !misaligned(p->a, 16) && p->ld_a % 4 == 0;
  int64_t wgs = (p->n * groups + RT_NT - 1) / RT_NT;
  wgs = wgs > 2048 ? 2048 : wgs;
  const hipStream_t st = (hipStream_t)stream;
  if (p->dtype == ZS_F32)
    hipLaunchKernelGGL(rvq_st_bwd_kernel<float>, dim3((unsigned)wgs), dim3(RT_NT), 0, st, *p, groups, avec);
  else
    hipLaunchKernelGGL(rvq_st_bwd_kernel<bf16_t>, dim3((unsigned)wgs), dim3(RT_NT), 0, st, *p, groups, avec);
  return zs_check_launch("zs_rvq_st_bwd");
}

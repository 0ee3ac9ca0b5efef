// zs_rvq_train.hip -- training a 'continues' model through its residual codebook (include/zs_amd.h): what a stage of the
// straight-through quantiser leaves over, with everything the step wants of it in the same pass (zs_rvq_commit), the commitment loss of
// the S stages from its partial sums (zs_rvq_loss) and the gradient (zs_rvq_st_bwd).  All three are memory-bound; the search, the
// fixed-point sums, the codebook's average and the restart of every stage are zs_vq_assign, zs_vq_accum, zs_vq_ema and zs_vq_restart,
// unchanged.  Nothing here adds floats atomically, so a step is bitwise reproducible.  zs_rvq_commit_drop (include/zs_amd_rvq_drop.h,
// DESIGN 37), the commit of a step under quantiser dropout, is the same kernel and the same host checks with DROP set.
//   rvq_commit_kernel   rvq_residual_kernel's layout: a row is owned by a team of 2^t <= 64 lanes of one wave, four columns per lane
//                       and round.  A lane reads its piece of x, of the one codeword row and (behind the first stage) of a, and
//                       writes its piece of r, of a and of the fp32 copy: every operand crosses the memory system once.  The row's
//                       magnitude check is an OR over the team by shuffles, as in vq_commit_kernel, and so is the tree of the doubles.
//                       One text for both entry points: zs_rvq_commit_drop with every count at S is zs_rvq_commit by construction.
//   rvq_loss_kernel     one workgroup: the [S][ZS_VQ_COMMIT_PARTS] partials in a fixed order.
//   rvq_st_bwd_kernel   one lane per 16-byte piece of dz, grid-stride.
// The row accesses and the teams' launch arithmetic are zs_quant.h's.
#include "zs_quant.h"
#include "../../include/zs_amd_rvq_drop.h"

// the definitions are stated operation by operation (a rounding each): nothing in this file may be fused into a multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int RT_NT = 256;

struct RtVec { int x, code, r, xf, a; };                          // which operands take 16-byte (x bf16: 8-byte) accesses

// ---- commit ------------------------------------------------------------------------------------------------------------------------
// DROP (zs_rvq_commit_drop, P = ZsRvqCommitDrop): only the rows of samples that still use stage p.stage take part (`act`).  Whether a
// row does is a property of its fragment, so of the whole team: the trip counts and the shuffles do not depend on it.
template <typename S, bool DROP, typename P> __global__ void __launch_bounds__(RT_NT)
rvq_commit_kernel(const P p, const int tl, const int groups, const RtVec vec) {
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
    bool act = live;                                                // the fragment's count decides for the whole team (a row has one
    if constexpr (DROP) act = live && p.stage < p.s_use[(int)row / p.rows_per_frag];        // fragment): the loop below runs either way
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
        q_load4<S>(xr, c, p.E, vec.x != 0, xv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          big |= (!DROP || act) && !(fabsf(xv[j]) < (float)ZS_VQ_MAX_ABS);     // (NaN: not below; the columns at or above E are zero)
          rv[j] = xv[j];
        }
        if (ok) {
          float cv[4];
          q_load4<float>(cr, c, p.E, vec.code != 0, cv);
          if (!p.first) q_load4<float>(ar, c, p.E, vec.a != 0, av);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            rv[j] = xv[j] - cv[j];                                  // one IEEE subtraction
            if (c + j < p.E) acc += (double)rv[j] * (double)rv[j];  // the stored value
            av[j] = p.first ? rv[j] : av[j] + rv[j];                // one fp32 add
          }
        }
        q_store4(rr, c, p.E, vec.r != 0, rv);                       // (a row that takes no part: the fp32 value of x)
        if (p.x_f32) q_store4(p.x_f32 + row * p.ld_xf, c, p.E, vec.xf != 0, xv);
        if (ok || ((!DROP || act) && p.first)) q_store4(ar, c, p.E, vec.a != 0, av);   // (a bad row: zero at the first stage, as behind it)
      }
    }
    for (int o = 1; o < tl; o <<= 1) big |= __shfl_xor(big, o, 64);  // over the team; every lane of the wave is here
    if (live && tlane == 0) {
      bad += (!DROP || act) && !ok;
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
      q_load4<float>(ar, c, p.E, avec != 0, lo);
      if (PER == 8) q_load4<float>(ar, c + 4, p.E, avec != 0, hi);
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

const char* rt_shape(int E, int64_t n) {
  if (E < 1 || E > ZS_CODE_MAX_E) return "E must be in [1, 1024]";
  if (n < 0 || n > 0x7fffffff) return "n must be in [0, 2^31)";
  return nullptr;
}

// zs_rvq_commit (P = ZsRvqCommit) and zs_rvq_commit_drop (DROP, P = ZsRvqCommitDrop): the checks, the teams and the launch
template <bool DROP, typename P> int commit_launch(const P* p, void* stream, const char* name) {
  ZS_REQUIRE(p, "%s: null argument", name);
  const char* why = rt_shape(p->E, p->n);
  if (!why && (p->K < 1 || p->K > ZS_CODE_MAX_K)) why = "K must be in [1, 65536]";
  if (!why && (p->ld_x < p->E || p->ld_code < p->E || p->ld_r < p->E || p->ld_a < p->E || (p->x_f32 && p->ld_xf < p->E)))
    why = "a leading dimension is below E";
  ZS_REQUIRE(!why, "%s: %s (n %lld, K %d, E %d, ld_x %lld, ld_code %lld, ld_r %lld, ld_xf %lld, ld_a %lld)", name, why, (long long)p->n,
             p->K, p->E, (long long)p->ld_x, (long long)p->ld_code, (long long)p->ld_r, (long long)p->ld_xf, (long long)p->ld_a);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "%s: bad dtype", name);
  const void* s_use = nullptr;                                    // DROP: an operand like the others
  if constexpr (DROP) {
    ZS_REQUIRE(p->rows_per_frag >= 1 && p->stage >= 0 && p->stage < ZS_RVQ_MAX_S && (p->first != 0) == (p->stage == 0),
               "%s: rows_per_frag must be >= 1, stage in [0, %d) and first set at stage 0 alone (got %d, stage %d, first %d)", name,
               ZS_RVQ_MAX_S, p->rows_per_frag, p->stage, p->first);
    s_use = p->s_use;
  }
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->x && p->idx && p->code && p->r && p->idx_acc && p->a && p->partial && p->bad && p->over && (!DROP || s_use),
             "%s: null operand", name);
  const bool f32 = p->src_f32 || p->dtype == ZS_F32;
  ZS_REQUIRE(!misaligned(p->x, f32 ? 4 : 2) && !misaligned(p->idx, 4) && !misaligned(p->code, 4) && !misaligned(p->r, 4) &&
                 !misaligned(p->x_f32, 4) && !misaligned(p->idx_acc, 4) && !misaligned(p->a, 4) && !misaligned(p->partial, 8) &&
                 !misaligned(p->bad, 4) && !misaligned(p->over, 4) && !misaligned(s_use, 4),
             "%s: an operand is not aligned to its element", name);
  const void* xv = p->x;
  ZS_REQUIRE(p->r != xv && p->a != xv && p->x_f32 != xv && p->r != p->a && p->r != p->x_f32 && p->a != p->x_f32,
             "%s: r, x_f32 and a must not be x or each other", name);
  ZS_REQUIRE(p->idx_acc != p->idx && (!DROP || p->idx_acc != s_use), "%s: idx_acc must not be idx%s", name, DROP ? " or s_use" : "");
  RtVec vec;
  vec.x = !misaligned(p->x, f32 ? 16 : 8) && p->ld_x % 4 == 0;
  vec.code = !misaligned(p->code, 16) && p->ld_code % 4 == 0;
  vec.r = !misaligned(p->r, 16) && p->ld_r % 4 == 0;
  vec.xf = p->x_f32 && !misaligned(p->x_f32, 16) && p->ld_xf % 4 == 0;
  vec.a = !misaligned(p->a, 16) && p->ld_a % 4 == 0;
  const int groups = (p->E + 3) / 4, tl = team_lanes(groups);
  const dim3 grid(team_wgs(p->n, tl, RT_NT, ZS_VQ_COMMIT_PARTS));
  const hipStream_t st = (hipStream_t)stream;
  if (f32)
    hipLaunchKernelGGL((rvq_commit_kernel<float, DROP, P>), grid, dim3(RT_NT), 0, st, *p, tl, groups, vec);
  else
    hipLaunchKernelGGL((rvq_commit_kernel<bf16_t, DROP, P>), grid, dim3(RT_NT), 0, st, *p, tl, groups, vec);
  return zs_check_launch(name);
}

}  // namespace

extern "C" int zs_rvq_commit(const ZsRvqCommit* p, void* stream) {
  return commit_launch<false>(p, stream, "zs_rvq_commit");
}

extern "C" int zs_rvq_commit_drop(const ZsRvqCommitDrop* p, void* stream) {
  return commit_launch<true>(p, stream, "zs_rvq_commit_drop");
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

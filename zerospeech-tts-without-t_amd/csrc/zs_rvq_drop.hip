// zs_rvq_drop.hip -- quantiser dropout for training through the residual codebook (include/zs_amd_rvq_drop.h): the stage
// count of every sample drawn on the device (zs_rvq_drop_draw).  The other two entry points of that header are instances of the
// kernels they mask: zs_rvq_commit_drop is rvq_commit_kernel with DROP set (zs_rvq_train.hip) and zs_rvq_gather_frag rvq_gather_kernel
// with FRAG set (zs_rvq.hip); the search, the sums, the average, the restart, the loss and the backward are the unchanged entry points.
//   rvq_drop_draw_kernel     one workgroup: lane t draws the samples t, t + 256, ..; the S integer counts go through the waves' shuffles.
//                            Integers alone: a step stays bitwise reproducible.
#include "zs_quant.h"
#include "../../include/zs_amd_rvq_drop.h"

namespace {

constexpr int RD_NT = 256;

// ---- draw --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RD_NT) rvq_drop_draw_kernel(const ZsRvqDropDraw p) {
  __shared__ int s_cnt[RD_NT / 64][ZS_RVQ_MAX_S];
  const int tid = threadIdx.x;
  const uint64_t base = p.seed + (p.seed_ptr ? *p.seed_ptr : 0ull) + (uint64_t)ZS_RVQ_DROP_SALT;
  int cnt[ZS_RVQ_MAX_S];
#pragma unroll
  for (int s = 0; s < ZS_RVQ_MAX_S; ++s) cnt[s] = 0;
  for (int b = tid; b < p.n_frag; b += RD_NT) {
    const uint64_t u = q_mix64(base + (uint64_t)b * 0x9E3779B97F4A7C15ull);
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

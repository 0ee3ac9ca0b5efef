// zs_eval.hip -- zs_eval_accum: one held-out validation batch added into device-resident tables (include/zs_amd.h).
// Three launches on the caller's stream, no host synchronisation:
//   eval_l1_kernel     |x_dec - x| of a share of one sample's rows per workgroup (ZS_EVAL_PARTS shares a sample, so B = 256 puts
//                      2048 workgroups on the chip, all resident at once): one HBM pass over both operands with eight 16-byte
//                      loads in flight per lane, per-lane double sums in a fixed order, one double partial per workgroup into `work`
//   eval_units_kernel  column counts of the 0 / 1 units: one lane per four unit columns walks the frames of its samples and keeps
//                      the previous frame's bits in registers; integer atomics at the end (integer sums do not depend on order)
//   eval_finish_kernel one lane per SPEAKER scans the samples b = 0 .. B-1 in order (speaker ids and sample sums staged in LDS) and
//                      adds those of its speaker to the running double it loaded from spk_sum: exactly the sequential pass
//                      spk_sum[c[b]] += s_b, without a floating-point atomic and without B dependent trips to memory
#include "zs_common.h"

namespace {

constexpr int NT = 256;
constexpr int TILE = 1024;                                        // samples staged per round of the finish kernel

struct alignas(4) F4 { float v[4]; };                             // four columns in one load; rows need 4-byte alignment only

__global__ void __launch_bounds__(NT) eval_l1_kernel(const ZsEvalAccum p) {
  __shared__ double sh[NT / 64];
  const int g = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = (int)((int64_t)g * p.T / ZS_EVAL_PARTS), r1 = (int)((int64_t)(g + 1) * p.T / ZS_EVAL_PARTS);
  const int nvec = p.F >> 2, ntail = p.F & 3;
  const int n4 = (r1 - r0) * nvec, n1 = (r1 - r0) * ntail;          // the share's 4-column pieces and tail columns, as flat lists
  for (int b = blockIdx.y; b < p.B; b += gridDim.y) {
    const float* d0 = p.x_dec + ((int64_t)b * p.T + r0) * p.ld_dec;
    const float* x0 = p.x + ((int64_t)b * p.T + r0) * p.ldx;
    double acc = 0.0;
    // four pieces per lane and round: eight 16-byte loads in flight before the first one is used
    for (int i0 = threadIdx.x; i0 < n4; i0 += 4 * NT) {
      F4 a[4], c[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * NT;
        if (i < n4) {
          const int r = i / nvec, v = i - r * nvec;
          a[k] = *reinterpret_cast<const F4*>(d0 + (int64_t)r * p.ld_dec + 4 * v);
          c[k] = *reinterpret_cast<const F4*>(x0 + (int64_t)r * p.ldx + 4 * v);
        } else {
          a[k] = F4{{0.f, 0.f, 0.f, 0.f}};
          c[k] = a[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)fabsf(a[k].v[j] - c[k].v[j]);
    }
    for (int i = threadIdx.x; i < n1; i += NT) {                    // columns F - F % 4 .. F - 1, one by one
      const int r = i / ntail, f = 4 * nvec + (i - r * ntail);
      acc += (double)fabsf(d0[(int64_t)r * p.ld_dec + f] - x0[(int64_t)r * p.ldx + f]);
    }
    acc = wave_sum_d(acc);
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) p.work[(int64_t)b * ZS_EVAL_PARTS + g] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
  }
}

// V columns per lane (4: one 16-byte load a frame, where E % 4 == 0 and bits_f32 is 16-byte aligned).  A workgroup row (blockIdx.y)
// takes whole samples, so a lane sees consecutive frames of one sample and a pair never spans two samples; eight frames are
// loaded before the first is looked at.
template <int V> __global__ void __launch_bounds__(NT) eval_units_kernel(const ZsEvalAccum p) {
  struct alignas(4 * V) Row { float v[V]; };
  const int j = (blockIdx.x * NT + threadIdx.x) * V;
  if (j >= p.E) return;
  unsigned long long ones[V], flips[V];
#pragma unroll
  for (int k = 0; k < V; ++k) ones[k] = flips[k] = 0;
  for (int b = blockIdx.y; b < p.B; b += gridDim.y) {
    const float* s = p.bits_f32 + (int64_t)b * p.T4 * p.E + j;
    bool prev[V];
    for (int t0 = 0; t0 < p.T4; t0 += 8) {
      Row r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (t0 + k < p.T4) r[k] = *reinterpret_cast<const Row*>(s + (int64_t)(t0 + k) * p.E);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (t0 + k < p.T4) {
#pragma unroll
          for (int q = 0; q < V; ++q) {
            const bool cur = r[k].v[q] != 0.f;
            ones[q] += cur;
            if (t0 + k > 0) flips[q] += cur != prev[q];
            prev[q] = cur;
          }
        }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if (ones[k]) atomicAdd(reinterpret_cast<unsigned long long*>(p.ones) + j + k, ones[k]);
    if (flips[k]) atomicAdd(reinterpret_cast<unsigned long long*>(p.flips) + j + k, flips[k]);
  }
}

__global__ void __launch_bounds__(NT) eval_finish_kernel(const ZsEvalAccum p) {
  __shared__ double s_sum[TILE];
  __shared__ int s_c[TILE];
  const int s = blockIdx.x * NT + threadIdx.x;
  const bool live = s < p.n_speakers;
  double acc = live ? p.spk_sum[s] : 0.0;
  long long cnt = 0;
  unsigned long long bad = 0;
  for (int b0 = 0; b0 < p.B; b0 += TILE) {
    const int n = p.B - b0 < TILE ? p.B - b0 : TILE;
    for (int i = threadIdx.x; i < n; i += NT) {
      const double* w = p.work + (int64_t)(b0 + i) * ZS_EVAL_PARTS;
      double v = w[0];
      for (int g = 1; g < ZS_EVAL_PARTS; ++g) v += w[g];
      const int64_t c = p.c[b0 + i];
      const bool ok = c >= 0 && c < p.n_speakers;                 // an id outside the tables is never an index
      s_c[i] = ok ? (int)c : -1;
      s_sum[i] = v;
      bad += !ok;
    }
    __syncthreads();
    if (live)
      for (int i = 0; i < n; ++i)
        if (s_c[i] == s) {
          acc += s_sum[i];
          ++cnt;
        }
    __syncthreads();
  }
  if (live && cnt) {
    p.spk_sum[s] = acc;
    p.spk_cnt[s] += cnt;
  }
  if (blockIdx.x == 0) {                                          // every workgroup sees every sample: one of them counts
    if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(p.bad), bad);
    if (threadIdx.x == 0 && p.bits_f32) {
      *p.rows += (uint64_t)p.B * (uint64_t)p.T4;
      *p.pairs += (uint64_t)p.B * (uint64_t)(p.T4 - 1);
    }
  }
}

}  // namespace

extern "C" int zs_eval_accum(const ZsEvalAccum* p, void* stream) {
  ZS_REQUIRE(p, "zs_eval_accum: null argument");
  ZS_REQUIRE(p->B > 0 && p->T > 0 && p->F > 0, "zs_eval_accum: B, T and F must be > 0 (got %d, %d, %d)", p->B, p->T, p->F);
  ZS_REQUIRE(p->n_speakers > 0 && p->n_speakers <= (1 << 24), "zs_eval_accum: n_speakers must be in [1, 2^24] (got %d)", p->n_speakers);
  ZS_REQUIRE(p->ld_dec >= p->F && p->ldx >= p->F, "zs_eval_accum: ld_dec and ldx must be >= F");
  ZS_REQUIRE((int64_t)p->T * p->F < (int64_t)1 << 31, "zs_eval_accum: T * F must be below 2^31");
  ZS_REQUIRE(p->x_dec && p->x && p->c && p->work && p->spk_sum && p->spk_cnt && p->bad, "zs_eval_accum: null operand");
  ZS_REQUIRE(((reinterpret_cast<uintptr_t>(p->x_dec) | reinterpret_cast<uintptr_t>(p->x)) & 3) == 0,
             "zs_eval_accum: x_dec and x must be 4-byte aligned");
  if (p->bits_f32) {
    ZS_REQUIRE(p->T4 > 0 && p->E > 0, "zs_eval_accum: T4 and E must be > 0 with bits_f32 (got %d, %d)", p->T4, p->E);
    ZS_REQUIRE(p->ones && p->flips && p->rows && p->pairs, "zs_eval_accum: bits_f32 needs ones, flips, rows and pairs");
  }
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(eval_l1_kernel, dim3(ZS_EVAL_PARTS, (unsigned)(p->B < 65535 ? p->B : 65535)), dim3(NT), 0, st, *p);
  if (p->bits_f32) {
    const unsigned by = (unsigned)(p->B < 256 ? p->B : 256);
    if (p->E % 4 == 0 && (reinterpret_cast<uintptr_t>(p->bits_f32) & 15) == 0)
      hipLaunchKernelGGL(eval_units_kernel<4>, dim3((unsigned)((p->E / 4 + NT - 1) / NT), by), dim3(NT), 0, st, *p);
    else
      hipLaunchKernelGGL(eval_units_kernel<1>, dim3((unsigned)((p->E + NT - 1) / NT), by), dim3(NT), 0, st, *p);
  }
  hipLaunchKernelGGL(eval_finish_kernel, dim3((unsigned)((p->n_speakers + NT - 1) / NT)), dim3(NT), 0, st, *p);
  return zs_check_launch("zs_eval_accum");
}

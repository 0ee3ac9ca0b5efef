// zs_abx.hip -- the kernels of --score_units (include/zs_amd_abx.h has the definitions; tests/abx_ref.py restates them in numpy).
//   abx_rownorm_kernel   one wave per row: lanes stride over the columns, one wave sum, 1 / sqrt.
//   abx_dtw_kernel       one wave per workgroup, 64 / W records per wave, one lane per column of the record's rectangle.  The
//                        rectangle is staged row by row into LDS as frame distances, ABX_ROWS = 16 rows at a time (a group of W lanes
//                        reads Lb consecutive floats of a row; the transcendental of the angular metric is paid once per cell, here);
//                        a lane only ever reads back what it wrote, so the tile needs no barrier.  The sweep of a slab then runs along
//                        the anti-diagonals: at step t lane j
//                        owns cell (t - j, j), `up` is its own value of step t - 1, `left` is the left lane's value of step t - 1 and
//                        `diag` the left lane's value of step t - 2, which is last step's `left`: ONE one-lane shift of (cost, len)
//                        per step.  The shift never has to know W: lane 0 of a group has no left neighbour and ignores what arrives.
//                        A record wider than W is kept back and run by the whole wave behind the others (the same device function
//                        with one lane per column), so W is a packing choice and never changes a result.
//                        THROUGHPUT-bound: pairs are independent.  The tile is 4 KB per wave and the kernel keeps 70 VGPRs (the 16
//                        loads of a slab are all in flight at once): seven waves per SIMD; a token of more than 16 rows pays Lb - 1 idle steps per further slab
//                        (DESIGN 41 has the measurements).
//   abx_count_kernel     one workgroup per job: the B values of the job go through LDS in tiles of 1024, every thread compares the A
//                        values it owns with the whole tile, integer sums meet by wave shuffles and one LDS round.
#include "zs_common.h"
#include "../../include/zs_amd_abx.h"

// fl32(g + m.cost) is a single rounding: nothing in this file may be fused into a multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int ABX_ROWS = 16;                                      // rows of the LDS tile: a record is swept in slabs of as many rows
constexpr int ABX_COUNT_NT = 256, ABX_COUNT_TILE = 1024, ABX_COUNT_MAX_BLOCKS = 65535 * 16;
constexpr float ABX_INV_PI = 0.318309886183790671537767526745f;

__global__ void __launch_bounds__(256) abx_rownorm_kernel(const ZsAbxRownorm p) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
  for (int64_t i = wave; i < p.n; i += nw) {
    const float* x = p.x + i * p.ld_x;
    float s = 0.f;
    for (int e = lane; e < p.E; e += 64) { const float v = x[e]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) p.rinv[i] = s == 0.f ? 0.f : __fdiv_rn(1.f, __fsqrt_rn(s));
  }
}

// the value of the lane below (lane 0 keeps its own): ds_bpermute, or the DPP wave shift that gfx9 has
template <bool DPP> __device__ __forceinline__ int abx_up1(int v) {
  if (DPP) return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  return __shfl_up(v, 1, 64);
}

struct AbxRec {                                                   // a record as the lanes of its group see it
  int row0, La, col0, Lb;
  bool live;                                                      // valid, and this lane has a column of it
};

__device__ __forceinline__ bool abx_lt(float ac, int al, float bc, int bl) { return ac < bc || (ac == bc && al < bl); }

// d of the record of this lane's group, in the lane of its last column (other lanes: unspecified).  j: the lane's column.
template <bool DPP> __device__ __forceinline__ float abx_dtw_group(const ZsAbxDtw& p, const AbxRec r, const int j, float* tile /* + lane */) {
  const float* s = p.scores + (int64_t)r.row0 * p.ld_s + r.col0 + j;
  const float e = (float)p.E, rc = r.live && p.metric == ZS_ABX_ANGULAR ? p.rinv_col[r.col0 + j] : 0.f;
  const int la = r.live ? r.La : 0;
  float cur_c = 0.f, dg_c = 0.f;
  int cur_l = 0, dg_l = 0;
  // ABX_ROWS rows at a time.  A slab is a sweep of its own: the lane's `up` of the slab's first row is its own value from the slab
  // before, and the left lane still holds ITS last value of that slab when this lane starts (one step later), which is `diag`.
  for (int i0 = 0; __any(i0 < la); i0 += ABX_ROWS) {
    const int nr = la - i0 < ABX_ROWS ? la - i0 : ABX_ROWS;       // rows of this slab (<= 0: the record is done)
    // stage: g(i, j) of this lane's column at tile[64 (i - i0)].  Every load of the slab is issued before the first is used: a
    // load per row that waits for the one before costs a memory latency per row, which is most of a short record's time.
    float v[ABX_ROWS], rr[ABX_ROWS];
#pragma unroll
    for (int k = 0; k < ABX_ROWS; ++k) v[k] = k < nr ? s[(int64_t)(i0 + k) * p.ld_s] : 0.f;
    if (p.metric == ZS_ABX_HAMMING) {
#pragma unroll
      for (int k = 0; k < ABX_ROWS; ++k)
        if (k < nr) tile[64 * k] = __fdiv_rn(v[k], e);
    } else {
#pragma unroll
      for (int k = 0; k < ABX_ROWS; ++k) rr[k] = k < nr ? p.rinv_row[r.row0 + i0 + k] : 0.f;
#pragma unroll
      for (int k = 0; k < ABX_ROWS; ++k)
        if (k < nr) {
          float c = ((-0.5f * v[k]) * rr[k]) * rc;
          c = c < -1.f ? -1.f : (c > 1.f ? 1.f : c);
          tile[64 * k] = acosf(c) * ABX_INV_PI;
        }
    }
    // sweep
    const int steps = nr > 0 ? nr + r.Lb - 1 : 0;
    for (int t = 0; __any(t < steps); ++t) {
      const float lf_c = __int_as_float(abx_up1<DPP>(__float_as_int(cur_c)));
      const int lf_l = abx_up1<DPP>(cur_l);
      const int k = t - j, i = i0 + k;
      if (k >= 0 && k < nr) {
        const float g = tile[64 * k];
        if (i == 0 && j == 0) {
          cur_c = g; cur_l = 1;
        } else {
          float mc = cur_c; int ml = cur_l;                       // up (exists when i > 0)
          if (j > 0) {
            if (i == 0 || abx_lt(lf_c, lf_l, mc, ml)) { mc = lf_c; ml = lf_l; }
            if (i > 0 && abx_lt(dg_c, dg_l, mc, ml)) { mc = dg_c; ml = dg_l; }
          }
          cur_c = g + mc; cur_l = ml + 1;
        }
      }
      dg_c = lf_c; dg_l = lf_l;
    }
  }
  return __fdiv_rn(cur_c, (float)cur_l);
}

__device__ __forceinline__ bool abx_dst_ok(const ZsAbxDtw& p, const ZsAbxPair& q) {
  return q.dst0 >= 0 && q.dst0 < p.n_out && q.dst1 >= -1 && q.dst1 < p.n_out;
}
__device__ __forceinline__ bool abx_rect_ok(const ZsAbxDtw& p, const ZsAbxPair& q) {
  return q.La >= 1 && q.La <= ZS_ABX_MAX_LEN && q.Lb >= 1 && q.Lb <= ZS_ABX_MAX_LEN && q.row0 >= 0 && q.col0 >= 0 &&
         (int64_t)q.row0 + q.La <= p.n_rows && (int64_t)q.col0 + q.Lb <= p.n_cols;
}
__device__ __forceinline__ void abx_put(const ZsAbxDtw& p, const ZsAbxPair& q, float d) {
  p.out[q.dst0] = d;
  if (q.dst1 >= 0) p.out[q.dst1] = d;
}

template <bool DPP> __global__ void __launch_bounds__(64) abx_dtw_kernel(const ZsAbxDtw p, const int W) {
  __shared__ float s_tile[ABX_ROWS * 64];
  const int lane = threadIdx.x, per = 64 / W, j = lane & (W - 1);
  float* tile = s_tile + lane;
  const int64_t rec = (int64_t)blockIdx.x * per + lane / W;
  ZsAbxPair q = {0, 0, 0, 0, -1, -1};
  bool ok = false, wide = false;
  if (rec < p.n_pairs) {
    q = p.pairs[rec];
    ok = abx_rect_ok(p, q) && abx_dst_ok(p, q);
    if (!ok && j == 0) {                                          // NaN to the destinations that exist, nothing read of S
      const float nan = __uint_as_float(0x7fc00000u);
      if (q.dst0 >= 0 && q.dst0 < p.n_out) p.out[q.dst0] = nan;
      if (q.dst1 >= 0 && q.dst1 < p.n_out) p.out[q.dst1] = nan;
      atomicAdd(p.bad, 1);
    }
    wide = ok && q.Lb > W;
  }
  const AbxRec r = {q.row0, q.La, q.col0, q.Lb, ok && !wide && j < q.Lb};
  const float d = abx_dtw_group<DPP>(p, r, j, tile);
  if (r.live && j == q.Lb - 1) abx_put(p, q, d);
  // the records wider than W, one at a time over the whole wave
  unsigned long long left = __ballot(wide && j == 0);
  while (left) {
    const int src = __ffsll((long long)left) - 1;
    left &= left - 1;
    ZsAbxPair w;
    w.row0 = __shfl(q.row0, src, 64); w.La = __shfl(q.La, src, 64); w.col0 = __shfl(q.col0, src, 64); w.Lb = __shfl(q.Lb, src, 64);
    w.dst0 = ((int64_t)__shfl((int)(q.dst0 >> 32), src, 64) << 32) | (uint32_t)__shfl((int)q.dst0, src, 64);
    w.dst1 = ((int64_t)__shfl((int)(q.dst1 >> 32), src, 64) << 32) | (uint32_t)__shfl((int)q.dst1, src, 64);
    const AbxRec rw = {w.row0, w.La, w.col0, w.Lb, lane < w.Lb};
    const float dw = abx_dtw_group<DPP>(p, rw, lane, tile);
    if (lane == w.Lb - 1) abx_put(p, w, dw);
  }
}

__global__ void __launch_bounds__(ABX_COUNT_NT) abx_count_kernel(const ZsAbxCount p) {
  __shared__ float s_b[ABX_COUNT_TILE];
  __shared__ unsigned long long s_sum[ABX_COUNT_NT / 64];
  const int tid = threadIdx.x;
  for (int64_t jb = blockIdx.x; jb < p.n_jobs; jb += gridDim.x) {
    const ZsAbxJob q = p.jobs[jb];
    const bool ok = q.x >= 0 && q.x < p.n && q.a0 >= 0 && q.a0 <= q.a1 && q.a1 <= p.n_cols && q.b0 >= 0 && q.b0 <= q.b1 && q.b1 <= p.n_cols;
    if (!ok) {                                                    // (uniform over the workgroup)
      if (tid == 0) { p.wins2[jb] = 0; atomicAdd(p.bad, 1); }
      continue;
    }
    const float* row = p.d + (int64_t)q.x * p.ld_d;
    unsigned long long sum = 0;
    for (int b0 = q.b0; b0 < q.b1; b0 += ABX_COUNT_TILE) {
      const int nb = q.b1 - b0 < ABX_COUNT_TILE ? q.b1 - b0 : ABX_COUNT_TILE;
      __syncthreads();                                            // the tile before is read
      for (int k = tid; k < nb; k += ABX_COUNT_NT) s_b[k] = row[b0 + k];
      __syncthreads();
      for (int a = q.a0 + tid; a < q.a1; a += ABX_COUNT_NT) {
        if (a == q.skip) continue;
        const float da = row[a];
        uint32_t lt = 0, eq = 0;
        for (int k = 0; k < nb; ++k) { const float db = s_b[k]; lt += da < db; eq += da == db; }
        sum += 2ull * lt + eq;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t hi = __shfl_xor((uint32_t)(sum >> 32), o, 64), lo = __shfl_xor((uint32_t)sum, o, 64);
      sum += ((unsigned long long)hi << 32) | lo;
    }
    __syncthreads();                                              // s_sum of the job before is read
    if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
      unsigned long long t = 0;
      for (int w = 0; w < ABX_COUNT_NT / 64; ++w) t += s_sum[w];
      p.wins2[jb] = t;
    }
  }
}

inline bool abx_misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

}  // namespace

extern "C" int zs_abx_rownorm(const ZsAbxRownorm* p, void* stream) {
  ZS_REQUIRE(p, "zs_abx_rownorm: null argument");
  ZS_REQUIRE(p->n >= 0 && p->n <= 0x7fffffff, "zs_abx_rownorm: n must be in [0, 2^31) (got %lld)", (long long)p->n);
  ZS_REQUIRE(p->E >= 1, "zs_abx_rownorm: E must be >= 1 (got %d)", p->E);
  ZS_REQUIRE(p->ld_x >= p->E, "zs_abx_rownorm: ld_x %lld is below E %d", (long long)p->ld_x, p->E);
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->x && p->rinv, "zs_abx_rownorm: null operand");
  ZS_REQUIRE(!abx_misaligned(p->x, 4) && !abx_misaligned(p->rinv, 4), "zs_abx_rownorm: an operand is not aligned to its element");
  const int64_t blocks = (p->n + 3) / 4;
  hipLaunchKernelGGL(abx_rownorm_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_abx_rownorm");
}

extern "C" int zs_abx_dtw(const ZsAbxDtw* p, void* stream) {
  ZS_REQUIRE(p, "zs_abx_dtw: null argument");
  ZS_REQUIRE(p->metric == ZS_ABX_HAMMING || p->metric == ZS_ABX_ANGULAR, "zs_abx_dtw: metric must be ZS_ABX_HAMMING or ZS_ABX_ANGULAR (got %d)",
             p->metric);
  ZS_REQUIRE(p->E >= 1, "zs_abx_dtw: E must be >= 1 (got %d)", p->E);
  ZS_REQUIRE(p->width == 0 || p->width == 4 || p->width == 8 || p->width == 16 || p->width == 32 || p->width == 64,
             "zs_abx_dtw: width must be 0, 4, 8, 16, 32 or 64 (got %d)", p->width);
  ZS_REQUIRE(p->n_pairs >= 0 && p->n_pairs <= 0x7fffffff && p->n_rows >= 0 && p->n_rows <= 0x7fffffff && p->n_cols >= 0 &&
                 p->n_cols <= 0x7fffffff && p->n_out >= 0, "zs_abx_dtw: n_pairs, n_rows and n_cols must be in [0, 2^31) and n_out >= 0 "
             "(got %lld, %lld, %lld, %lld)", (long long)p->n_pairs, (long long)p->n_rows, (long long)p->n_cols, (long long)p->n_out);
  ZS_REQUIRE(p->ld_s >= p->n_cols, "zs_abx_dtw: ld_s %lld is below n_cols %lld", (long long)p->ld_s, (long long)p->n_cols);
  if (p->n_pairs == 0) return ZS_OK;
  ZS_REQUIRE(p->pairs && p->bad, "zs_abx_dtw: null operand");
  ZS_REQUIRE((p->scores || p->n_rows == 0 || p->n_cols == 0) && (p->out || p->n_out == 0), "zs_abx_dtw: null operand");
  ZS_REQUIRE(p->metric != ZS_ABX_ANGULAR || ((p->rinv_row || p->n_rows == 0) && (p->rinv_col || p->n_cols == 0)),
             "zs_abx_dtw: the angular metric needs rinv_row and rinv_col");
  ZS_REQUIRE(!abx_misaligned(p->scores, 4) && !abx_misaligned(p->rinv_row, 4) && !abx_misaligned(p->rinv_col, 4) &&
                 !abx_misaligned(p->pairs, 8) && !abx_misaligned(p->out, 4) && !abx_misaligned(p->bad, 4),
             "zs_abx_dtw: an operand is not aligned to its element (pairs: 8 bytes)");
  const int W = p->width ? p->width : 64;
  const dim3 g((unsigned)((p->n_pairs + 64 / W - 1) / (64 / W))), b(64);
  if (p->dpp) hipLaunchKernelGGL(abx_dtw_kernel<true>, g, b, 0, (hipStream_t)stream, *p, W);
  else hipLaunchKernelGGL(abx_dtw_kernel<false>, g, b, 0, (hipStream_t)stream, *p, W);
  return zs_check_launch("zs_abx_dtw");
}

extern "C" int zs_abx_count(const ZsAbxCount* p, void* stream) {
  ZS_REQUIRE(p, "zs_abx_count: null argument");
  ZS_REQUIRE(p->n_jobs >= 0 && p->n_jobs <= 0x7fffffff && p->n >= 0 && p->n <= 0x7fffffff && p->n_cols >= 0 && p->n_cols <= 0x7fffffff,
             "zs_abx_count: n_jobs, n and n_cols must be in [0, 2^31) (got %lld, %lld, %lld)", (long long)p->n_jobs, (long long)p->n,
             (long long)p->n_cols);
  ZS_REQUIRE(p->ld_d >= p->n_cols, "zs_abx_count: ld_d %lld is below n_cols %lld", (long long)p->ld_d, (long long)p->n_cols);
  if (p->n_jobs == 0) return ZS_OK;
  ZS_REQUIRE(p->jobs && p->wins2 && p->bad, "zs_abx_count: null operand");
  ZS_REQUIRE(p->d || p->n == 0 || p->n_cols == 0, "zs_abx_count: null operand");
  ZS_REQUIRE(!abx_misaligned(p->d, 4) && !abx_misaligned(p->jobs, 4) && !abx_misaligned(p->wins2, 8) && !abx_misaligned(p->bad, 4),
             "zs_abx_count: an operand is not aligned to its element");
  const unsigned grid = (unsigned)(p->n_jobs < ABX_COUNT_MAX_BLOCKS ? p->n_jobs : ABX_COUNT_MAX_BLOCKS);
  hipLaunchKernelGGL(abx_count_kernel, dim3(grid), dim3(ABX_COUNT_NT), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_abx_count");
}

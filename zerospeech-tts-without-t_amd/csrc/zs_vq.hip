// zs_vq.hip -- the vector codebook of enc_mode 'continues' (include/zs_amd.h): nearest codeword in Euclidean distance
// (zs_vq_assign, a GEMM with an argmin epilogue on the exact-fp32 MFMA), the two halves of a k-means iteration around it
// (zs_vq_accum, zs_vq_update: fixed-point int64 sums, so a fit is bitwise reproducible) and the Decoder's input operand of an
// inference chunk built from indices (zs_vq_gather).
//   vq_assign_kernel   a workgroup owns VQ_BM = 128 rows of x (32 per wave) and walks its codewords ZS_VQ_TILE_K = 128 at a time; per
//                      tile the E columns pass through LDS 32 at a time, both operands transposed ([column][row], pitch 129: the
//                      staging writes of a 32-lane group hit 32 banks, the fragment reads are 32 consecutive words).  A wave holds
//                      4 accumulators of v_mfma_f32_32x32x2_f32 with the codewords on the M side and its rows on the N side, so lane l
//                      sees row l % 32 in every accumulator register: the running best of a row is ONE 64-bit word per lane,
//                      (orderable score << 32) | k, kept by an unsigned min.  The least word is the least score at the lowest index
//                      in whatever order the codewords come, so the tie rule survives the tiling and the split over K.  The score
//                      of a (row, codeword) pair is the same chain of MFMAs over the same zero-padded columns wherever the codeword
//                      sits in a tile, in either decomposition.
//                      blockIdx.y splits K (rows below ZS_VQ_SPLIT_N with a workspace): the words of a row meet by a 64-bit
//                      atomic min in the workspace, and vq_finish_kernel writes the outputs.
//   vq_scores_kernel   zs_vq_scores (--segment): the same tile loop and score expression (vq_tile_products, vq_score: one device function
//                      each, compiled into both kernels), one 128 x 128 tile per workgroup, the scores stored instead of reduced.
//   vq_accum_kernel    zs_code_accum's scheme: a workgroup owns a tile of codewords (those whose int64 sums fit 64 KiB of LDS) and
//                      a slice of the rows, lists the rows of its codewords per round and adds their quantised columns with LDS
//                      atomics; the non-zero sums go to memory with one 64-bit atomic each.
//   vq_update_kernel   one workgroup per codeword.
//   vq_gather_kernel   one lane per 16-byte piece of the operand, as units_unpack_kernel (the piece store is zs_quant.h's).
#include "zs_quant.h"

// nothing in this file is defined a rounding at a time: the scores and the norms contract as the compiler sees fit
#pragma clang fp contract(fast)

namespace {

constexpr int VQ_NT = 256, VQ_BM = 128, VQ_BN = ZS_VQ_TILE_K, VQ_KC = 32, VQ_P = 129;
static_assert(VQ_BN == 128 && VQ_BM == 128, "the staging maps below are written for 128 x 128 tiles");

// float -> a word whose unsigned order is the float order (-inf lowest; NaN above +inf, so it never wins against a number)
__device__ __forceinline__ uint32_t vq_ord(float s) {
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float vq_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// columns c .. c + 3 of a row as fp32; those at or above E, and every column of a row that is not `ok`, read nothing and are zero
template <typename S> __device__ __forceinline__ void vq_load4(const S* row, int c, int E, bool ok, bool vec, float (&v)[4]);
template <> __device__ __forceinline__ void vq_load4<float>(const float* row, int c, int E, bool ok, bool vec, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (!ok || c >= E) return;
  if (vec && c + 4 <= E) {
    const float4 a = *reinterpret_cast<const float4*>(row + c);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c + i < E) v[i] = row[c + i];
}
template <> __device__ __forceinline__ void vq_load4<bf16_t>(const bf16_t* row, int c, int E, bool ok, bool vec, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (!ok || c >= E) return;
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

// the outputs of one row from its winning word; every lane of the wave calls it (live: this lane has a row)
__device__ __forceinline__ void vq_finish_row(const ZsVqAssign& p, bool live, int64_t row, uint64_t key, float xn) {
  const int k = (int)(uint32_t)key;
  int mv = 0;
  if (live) {
    if (p.idx) {
      if (p.count_moved) mv = p.idx[row] != k;
      p.idx[row] = k;
    }
    if (p.dist) p.dist[row] = fmaxf(0.f, xn + vq_unord((uint32_t)(key >> 32)));
  }
  if (p.count_moved) {
    const int m = __popcll(__ballot(mv));
    if (m && (threadIdx.x & 63) == 0) atomicAdd(p.moved, m);
  }
}

// THE tile loop of zs_vq_assign and zs_vq_scores: the products of the workgroup's 128 rows (from row0) with the codewords k0 .. k0 +
// 127 (those below kend; the others are zero) over the E columns, zero-padded to pairs, into the wave's 4 accumulators; cnorm of the
// tile into sCn.  SQ: the squared norms of the rows are added to sq as the rows pass (zs_vq_assign's dist).
template <typename S, bool SQ, typename P>
__device__ __forceinline__ void vq_tile_products(const P& o, int64_t row0, int k0, int kend, int xvec, int cvec, float* sX,
                                                 float* sC, float* sCn, f32x16 (&acc)[4], bool want_sq, float (&sq)[4], int wave) {
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
  const S* x = static_cast<const S*>(o.x);
  const int g = tid & 7, rr = tid >> 3;                           // staging: columns 4g .. 4g + 3 of the tile rows rr + 32q
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[cb][v] = 0.f;
  for (int j0 = 0; j0 < o.E; j0 += VQ_KC) {
    __syncthreads();                                              // the chunk (and the tile's epilogue) before is done with LDS
    if (j0 == 0 && tid < VQ_BN) sCn[tid] = k0 + tid < kend ? o.cnorm[k0 + tid] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = rr + 32 * q;
      float v[4];
      vq_load4<S>(x + (row0 + r) * o.ld_x, j0 + 4 * g, o.E, row0 + r < o.n, xvec != 0, v);
      if (SQ && want_sq) sq[q] += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) sX[(4 * g + i) * VQ_P + r] = v[i];
      vq_load4<float>(o.code + (int64_t)(k0 + r) * o.ld_code, j0 + 4 * g, o.E, k0 + r < kend, cvec != 0, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) sC[(4 * g + i) * VQ_P + r] = v[i];
    }
    __syncthreads();
    const int cols = o.E - j0 < VQ_KC ? o.E - j0 : VQ_KC;         // an odd last column pairs with a zero one
    const int steps = (cols + 1) >> 1;
    const float* xb = sX + half * VQ_P + wave * 32 + l32;
    const float* cb0 = sC + half * VQ_P + l32;
    for (int s = 0; s < steps; ++s) {
      const float b = xb[2 * s * VQ_P];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(cb0[2 * s * VQ_P + cb * 32], b, acc[cb], 0, 0, 0);
    }
  }
}

// THE score of a (row, codeword) pair from its accumulator register
__device__ __forceinline__ float vq_score(float cn, float acc) {
  const float s = cn - 2.f * acc;
  return s == 0.f ? 0.f : s;                                      // one zero
}
// register v of accumulator cb: codeword k0 + 32 cb + 8 (v / 4) + 4 half + v % 4, row wave * 32 + l32
__device__ __forceinline__ int vq_acc_codeword(int cb, int v, int half) { return 32 * cb + 8 * (v >> 2) + 4 * half + (v & 3); }

template <typename S> __global__ void __launch_bounds__(VQ_NT)
vq_assign_kernel(const ZsVqAssign p, const int kper, const int xvec, const int cvec, const int split) {
  __shared__ float sX[VQ_KC * VQ_P], sC[VQ_KC * VQ_P];
  __shared__ float sCn[VQ_BN], sXn[VQ_BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  const int64_t row0 = (int64_t)blockIdx.x * VQ_BM;
  const int kbeg = blockIdx.y * kper, kend = kbeg + kper < p.K ? kbeg + kper : p.K;
  const int g = tid & 7, rr = tid >> 3;
  const bool want_norm = p.dist != nullptr && blockIdx.y == 0;
  float sq[4] = {0.f, 0.f, 0.f, 0.f};
  uint64_t best = ~(uint64_t)0;
  for (int k0 = kbeg; k0 < kend; k0 += VQ_BN) {
    f32x16 acc[4];
    vq_tile_products<S, true>(p, row0, k0, kend, xvec, cvec, sX, sC, sCn, acc, want_norm && k0 == kbeg, sq, wave);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int kl = vq_acc_codeword(cb, v, half);
        if (k0 + kl < kend) {
          const float s = vq_score(sCn[kl], acc[cb][v]);
          const uint64_t key = ((uint64_t)vq_ord(s) << 32) | (uint32_t)(k0 + kl);
          best = key < best ? key : best;
        }
      }
  }
  {
    const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), 32, 64), lo = __shfl_xor((uint32_t)best, 32, 64);
    const uint64_t other = ((uint64_t)hi << 32) | lo;
    best = other < best ? other : best;
  }
  if (want_norm) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float s = sq[q];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      if (g == 0) sXn[rr + 32 * q] = s;
    }
  }
  __syncthreads();
  const int r = wave * 32 + l32;
  const int64_t row = row0 + r;
  const bool live = half == 0 && row < p.n;
  if (split) {
    if (live) {
      atomicMin(static_cast<unsigned long long*>(p.work) + row, (unsigned long long)best);
      if (want_norm) reinterpret_cast<float*>(static_cast<unsigned long long*>(p.work) + p.n)[row] = sXn[r];
    }
  } else {
    vq_finish_row(p, live, row, best, want_norm ? sXn[r] : 0.f);
  }
}

__global__ void __launch_bounds__(VQ_NT) vq_finish_kernel(const ZsVqAssign p) {
  const int64_t row = (int64_t)blockIdx.x * VQ_NT + threadIdx.x;
  const bool live = row < p.n;
  const unsigned long long* keys = static_cast<const unsigned long long*>(p.work);
  const uint64_t key = live ? keys[row] : 0;
  const float xn = live && p.dist ? reinterpret_cast<const float*>(keys + p.n)[row] : 0.f;
  vq_finish_row(p, live, row, key, xn);
}

// zs_vq_scores: workgroup (x, y) writes the tile of rows 128 x .. and codewords 128 y ..: vq_tile_products and vq_score, then stores.
// A lane's registers 4i .. 4i + 3 of an accumulator are 4 consecutive codewords of its row: one 16-byte store where VEC (scores 16-byte
// aligned, ld_s a multiple of 4; a group of 4 starts at a multiple of 4 and K cuts it only in the last one), single elements otherwise.
template <typename S, bool VEC> __global__ void __launch_bounds__(VQ_NT)
vq_scores_kernel(const ZsVqScores p, const int xvec, const int cvec) {
  __shared__ float sX[VQ_KC * VQ_P], sC[VQ_KC * VQ_P];
  __shared__ float sCn[VQ_BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  const int64_t row0 = (int64_t)blockIdx.x * VQ_BM;
  const int k0 = blockIdx.y * VQ_BN, kend = p.K;
  float sq[4] = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc[4];
  vq_tile_products<S, false>(p, row0, k0, kend, xvec, cvec, sX, sC, sCn, acc, false, sq, wave);
  const int64_t row = row0 + wave * 32 + l32;
  if (row >= p.n) return;
  float* out = p.scores + row * p.ld_s + k0;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int v4 = 0; v4 < 16; v4 += 4) {
      const int kl = vq_acc_codeword(cb, v4, half);
      float s[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = vq_score(sCn[kl + i], acc[cb][v4 + i]);
      if (VEC && k0 + kl + 4 <= kend) {
        *reinterpret_cast<float4*>(out + kl) = make_float4(s[0], s[1], s[2], s[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (k0 + kl + i < kend) out[kl + i] = s[i];
      }
    }
}

// ---- accum -------------------------------------------------------------------------------------------------------------------------
constexpr int ACC_NT = 256, ACC_PER = 4, ACC_CHUNK = ACC_NT * ACC_PER;          // idx entries a workgroup looks at per round
constexpr int ACC_WORDS = 7168, ACC_MAX_KT = 256;                               // 56 KiB of private int64 sums (+ the list: < 64 KiB)

__global__ void __launch_bounds__(ACC_NT) vq_accum_kernel(const ZsVqAccum p, const int KT, const int64_t slice, const double scale) {
  __shared__ unsigned long long s_sum[ACC_WORDS];
  __shared__ int s_cnt[ACC_MAX_KT];
  __shared__ int s_list[ACC_CHUNK];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  const int k0 = blockIdx.x * KT, kt = p.K - k0 < KT ? p.K - k0 : KT;
  const int64_t r0 = (int64_t)blockIdx.y * slice, r1 = r0 + slice < p.n ? r0 + slice : p.n;
  for (int i = tid; i < kt * p.E; i += ACC_NT) s_sum[i] = 0;
  for (int i = tid; i < kt; i += ACC_NT) s_cnt[i] = 0;
  int bad = 0;
  for (int64_t base = r0; base < r1; base += ACC_CHUNK) {
    __syncthreads();                                              // the round before is done with the list (first: the sums are zero)
    if (tid == 0) s_n = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ACC_PER; ++q) {
      const int64_t r = base + q * ACC_NT + tid;
      if (r < r1) {
        const int k = p.idx[r];
        if (k < 0 || k >= p.K) {                                  // never an index; counted once, by the first column of workgroups
          bad += blockIdx.x == 0;
        } else if (k >= k0 && k < k0 + kt) {
          s_list[atomicAdd(&s_n, 1)] = ((q * ACC_NT + tid) << 10) | (k - k0);
        }
      }
    }
    __syncthreads();
    const int m = s_n, work = m * p.E;                            // <= 1024 x 1024
    for (int w = tid; w < work; w += ACC_NT) {
      const int j = w / p.E, c = w - j * p.E;
      const int e = s_list[j], kl = e & 1023;
      const double d = rint((double)p.x[(base + (e >> 10)) * p.ld_x + c] * scale);          // exact product, half to even
      atomicAdd(&s_sum[kl * p.E + c], (unsigned long long)(long long)d);
      if (c == 0) atomicAdd(&s_cnt[kl], 1);
    }
  }
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(p.sum) + (int64_t)k0 * p.E;
  for (int i = tid; i < kt * p.E; i += ACC_NT)
    if (const unsigned long long v = s_sum[i]) atomicAdd(out + i, v);
  for (int i = tid; i < kt; i += ACC_NT)
    if (const int v = s_cnt[i]) atomicAdd(p.cnt + k0 + i, v);
  if (bad) atomicAdd(p.bad, bad);
}

// ---- update ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VQ_NT) vq_update_kernel(const ZsVqUpdate p, const double inv_scale) {
  __shared__ double s_part[VQ_NT / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int c = p.cnt[k];
  float* row = p.code + (int64_t)k * p.ld_code;
  const int64_t* sum = p.sum + (int64_t)k * p.E;
  int diff = 0;
  double sq = 0.0;
  for (int j = tid; j < p.E; j += VQ_NT) {
    float v = row[j];
    if (c > 0) {
      const float nv = (float)((double)sum[j] / (double)c * inv_scale);
      if (__float_as_uint(nv) != __float_as_uint(v)) {
        diff = 1;
        row[j] = nv;
      }
      v = nv;
    }
    sq += (double)v * (double)v;
  }
  sq = wave_sum_d(sq);
  if ((tid & 63) == 0) s_part[tid >> 6] = sq;
  const int any = __syncthreads_or(diff);
  if (tid == 0) {
    p.cnorm[k] = (float)(s_part[0] + s_part[1] + s_part[2] + s_part[3]);
    if (any) atomicAdd(p.changed, 1);
  }
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------
template <typename T> __global__ void __launch_bounds__(VQ_NT) vq_gather_kernel(const ZsVqGather p) {
  constexpr int PER = 16 / (int)sizeof(T);                        // columns of a 16-byte piece
  const int groups = (int)(p.ld_dst / PER);
  const int64_t per_frag = (int64_t)p.T * groups;
  const int64_t tid = (int64_t)blockIdx.x * VQ_NT + threadIdx.x, nthr = (int64_t)gridDim.x * VQ_NT;
  int bad = 0;
  for (int64_t f = blockIdx.y; f < p.n_frag; f += gridDim.y) {
    const int64_t start = p.start[f];
    const int len = p.len[f];
    const bool ok = len >= 0 && len <= p.T && start >= 0 && start <= p.n_idx - len;          // else: a zero fragment, nothing read
    T* dst = static_cast<T*>(p.dst) + f * p.T * p.ld_dst;
    for (int64_t i = tid; i < per_frag; i += nthr) {
      const int t = (int)(i / groups), g = (int)(i - (int64_t)t * groups);
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (ok && t < len) {
        const int k = p.idx[start + t];
        if (k < 0 || k >= p.K) {
          bad += g == 0;                                          // once per row
        } else {
          const float* cw = p.code + (int64_t)k * p.ld_code;
#pragma unroll
          for (int j = 0; j < PER; ++j)
            if (PER * g + j < p.E) v[j] = cw[PER * g + j];
        }
      }
      q_store_piece<T>(dst + (int64_t)t * p.ld_dst + PER * g, v);
    }
  }
  if (bad) atomicAdd(p.bad, bad);
}

const char* vq_shape(int K, int E, int64_t n, int64_t ld_a, int64_t ld_b) {
  if (K < 1 || K > ZS_CODE_MAX_K) return "K must be in [1, 65536]";
  if (E < 1 || E > ZS_CODE_MAX_E) return "E must be in [1, 1024]";
  if (n < 0 || n > 0x7fffffff) return "n must be in [0, 2^31)";
  if (ld_a < E || ld_b < E) return "a leading dimension is below E";
  return nullptr;
}

}  // namespace

extern "C" int zs_vq_assign(const ZsVqAssign* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_assign: null argument");
  const char* why = vq_shape(p->K, p->E, p->n, p->ld_x, p->ld_code);
  ZS_REQUIRE(!why, "zs_vq_assign: %s (n %lld, K %d, E %d, ld_x %lld, ld_code %lld)", why, (long long)p->n, p->K, p->E, (long long)p->ld_x,
             (long long)p->ld_code);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_vq_assign: bad dtype");
  ZS_REQUIRE(p->work_bytes >= 0, "zs_vq_assign: work_bytes must be >= 0");
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->x && p->code && p->cnorm, "zs_vq_assign: null operand");
  ZS_REQUIRE(!p->count_moved || (p->idx && p->moved), "zs_vq_assign: count_moved needs idx and moved");
  const bool f32 = p->src_f32 || p->dtype == ZS_F32;
  ZS_REQUIRE(!misaligned(p->x, f32 ? 4 : 2) && !misaligned(p->code, 4) && !misaligned(p->cnorm, 4) && !misaligned(p->idx, 4) &&
                 !misaligned(p->dist, 4) && !misaligned(p->moved, 4) && !misaligned(p->work, 8),
             "zs_vq_assign: an operand is not aligned to its element");
  const int xvec = !misaligned(p->x, f32 ? 16 : 8) && p->ld_x % 4 == 0;
  const int cvec = !misaligned(p->code, 16) && p->ld_code % 4 == 0;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned row_tiles = (unsigned)((p->n + VQ_BM - 1) / VQ_BM);
  const int ktiles = (p->K + VQ_BN - 1) / VQ_BN;
  // K over workgroups: below ZS_VQ_SPLIT_N rows, with a workspace, when there is more than one tile of codewords.  About
  // ZS_VQ_SPLIT_WGS workgroups in all; a split takes whole tiles.
  int splits = 1;
  if (p->n < ZS_VQ_SPLIT_N && p->work && ktiles > 1) {
    ZS_REQUIRE(p->work_bytes >= 12 * p->n, "zs_vq_assign: the workspace holds %lld bytes, %lld rows need %lld (ZS_VQ_WORK_BYTES)",
               (long long)p->work_bytes, (long long)p->n, (long long)(12 * p->n));
    splits = (ZS_VQ_SPLIT_WGS + (int)row_tiles - 1) / (int)row_tiles;
    splits = splits > ktiles ? ktiles : splits;
  }
  const int kper = (ktiles + splits - 1) / splits * VQ_BN;
  splits = (p->K + kper - 1) / kper;
  const int split = splits > 1;
  if (split && hipMemsetAsync(p->work, 0xff, 8 * (size_t)p->n, st) != hipSuccess) return zs_check_launch("zs_vq_assign (workspace)");
  const dim3 grid(row_tiles, (unsigned)splits);
  if (f32)
    hipLaunchKernelGGL(vq_assign_kernel<float>, grid, dim3(VQ_NT), 0, st, *p, kper, xvec, cvec, split);
  else
    hipLaunchKernelGGL(vq_assign_kernel<bf16_t>, grid, dim3(VQ_NT), 0, st, *p, kper, xvec, cvec, split);
  if (split && (p->idx || p->dist))
    hipLaunchKernelGGL(vq_finish_kernel, dim3((unsigned)((p->n + VQ_NT - 1) / VQ_NT)), dim3(VQ_NT), 0, st, *p);
  return zs_check_launch("zs_vq_assign");
}

extern "C" int zs_vq_scores(const ZsVqScores* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_scores: null argument");
  const char* why = vq_shape(p->K, p->E, p->n, p->ld_x, p->ld_code);
  ZS_REQUIRE(!why, "zs_vq_scores: %s (n %lld, K %d, E %d, ld_x %lld, ld_code %lld)", why, (long long)p->n, p->K, p->E, (long long)p->ld_x,
             (long long)p->ld_code);
  ZS_REQUIRE(p->K <= ZS_SEG_MAX_K, "zs_vq_scores: K must be in [1, %d] (got %d)", ZS_SEG_MAX_K, p->K);
  ZS_REQUIRE(p->ld_s >= p->K, "zs_vq_scores: ld_s %lld is below K %d", (long long)p->ld_s, p->K);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_vq_scores: bad dtype");
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->x && p->code && p->cnorm && p->scores, "zs_vq_scores: null operand");
  const bool f32 = p->src_f32 || p->dtype == ZS_F32;
  ZS_REQUIRE(!misaligned(p->x, f32 ? 4 : 2) && !misaligned(p->code, 4) && !misaligned(p->cnorm, 4) && !misaligned(p->scores, 4),
             "zs_vq_scores: an operand is not aligned to its element");
  const int xvec = !misaligned(p->x, f32 ? 16 : 8) && p->ld_x % 4 == 0;
  const int cvec = !misaligned(p->code, 16) && p->ld_code % 4 == 0;
  const bool svec = !misaligned(p->scores, 16) && p->ld_s % 4 == 0;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((p->n + VQ_BM - 1) / VQ_BM), (unsigned)((p->K + VQ_BN - 1) / VQ_BN));
  if (f32 && svec) hipLaunchKernelGGL((vq_scores_kernel<float, true>), grid, dim3(VQ_NT), 0, st, *p, xvec, cvec);
  else if (f32) hipLaunchKernelGGL((vq_scores_kernel<float, false>), grid, dim3(VQ_NT), 0, st, *p, xvec, cvec);
  else if (svec) hipLaunchKernelGGL((vq_scores_kernel<bf16_t, true>), grid, dim3(VQ_NT), 0, st, *p, xvec, cvec);
  else hipLaunchKernelGGL((vq_scores_kernel<bf16_t, false>), grid, dim3(VQ_NT), 0, st, *p, xvec, cvec);
  return zs_check_launch("zs_vq_scores");
}

extern "C" int zs_vq_accum(const ZsVqAccum* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_accum: null argument");
  const char* why = vq_shape(p->K, p->E, p->n, p->ld_x, p->E);
  ZS_REQUIRE(!why, "zs_vq_accum: %s (n %lld, K %d, E %d, ld_x %lld)", why, (long long)p->n, p->K, p->E, (long long)p->ld_x);
  ZS_REQUIRE(p->shift >= -64 && p->shift <= 62, "zs_vq_accum: shift must be in [-64, 62] (got %d)", p->shift);
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->x && p->idx && p->cnt && p->sum && p->bad, "zs_vq_accum: null operand");
  ZS_REQUIRE(!misaligned(p->x, 4) && !misaligned(p->idx, 4) && !misaligned(p->cnt, 4) && !misaligned(p->bad, 4) && !misaligned(p->sum, 8),
             "zs_vq_accum: an operand is not aligned to its element");
  int KT = ACC_WORDS / p->E;                                      // codewords whose sums fit a workgroup's LDS: >= 7
  KT = KT > ACC_MAX_KT ? ACC_MAX_KT : KT;
  KT = KT > p->K ? p->K : KT;
  const int ktiles = (p->K + KT - 1) / KT;
  const int64_t chunks = (p->n + ACC_CHUNK - 1) / ACC_CHUNK;
  int64_t ns = 2048 / ktiles;                                     // row slices: about 2048 workgroups where the rows allow
  ns = ns < 1 ? 1 : (ns > chunks ? chunks : ns);
  const int64_t slice = (chunks + ns - 1) / ns * ACC_CHUNK;
  ns = (p->n + slice - 1) / slice;
  hipLaunchKernelGGL(vq_accum_kernel, dim3((unsigned)ktiles, (unsigned)ns), dim3(ACC_NT), 0, (hipStream_t)stream, *p, KT, slice,
                     ldexp(1.0, p->shift));
  return zs_check_launch("zs_vq_accum");
}

extern "C" int zs_vq_update(const ZsVqUpdate* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_update: null argument");
  const char* why = vq_shape(p->K, p->E, 0, p->ld_code, p->E);
  ZS_REQUIRE(!why, "zs_vq_update: %s (K %d, E %d, ld_code %lld)", why, p->K, p->E, (long long)p->ld_code);
  ZS_REQUIRE(p->shift >= -64 && p->shift <= 62, "zs_vq_update: shift must be in [-64, 62] (got %d)", p->shift);
  ZS_REQUIRE(p->code && p->cnorm && p->cnt && p->sum && p->changed, "zs_vq_update: null operand");
  ZS_REQUIRE(!misaligned(p->code, 4) && !misaligned(p->cnorm, 4) && !misaligned(p->cnt, 4) && !misaligned(p->changed, 4) &&
                 !misaligned(p->sum, 8), "zs_vq_update: an operand is not aligned to its element");
  hipLaunchKernelGGL(vq_update_kernel, dim3((unsigned)p->K), dim3(VQ_NT), 0, (hipStream_t)stream, *p, ldexp(1.0, -p->shift));
  return zs_check_launch("zs_vq_update");
}

extern "C" int zs_vq_gather(const ZsVqGather* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_gather: null argument");
  ZS_REQUIRE(p->n_frag >= 0 && p->n_frag <= ZS_UNITS_MAX_FRAG, "zs_vq_gather: n_frag must be in [0, %d] (got %d)", ZS_UNITS_MAX_FRAG,
             p->n_frag);
  const char* why = vq_shape(p->K, p->E, p->n_idx, p->ld_dst, p->ld_code);
  ZS_REQUIRE(!why, "zs_vq_gather: %s (n_idx %lld, K %d, E %d, ld_dst %lld, ld_code %lld)", why, (long long)p->n_idx, p->K, p->E,
             (long long)p->ld_dst, (long long)p->ld_code);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_vq_gather: bad dtype");
  ZS_REQUIRE(p->T > 0 && p->ld_dst % 8 == 0, "zs_vq_gather: T must be > 0 and ld_dst a multiple of 8");
  if (p->n_frag == 0) return ZS_OK;
  ZS_REQUIRE(p->dst && p->start && p->len && p->code && p->bad && (p->idx || p->n_idx == 0), "zs_vq_gather: null operand");
  ZS_REQUIRE(!misaligned(p->dst, 16) && !misaligned(p->code, 4) && !misaligned(p->idx, 4) && !misaligned(p->bad, 4) &&
                 !misaligned(p->start, 8) && !misaligned(p->len, 4), "zs_vq_gather: an operand is misaligned (dst: 16 bytes)");
  const int per = p->dtype == ZS_F32 ? 4 : 8;
  int64_t bx = ((int64_t)p->T * (p->ld_dst / per) + VQ_NT - 1) / VQ_NT;
  bx = bx > 64 ? 64 : bx;
  const dim3 grid((unsigned)bx, (unsigned)(p->n_frag < 65535 ? p->n_frag : 65535));
  if (p->dtype == ZS_F32)
    hipLaunchKernelGGL(vq_gather_kernel<float>, grid, dim3(VQ_NT), 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL(vq_gather_kernel<bf16_t>, grid, dim3(VQ_NT), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_vq_gather");
}

// zs_segment.hip -- zs_seg_viterbi: the index sequence of every utterance chosen at once under a switch penalty (include/zs_amd_segment.h has
// the definition; tests/segment_ref.py restates it in numpy fp32 and is reproduced bit for bit).
//   seg_viterbi_kernel<NS, NW>  one workgroup of NW waves per utterance, the grid strides over the utterances.  Lane `tid` keeps the
//                      states k = tid + 64 NW j (j < NS) in registers, so a score row is read in whole coalesced pieces and K <= 4096
//                      needs at most 16 states per lane.  Per frame: every lane folds its states into ONE 64-bit word,
//                      (orderable cost << 32) | k, as vq_assign_kernel does; the least word is the least cost at the lowest k, so
//                      one unsigned min gives m_t, a_t and the tie rule.  The words meet across the wave by lane exchange (DPP inside
//                      a row of 16 lanes, two exchanges across rows) and across the waves through two LDS slots used in turn: ONE
//                      barrier per frame.  The score row of frame t + 1 (and the row index of t + 2) is loaded before the reduction
//                      of frame t.  The switch bits of a frame are wave ballots: whole 64-bit words, word k / 64 of the frame.
//                      After the sweep wave 0 walks the path back 64 frames at a time: every lane reads the bit of its own frame
//                      for the state the walk is in, a ballot finds the first switch, the state changes there and the lanes behind
//                      it look again: one round of loads per run of the path, not per frame.
// The kernel is latency-bound by construction: a frame is a barrier-separated reduction of a handful of instructions, and a frame
// depends on the one before.  Its measure is microseconds per frame, not bytes per second: 0.7 - 0.9 at K = 64, 1.2 - 1.4 at K = 1024,
// 3.0 - 3.2 at K = 4096 on one utterance of 20 000 units.
#include "zs_common.h"

// c_t = fl32(s + p) and d = fl32(c - m) are single roundings: nothing in this file may be fused into a multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int SEG_MAX_BLOCKS = 256 * 4;

__device__ __forceinline__ uint32_t seg_ord(float s) {           // vq_ord: unsigned order = float order, NaN above +inf
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float seg_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

template <int CTRL> __device__ __forceinline__ uint64_t seg_dpp(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, false);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t seg_min(uint64_t a, uint64_t b) { return b < a ? b : a; }

// the least word of the wave, in every lane
__device__ __forceinline__ uint64_t seg_wave_min(uint64_t v) {
  v = seg_min(v, seg_dpp<0xB1>(v));                               // quad_perm [1, 0, 3, 2]
  v = seg_min(v, seg_dpp<0x4E>(v));                               // quad_perm [2, 3, 0, 1]: a quad agrees
  v = seg_min(v, seg_dpp<0x141>(v));                              // row_half_mirror: 8 lanes agree
  v = seg_min(v, seg_dpp<0x140>(v));                              // row_mirror: a row of 16 agrees
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), o, 64), lo = __shfl_xor((uint32_t)v, o, 64);
    v = seg_min(v, ((uint64_t)hi << 32) | lo);
  }
  return v;
}

template <int NS, int NW> __global__ void __launch_bounds__(64 * NW) seg_viterbi_kernel(const ZsSegViterbi p, const float lam) {
  constexpr int NT = 64 * NW;
  __shared__ unsigned long long s_key[2][NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = (p.K + 63) >> 6;
  unsigned long long* bits = static_cast<unsigned long long*>(p.work);
  int32_t* wa = reinterpret_cast<int32_t*>(bits + p.n_units * W);
  bool live[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) live[j] = tid + NT * j < p.K;
  int par = 0;                                                    // the LDS slot of the next reduction
  for (int64_t u = blockIdx.x; u < p.n_utt; u += gridDim.x) {
    const int64_t u0 = p.uoffs[u], u1 = p.uoffs[u + 1], T = u1 - u0;
    if (u0 < 0 || u1 > p.n_units || T < 0) {                      // not a range of units: nothing of it is touched
      if (tid == 0) {
        atomicAdd(p.bad, 1);
        if (p.n_seg) p.n_seg[u] = 0;
        if (p.cost) p.cost[u] = 0.0;
      }
      continue;
    }
    if (T == 0) {
      if (tid == 0) {
        if (p.n_seg) p.n_seg[u] = 0;
        if (p.cost) p.cost[u] = 0.0;
      }
      continue;
    }
    if (p.row) {                                                  // every score row of the utterance, before one is used
      int out = 0;
      for (int64_t t = tid; t < T; t += NT) {
        const int64_t r = p.row[u0 + t];
        out |= r < 0 || r >= p.n_rows;
      }
      if (__syncthreads_or(out)) {
        for (int64_t t = tid; t < T; t += NT) p.idx[u0 + t] = -1;
        if (tid == 0) {
          atomicAdd(p.bad, 1);
          if (p.n_seg) p.n_seg[u] = 0;
          if (p.cost) p.cost[u] = 0.0;
        }
        continue;
      }
    }
    float c[NS], sn[NS];
    {
      const float* s0 = p.scores + (p.row ? p.row[u0] : u0) * p.ld_s;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const float v = live[j] ? s0[tid + NT * j] : 0.f;
        c[j] = v == 0.f ? 0.f : v;                                // one zero: -0 and +0 are one cost, the lowest k takes it
      }
    }
    int64_t r_next = T > 1 ? (p.row ? p.row[u0 + 1] : u0 + 1) : 0;
    double cost = 0.0;
    int a = 0;
    for (int64_t t = 0; t < T; ++t) {
      const bool more = t + 1 < T;
      if (more) {                                                 // frame t + 1 does not wait for the reduction of frame t
        const float* s1 = p.scores + r_next * p.ld_s;
#pragma unroll
        for (int j = 0; j < NS; ++j) sn[j] = live[j] ? s1[tid + NT * j] : 0.f;
        r_next = t + 2 < T ? (p.row ? p.row[u0 + t + 2] : u0 + t + 2) : 0;
      }
      uint64_t key = ~(uint64_t)0;
#pragma unroll
      for (int j = 0; j < NS; ++j)
        if (live[j]) key = seg_min(key, ((uint64_t)seg_ord(c[j]) << 32) | (uint32_t)(tid + NT * j));
      key = seg_wave_min(key);
      if (NW > 1) {
        if (lane == 0) s_key[par][wave] = key;
        __syncthreads();                                          // the other slot is free again once every wave is past this one
#pragma unroll
        for (int w = 0; w < NW; ++w) key = seg_min(key, (uint64_t)s_key[par][w]);
        par ^= 1;
      }
      const float m = seg_unord((uint32_t)(key >> 32));
      a = (int)(uint32_t)key;
      cost += (double)m;
      if (tid == 0) wa[u0 + t] = a;
      if (more) {
        unsigned long long mine = 0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          const int k = tid + NT * j;
          const float d = c[j] - m;
          const bool stay = d < lam || (d == lam && k <= a);      // (d, k) against (lambda, a), lexicographic
          const unsigned long long b = __ballot(live[j] && !stay);
          if (lane == j) mine = b;
          c[j] = sn[j] + (stay ? d : lam);
        }
        if (lane < NS && NW * lane + wave < W) bits[(u0 + t + 1) * W + NW * lane + wave] = mine;
      }
    }
    if (tid == 0) {
      if (p.cost) p.cost[u] = cost;
    }
    __threadfence_block();
    __syncthreads();                                              // the bits and a_t of every wave are written
    if (wave == 0) {
      int k = a, nseg = 1;
      for (int64_t tb = T - 1; tb >= 1; tb -= 64) {               // lane l looks at frame tb - l
        const int64_t t = tb - lane;
        const bool valid = t >= 1;
        const int a_prev = valid ? wa[u0 + t - 1] : 0;
        int pos = 0;                                              // the lanes below pos have their state
        while (pos < 64) {
          const bool mineq = valid && lane >= pos;
          const unsigned long long word = mineq ? bits[(u0 + t) * W + (k >> 6)] : 0;
          const unsigned long long sw = __ballot(mineq && ((word >> (k & 63)) & 1));
          const int first = sw ? __ffsll((long long)sw) - 1 : 64;
          if (mineq && lane <= first) p.idx[u0 + t] = k;
          if (first == 64) break;
          const int nk = __shfl(a_prev, first, 64);
          nseg += nk != k;
          k = nk;
          pos = first + 1;
        }
      }
      if (lane == 0) {
        p.idx[u0] = k;
        if (p.n_seg) p.n_seg[u] = nseg;
      }
    }
    if (NW > 1) __syncthreads();                                  // wa and bits of this utterance are read before the next one starts
  }
}

template <int NW> void seg_launch(const ZsSegViterbi& p, int ns, unsigned grid, hipStream_t st) {
  const dim3 g(grid), b(64 * NW);
  const float lam = p.lam == 0.f ? 0.f : p.lam;                   // -0 is 0
  if (ns <= 1) hipLaunchKernelGGL((seg_viterbi_kernel<1, NW>), g, b, 0, st, p, lam);
  else if (ns <= 2) hipLaunchKernelGGL((seg_viterbi_kernel<2, NW>), g, b, 0, st, p, lam);
  else if (ns <= 4) hipLaunchKernelGGL((seg_viterbi_kernel<4, NW>), g, b, 0, st, p, lam);
  else if (ns <= 8) hipLaunchKernelGGL((seg_viterbi_kernel<8, NW>), g, b, 0, st, p, lam);
  else hipLaunchKernelGGL((seg_viterbi_kernel<16, NW>), g, b, 0, st, p, lam);
}

inline bool seg_misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

}  // namespace

extern "C" int zs_seg_viterbi(const ZsSegViterbi* p, void* stream) {
  ZS_REQUIRE(p, "zs_seg_viterbi: null argument");
  ZS_REQUIRE(p->K >= 1 && p->K <= ZS_SEG_MAX_K, "zs_seg_viterbi: K must be in [1, %d] (got %d)", ZS_SEG_MAX_K, p->K);
  ZS_REQUIRE(p->n_units >= 0 && p->n_units <= 0x7fffffff && p->n_utt >= 0 && p->n_utt <= 0x7fffffff && p->n_rows >= 0 &&
                 p->n_rows <= 0x7fffffff, "zs_seg_viterbi: n_units, n_utt and n_rows must be in [0, 2^31) (got %lld, %lld, %lld)",
             (long long)p->n_units, (long long)p->n_utt, (long long)p->n_rows);
  ZS_REQUIRE(p->ld_s >= p->K, "zs_seg_viterbi: ld_s %lld is below K %d", (long long)p->ld_s, p->K);
  ZS_REQUIRE(p->lam >= 0.f && p->lam <= 3.402823466e38f, "zs_seg_viterbi: lambda must be finite and >= 0 (got %g)", (double)p->lam);
  ZS_REQUIRE(p->work_bytes >= 0, "zs_seg_viterbi: work_bytes must be >= 0");
  ZS_REQUIRE(p->row || p->n_rows >= p->n_units, "zs_seg_viterbi: without `row`, unit i is score row i: n_rows %lld is below n_units %lld",
             (long long)p->n_rows, (long long)p->n_units);
  if (p->n_utt == 0) return ZS_OK;
  ZS_REQUIRE(p->uoffs && p->bad, "zs_seg_viterbi: null operand");
  ZS_REQUIRE(p->n_units == 0 || (p->scores && p->idx && p->work), "zs_seg_viterbi: null operand");
  ZS_REQUIRE(!seg_misaligned(p->scores, 4) && !seg_misaligned(p->uoffs, 8) && !seg_misaligned(p->row, 8) && !seg_misaligned(p->idx, 4) &&
                 !seg_misaligned(p->n_seg, 4) && !seg_misaligned(p->cost, 8) && !seg_misaligned(p->bad, 4) && !seg_misaligned(p->work, 8),
             "zs_seg_viterbi: an operand is not aligned to its element (work: 8 bytes)");
  ZS_REQUIRE(p->work_bytes >= ZS_SEG_WORK_BYTES(p->n_units, p->K), "zs_seg_viterbi: the workspace holds %lld bytes, %lld units of K = %d "
             "need %lld (ZS_SEG_WORK_BYTES)", (long long)p->work_bytes, (long long)p->n_units, p->K,
             (long long)ZS_SEG_WORK_BYTES(p->n_units, p->K));
  const unsigned grid = (unsigned)(p->n_utt < SEG_MAX_BLOCKS ? p->n_utt : SEG_MAX_BLOCKS);
  const hipStream_t st = (hipStream_t)stream;
  if (p->K <= 64) seg_launch<1>(*p, 1, grid, st);
  else seg_launch<4>(*p, (p->K + 255) / 256, grid, st);
  return zs_check_launch("zs_seg_viterbi");
}

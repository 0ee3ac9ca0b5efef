// zs_vq_train.hip -- training a 'continues' model through its vector codebook (include/zs_amd.h): the straight-through
// quantiser and the commitment loss (zs_vq_commit), their gradient (zs_vq_st_bwd) and the exponential moving average that moves the
// codebook after the encoder (zs_vq_ema).  All three are memory-bound and row-parallel; nothing here adds floats atomically, so a
// step is bitwise reproducible.
//   vq_commit_kernel    a row of z is owned by a team of 2^t <= 64 lanes of one wave, one 16-byte piece of q per lane and round: the
//                       lanes of a team read consecutive pieces of z and of the one codeword row (contiguous, read once per row).  The
//                       row's magnitude check is an OR over the team by shuffles.  Every lane keeps one double of squared residuals;
//                       a workgroup's sum goes to partial[workgroup] and vq_commit_finish_kernel adds the partials.
//   vq_st_bwd_kernel    one lane per 16-byte piece of dz, grid-stride.
//   vq_ema_kernel       one workgroup per codeword, as vq_update_kernel (the same order of the norm's sum).
//   vq_restart_*        zs_vq_restart: one workgroup ranks the dead codewords, then one workgroup per dead codeword copies
//                       an encoder row over it, as vq_ema_kernel is laid out.
// The piece store, the hash of the restart's draw and the teams' launch arithmetic are zs_quant.h's; vt_load and vt_load_code stay here
// (their early return for a piece at or above E is part of vq_commit_kernel's and vq_st_bwd_kernel's instruction streams).
#include "zs_quant.h"

// the definitions are stated operation by operation (a rounding each): nothing in this file may be fused into a multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int VT_NT = 256;

// the columns c .. c + PER - 1 of a row as fp32 (PER = 16 / sizeof(T)); those at or above E read nothing and are zero
template <typename T> __device__ __forceinline__ void vt_load(const T* row, int c, int E, bool vec, float (&v)[8]);
template <> __device__ __forceinline__ void vt_load<float>(const float* row, int c, int E, bool vec, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (c >= E) return;
  if (vec && c + 4 <= E) {
    const float4 a = *reinterpret_cast<const float4*>(row + c);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c + i < E) v[i] = row[c + i];
}
template <> __device__ __forceinline__ void vt_load<bf16_t>(const bf16_t* row, int c, int E, bool vec, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (c >= E) return;
  if (vec && c + 8 <= E) {
    load8<bf16_t>(row + c, v);
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (c + i < E) v[i] = bf2f(row[c + i]);
}
// per columns (4 or 8) of a codeword row
template <int PER> __device__ __forceinline__ void vt_load_code(const float* row, int c, int E, bool vec, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (c >= E) return;
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

// ---- commit ------------------------------------------------------------------------------------------------------------------------
template <typename T> __global__ void __launch_bounds__(VT_NT)
vq_commit_kernel(const ZsVqCommit p, const int tl, const int groups, const int zvec, const int cvec, const int fvec) {
  constexpr int PER = 16 / (int)sizeof(T);
  __shared__ double s_part[VT_NT / 64];
  const int tid = threadIdx.x, tlane = tid & (tl - 1);
  const int64_t n_teams = (int64_t)gridDim.x * (VT_NT / tl);
  const int64_t team = (int64_t)blockIdx.x * (VT_NT / tl) + tid / tl;
  const int64_t rounds = (p.n + n_teams - 1) / n_teams;          // the same for every lane: the shuffles below see whole waves
  const T* z = static_cast<const T*>(p.z);
  T* q = static_cast<T*>(p.q);
  double acc = 0.0;
  int bad = 0, over = 0;
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t row = team + r * n_teams;
    const bool live = row < p.n;
    const int k = live ? p.idx[row] : 0;
    const bool ok = live && k >= 0 && k < p.K;                    // else never an index: a zero row, left out of the loss
    int big = 0;
    if (live) {
      const T* zr = z + row * p.ld_z;
      const float* cr = p.code + (int64_t)(ok ? k : 0) * p.ld_code;
      for (int g = tlane; g < groups; g += tl) {
        const int c = PER * g;
        float zv[8], cv[8], qv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        vt_load<T>(zr, c, p.E, zvec != 0, zv);
        if (ok) {
          vt_load_code<PER>(cr, c, p.E, cvec != 0, cv);
#pragma unroll
          for (int j = 0; j < PER; ++j)
            if (c + j < p.E) {
              qv[j] = cv[j];
              const double d = (double)zv[j] - (double)cv[j];
              acc += d * d;
            }
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) big |= !(fabsf(zv[j]) < (float)ZS_VQ_MAX_ABS);        // (NaN: not below)
        q_store_piece<T>(q + row * p.ld_q + c, qv);
        if (p.z_f32 && c < p.E) {
          float* fr = p.z_f32 + row * p.ld_zf + c;
          if (fvec && c + PER <= p.E) {
            *reinterpret_cast<float4*>(fr) = make_float4(zv[0], zv[1], zv[2], zv[3]);
            if (PER == 8) *reinterpret_cast<float4*>(fr + 4) = make_float4(zv[4], zv[5], zv[6], zv[7]);
          } else {
#pragma unroll
            for (int j = 0; j < PER; ++j)
              if (c + j < p.E) fr[j] = zv[j];
          }
        }
      }
    }
    for (int o = 1; o < tl; o <<= 1) big |= __shfl_xor(big, o, 64);                          // over the team
    if (live && tlane == 0) {
      bad += !ok;
      over += big;
      if (p.idx_acc) p.idx_acc[row] = (ok && !big) ? k : -1;
    }
  }
  if (p.loss) {
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) p.partial[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
  }
  if (bad) atomicAdd(p.bad, bad);
  if (over && p.over) atomicAdd(p.over, over);
}

__global__ void __launch_bounds__(VT_NT) vq_commit_finish_kernel(const double* partial, const int parts, const double scale, float* loss) {
  __shared__ double s_part[VT_NT / 64];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < parts; i += VT_NT) s += partial[i];
  s = wave_sum_d(s);
  if ((tid & 63) == 0) s_part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) *loss = (float)(scale * (s_part[0] + s_part[1] + s_part[2] + s_part[3]));
}

// ---- straight-through backward ---------------------------------------------------------------------------------------------------------
template <typename T> __global__ void __launch_bounds__(VT_NT)
vq_st_bwd_kernel(const ZsVqStBwd p, const int groups, const int zvec, const int cvec) {
  constexpr int PER = 16 / (int)sizeof(T);
  const int64_t total = p.n * groups;
  const int64_t nthr = (int64_t)gridDim.x * VT_NT;
  const T* dq = static_cast<const T*>(p.dq);
  const T* z = static_cast<const T*>(p.z);
  T* dz = static_cast<T*>(p.dz);
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * VT_NT + threadIdx.x; i < total; i += nthr) {
    const int64_t row = i / groups;
    const int g = (int)(i - row * groups), c = PER * g;
    float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < p.E) {
      float dv[8], zv[8], cv[8];
      vt_load<T>(dq + row * p.ld_dq, c, p.E, true, dv);          // (dq is 16-byte aligned at a pitch of whole pieces)
      const int k = p.idx[row];
      if (k < 0 || k >= p.K) {                                    // never an index: the gradient passes through
        bad += g == 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) out[j] = dv[j];
      } else {
        vt_load<T>(z + row * p.ld_z, c, p.E, zvec != 0, zv);
        vt_load_code<PER>(p.code + (int64_t)k * p.ld_code, c, p.E, cvec != 0, cv);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const float d = zv[j] - cv[j];                          // three fp32 operations, a rounding each (contract off)
          const float t = p.g * d;
          out[j] = c + j < p.E ? dv[j] + t : 0.f;
        }
      }
    }
    q_store_piece<T>(dz + row * p.ld_dz + c, out);
  }
  if (bad) atomicAdd(p.bad, bad);
}

// ---- codebook EMA ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VT_NT) vq_ema_kernel(const ZsVqEma p, const double keep, const double inv_scale) {
  __shared__ double s_part[VT_NT / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int c = p.cnt[k];
  const float n_new = (float)(p.decay * (double)p.N[k] + keep * (double)c);
  const bool live = (double)n_new >= 1e-3;
  float* row = p.code + (int64_t)k * p.ld_code;
  float* m = p.m + (int64_t)k * p.E;
  const int64_t* sum = p.sum + (int64_t)k * p.E;
  double sq = 0.0;
  for (int j = tid; j < p.E; j += VT_NT) {
    const float m_new = (float)(p.decay * (double)m[j] + keep * (double)sum[j] * inv_scale);
    m[j] = m_new;
    float v = row[j];
    if (live) {
      v = (float)((double)m_new / (double)n_new);
      row[j] = v;
    }
    sq += (double)v * (double)v;
  }
  sq = wave_sum_d(sq);
  if ((tid & 63) == 0) s_part[tid >> 6] = sq;
  __syncthreads();                                                // every lane has read N[k]
  if (tid == 0) {
    p.N[k] = n_new;
    p.cnorm[k] = (float)(s_part[0] + s_part[1] + s_part[2] + s_part[3]);
    if (p.used && c > 0) atomicAdd(p.used, 1);
  }
}

// ---- restart of dead codewords ---------------------------------------------------------------------------------------------
constexpr int VR_MAX_WG = 1024;                                   // workgroups of the copy: more dead codewords than that stride

// One workgroup ranks the K flags: a coalesced pass leaves them as 64-bit ballots in LDS (K / 64 <= 1024 words), lane t owns the
// contiguous words [t wp, (t + 1) wp), counts them, the counts are scanned over the wave and then over the four waves, and every lane
// writes the k of its dead codewords to work[rank].  work[K] = the number of dead codewords.
__global__ void __launch_bounds__(VT_NT) vq_restart_rank_kernel(const ZsVqRestart p) {
  __shared__ unsigned long long s_bits[ZS_CODE_MAX_K / 64];
  __shared__ int s_wave[VT_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll 4
  for (int base = 0; base < p.K; base += VT_NT) {                 // (the same trip count for every lane: the ballot sees whole waves)
    const int k = base + tid;
    bool dead = false;
    if (k < p.K) {
      const int c = p.cnt[k];
      const float n = p.N[k];
      dead = c == 0 && n < p.thresh;                              // (NaN: not below)
    }
    const unsigned long long b = __ballot(dead);
    if (lane == 0) s_bits[(base >> 6) + (tid >> 6)] = b;
  }
  __syncthreads();
  const int words = (p.K + 63) >> 6, wp = (words + VT_NT - 1) / VT_NT;
  const int lo = tid * wp < words ? tid * wp : words, hi = lo + wp < words ? lo + wp : words;
  int mine = 0;
  for (int w = lo; w < hi; ++w) mine += __popcll(s_bits[w]);
  int inc = mine;                                                 // inclusive over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) s_wave[tid >> 6] = inc;
  __syncthreads();
  int rank = inc - mine;
  for (int w = 0; w < (tid >> 6); ++w) rank += s_wave[w];
  for (int w = lo; w < hi; ++w) {
    unsigned long long b = s_bits[w];
    while (b) {
      p.work[rank++] = (w << 6) + (__ffsll(b) - 1);
      b &= b - 1;
    }
  }
  if (tid == VT_NT - 1) p.work[p.K] = rank;                       // (the last lane's rank behind its own words: all of them)
}

// One workgroup per dead codeword, laid out as vq_ema_kernel (the same order of the norm's sum).
__global__ void __launch_bounds__(VT_NT) vq_restart_copy_kernel(const ZsVqRestart p) {
  __shared__ double s_part[VT_NT / 64];
  const int tid = threadIdx.x;
  const int dead = p.work[p.K];
  if ((int)blockIdx.x >= dead) return;                            // the usual case: nothing is written
  const uint64_t n = (uint64_t)p.n;
  const uint64_t start = q_mix64(p.seed + (p.seed_ptr ? *p.seed_ptr : 0ull) + 0x5651524553544152ull) % n;
  for (int j = blockIdx.x; j < dead; j += gridDim.x) {
    const int k = p.work[j];
    const int64_t r = (int64_t)((start + ((uint64_t)j % n) * (uint64_t)p.stride) % n);
    if (p.idx_acc && p.idx_acc[r] < 0) {                          // left out of the average for its magnitude (the whole workgroup agrees)
      if (tid == 0) atomicAdd(p.skipped, 1);
      continue;
    }
    const float* xr = p.x + r * p.ld_x;
    float* row = p.code + (int64_t)k * p.ld_code;
    float* m = p.m + (int64_t)k * p.E;
    double sq = 0.0;
    for (int e = tid; e < p.E; e += VT_NT) {
      const float v = xr[e];
      row[e] = v;
      m[e] = v;
      sq += (double)v * (double)v;
    }
    sq = wave_sum_d(sq);
    if ((tid & 63) == 0) s_part[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
      p.N[k] = 1.f;
      p.cnorm[k] = (float)(s_part[0] + s_part[1] + s_part[2] + s_part[3]);
      atomicAdd(p.restarted, 1);
    }
    __syncthreads();                                              // s_part is written again in the next round
  }
}

const char* vt_shape(int K, int E, int64_t n, int64_t ld_a, int64_t ld_b, int64_t ld_c) {
  if (K < 1 || K > ZS_CODE_MAX_K) return "K must be in [1, 65536]";
  if (E < 1 || E > ZS_CODE_MAX_E) return "E must be in [1, 1024]";
  if (n < 0 || n > 0x7fffffff) return "n must be in [0, 2^31)";
  if (ld_a < E || ld_b < E || ld_c < E) return "a leading dimension is below E";
  return nullptr;
}

}  // namespace

extern "C" int zs_vq_commit(const ZsVqCommit* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_commit: null argument");
  const char* why = vt_shape(p->K, p->E, p->n, p->ld_z, p->ld_code, p->ld_q);
  ZS_REQUIRE(!why, "zs_vq_commit: %s (n %lld, K %d, E %d, ld_z %lld, ld_code %lld, ld_q %lld)", why, (long long)p->n, p->K, p->E,
             (long long)p->ld_z, (long long)p->ld_code, (long long)p->ld_q);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_vq_commit: bad dtype");
  ZS_REQUIRE(p->ld_q % 8 == 0, "zs_vq_commit: ld_q must be a multiple of 8 (got %lld)", (long long)p->ld_q);
  ZS_REQUIRE(!p->z_f32 || p->ld_zf >= p->E, "zs_vq_commit: a leading dimension is below E (ld_zf %lld, E %d)", (long long)p->ld_zf, p->E);
  ZS_REQUIRE(!p->loss == !p->partial, "zs_vq_commit: loss and partial go together");
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->z && p->idx && p->code && p->q && p->bad, "zs_vq_commit: null operand");
  const uintptr_t es = p->dtype == ZS_F32 ? 4 : 2;
  ZS_REQUIRE(!misaligned(p->z, es) && !misaligned(p->idx, 4) && !misaligned(p->code, 4) && !misaligned(p->q, 16) && !misaligned(p->z_f32, 4) &&
                 !misaligned(p->idx_acc, 4) && !misaligned(p->partial, 8) && !misaligned(p->loss, 4) && !misaligned(p->bad, 4) &&
                 !misaligned(p->over, 4), "zs_vq_commit: an operand is misaligned (q: 16 bytes)");
  ZS_REQUIRE(!p->idx_acc || p->idx_acc != p->idx, "zs_vq_commit: idx_acc must not be idx");
  const int per = 16 / (int)es;
  const int groups = (int)(p->ld_q / per), tl = team_lanes(groups);
  const int zvec = !misaligned(p->z, 16) && p->ld_z % per == 0;
  const int cvec = !misaligned(p->code, 16) && p->ld_code % 4 == 0;
  const int fvec = p->z_f32 && !misaligned(p->z_f32, 16) && p->ld_zf % 4 == 0;
  const unsigned wgs = team_wgs(p->n, tl, VT_NT, ZS_VQ_COMMIT_PARTS);
  const hipStream_t st = (hipStream_t)stream;
  if (p->dtype == ZS_F32)
    hipLaunchKernelGGL(vq_commit_kernel<float>, dim3(wgs), dim3(VT_NT), 0, st, *p, tl, groups, zvec, cvec, fvec);
  else
    hipLaunchKernelGGL(vq_commit_kernel<bf16_t>, dim3(wgs), dim3(VT_NT), 0, st, *p, tl, groups, zvec, cvec, fvec);
  if (p->loss) hipLaunchKernelGGL(vq_commit_finish_kernel, dim3(1), dim3(VT_NT), 0, st, p->partial, (int)wgs, p->scale, p->loss);
  return zs_check_launch("zs_vq_commit");
}

extern "C" int zs_vq_st_bwd(const ZsVqStBwd* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_st_bwd: null argument");
  const char* why = vt_shape(p->K, p->E, p->n, p->ld_z, p->ld_code, p->ld_dq < p->ld_dz ? p->ld_dq : p->ld_dz);
  ZS_REQUIRE(!why, "zs_vq_st_bwd: %s (n %lld, K %d, E %d, ld_dq %lld, ld_z %lld, ld_code %lld, ld_dz %lld)", why, (long long)p->n, p->K, p->E,
             (long long)p->ld_dq, (long long)p->ld_z, (long long)p->ld_code, (long long)p->ld_dz);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_vq_st_bwd: bad dtype");
  ZS_REQUIRE(p->ld_dq % 8 == 0 && p->ld_dz % 8 == 0, "zs_vq_st_bwd: ld_dq and ld_dz must be multiples of 8 (got %lld, %lld)",
             (long long)p->ld_dq, (long long)p->ld_dz);
  ZS_REQUIRE(!p->dq || p->dq != p->dz || p->ld_dq == p->ld_dz, "zs_vq_st_bwd: in place (dz == dq) needs ld_dz == ld_dq");
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->dq && p->z && p->idx && p->code && p->dz && p->bad, "zs_vq_st_bwd: null operand");
  const uintptr_t es = p->dtype == ZS_F32 ? 4 : 2;
  ZS_REQUIRE(!misaligned(p->dq, 16) && !misaligned(p->dz, 16) && !misaligned(p->z, es) && !misaligned(p->idx, 4) && !misaligned(p->code, 4) &&
                 !misaligned(p->bad, 4), "zs_vq_st_bwd: an operand is misaligned (dq, dz: 16 bytes)");
  const int per = 16 / (int)es;
  const int groups = (int)(p->ld_dz / per);
  const int zvec = !misaligned(p->z, 16) && p->ld_z % per == 0;
  const int cvec = !misaligned(p->code, 16) && p->ld_code % 4 == 0;
  int64_t wgs = (p->n * groups + VT_NT - 1) / VT_NT;
  wgs = wgs > 2048 ? 2048 : wgs;
  const hipStream_t st = (hipStream_t)stream;
  if (p->dtype == ZS_F32)
    hipLaunchKernelGGL(vq_st_bwd_kernel<float>, dim3((unsigned)wgs), dim3(VT_NT), 0, st, *p, groups, zvec, cvec);
  else
    hipLaunchKernelGGL(vq_st_bwd_kernel<bf16_t>, dim3((unsigned)wgs), dim3(VT_NT), 0, st, *p, groups, zvec, cvec);
  return zs_check_launch("zs_vq_st_bwd");
}

extern "C" int zs_vq_ema(const ZsVqEma* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_ema: null argument");
  const char* why = vt_shape(p->K, p->E, 0, p->ld_code, p->E, p->E);
  ZS_REQUIRE(!why, "zs_vq_ema: %s (K %d, E %d, ld_code %lld)", why, p->K, p->E, (long long)p->ld_code);
  ZS_REQUIRE(p->shift >= -64 && p->shift <= 62, "zs_vq_ema: shift must be in [-64, 62] (got %d)", p->shift);
  ZS_REQUIRE(p->decay >= 0.0 && p->decay < 1.0, "zs_vq_ema: decay must be in [0, 1) (got %g)", p->decay);
  ZS_REQUIRE(p->cnt && p->sum && p->N && p->m && p->code && p->cnorm, "zs_vq_ema: null operand");
  ZS_REQUIRE(!misaligned(p->cnt, 4) && !misaligned(p->sum, 8) && !misaligned(p->N, 4) && !misaligned(p->m, 4) && !misaligned(p->code, 4) &&
                 !misaligned(p->cnorm, 4) && !misaligned(p->used, 4), "zs_vq_ema: an operand is not aligned to its element");
  hipLaunchKernelGGL(vq_ema_kernel, dim3((unsigned)p->K), dim3(VT_NT), 0, (hipStream_t)stream, *p, 1.0 - p->decay, ldexp(1.0, -p->shift));
  return zs_check_launch("zs_vq_ema");
}

extern "C" int zs_vq_restart(const ZsVqRestart* p, void* stream) {
  ZS_REQUIRE(p, "zs_vq_restart: null argument");
  const char* why = vt_shape(p->K, p->E, p->n, p->ld_x, p->ld_code, p->E);
  ZS_REQUIRE(!why, "zs_vq_restart: %s (n %lld, K %d, E %d, ld_x %lld, ld_code %lld)", why, (long long)p->n, p->K, p->E, (long long)p->ld_x,
             (long long)p->ld_code);
  ZS_REQUIRE(p->thresh > 0.f && p->thresh < 1.f, "zs_vq_restart: thresh must be in (0, 1) (got %g)", (double)p->thresh);
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->stride >= 1 && p->stride <= p->n, "zs_vq_restart: stride must be in [1, n] (got %d, n %lld)", p->stride, (long long)p->n);
  ZS_REQUIRE(p->x && p->cnt && p->N && p->m && p->code && p->cnorm && p->work && p->restarted && p->skipped, "zs_vq_restart: null operand");
  ZS_REQUIRE(!misaligned(p->x, 4) && !misaligned(p->idx_acc, 4) && !misaligned(p->cnt, 4) && !misaligned(p->N, 4) && !misaligned(p->m, 4) &&
                 !misaligned(p->code, 4) && !misaligned(p->cnorm, 4) && !misaligned(p->seed_ptr, 8) && !misaligned(p->work, 4) &&
                 !misaligned(p->restarted, 4) && !misaligned(p->skipped, 4), "zs_vq_restart: an operand is not aligned to its element");
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(vq_restart_rank_kernel, dim3(1), dim3(VT_NT), 0, st, *p);
  hipLaunchKernelGGL(vq_restart_copy_kernel, dim3((unsigned)(p->K < VR_MAX_WG ? p->K : VR_MAX_WG)), dim3(VT_NT), 0, st, *p);
  return zs_check_launch("zs_vq_restart");
}

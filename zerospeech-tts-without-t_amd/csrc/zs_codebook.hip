// zs_codebook.hip -- the unit codebook (include/zs_amd.h): nearest codeword in Hamming distance over bit-packed units
// (zs_code_assign) and the two halves of a k-modes iteration around it (zs_code_accum, zs_code_update).  Rows are zs_units_pack's:
// bit j of byte b is column 8b + j, so dword i of a row, read little-endian, holds columns 32i .. 32i + 31 with column c at bit c % 32.
//   code_assign_kernel  one unit row per lane in registers (W dwords, W the next power of two of ceil(E / 32); R rows per lane).  The
//                       codewords pass through LDS, ZS_CODE_TILE_WORDS dwords at a time, already masked to the columns < E; every
//                       lane of a wave reads the same codeword address (a broadcast: no bank conflict) and pays W xor + W popcount
//                       per codeword and row, so with R = 2 one 16-byte LDS read serves eight of them and the LDS array stays
//                       under half of what the four SIMDs could ask of it.  The running best is ONE word, (dist << 16) | k, kept by
//                       an unsigned min: dist <= 1024 and k < 65536 fit, and the least word is the least distance at the lowest
//                       index whatever the order the codewords come in -- the tie rule survives tiling over K and the split below.
//                       S > 1 (few rows, an inference chunk): the S waves of a workgroup hold the SAME 64 rows and take an S-th of
//                       every pass each; their words meet in LDS and wave 0 writes the results.
//   code_scores_kernel  zs_code_scores (--segment): the same rows in registers and the same LDS tiles (stage_codes, one function for
//                       both), every distance written as fp32 instead of reduced.
//   code_accum_kernel   a workgroup owns a tile of codewords (those whose counters, KT x E int32, fit 64 KiB of LDS) and a slice of
//                       the rows.  It scans its slice of idx, lists the rows of its codewords and adds their bits to the LDS
//                       counters (one lane per byte of a row), then adds the non-zero counters to `ones` and `cnt` with integer
//                       atomics: K x E x slices global atomics instead of one per set bit, and none of them contended.
//   code_update_kernel  one workgroup per codeword, one lane per byte.
#include "zs_common.h"

namespace {

constexpr int TILE_WORDS = ZS_CODE_TILE_WORDS;

// dword i of a packed row whose first nbytes bytes carry columns; bytes from nbytes on are never read and count as zero
__device__ __forceinline__ uint32_t row_word(const uint8_t* p, int i, int nbytes, bool al4) {
  const int b = 4 * i;
  if (al4 && b + 4 <= nbytes) return *reinterpret_cast<const uint32_t*>(p + b);
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (b + j < nbytes) w |= (uint32_t)p[b + j] << (8 * j);
  return w;
}
__device__ __forceinline__ void put_word(uint8_t* p, int i, int nbytes, bool al4, uint32_t w) {
  const int b = 4 * i;
  if (al4 && b + 4 <= nbytes) {
    *reinterpret_cast<uint32_t*>(p + b) = w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (b + j < nbytes) p[b + j] = (uint8_t)(w >> (8 * j));
}
// the columns < E of dword i
__device__ __forceinline__ uint32_t word_mask(int i, int E) {
  const int full = E >> 5;
  return i < full ? 0xffffffffu : (i == full ? ((1u << (E & 31)) - 1u) : 0u);
}

// a row into W registers, masked.  mode 2: 16-byte loads (row 16-byte aligned, nbytes a multiple of 16), 1: dwords, 0: bytes
template <int W> __device__ __forceinline__ void load_row(const uint8_t* p, int nbytes, int E, int mode, uint32_t (&u)[W]) {
  if (W >= 4 && mode == 2) {
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (16 * q + 16 <= nbytes) v = *reinterpret_cast<const uint4*>(p + 16 * q);
      u[4 * q] = v.x; u[4 * q + 1] = v.y; u[4 * q + 2] = v.z; u[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < W; ++i) u[i] = row_word(p, i, nbytes, mode != 0);
  }
#pragma unroll
  for (int i = 0; i < W; ++i) u[i] &= word_mask(i, E);
}

// dst row = src row over the columns < E (the bytes that carry columns; those behind them are left alone)
template <int W> __device__ __forceinline__ void copy_row(uint8_t* dst, int dmode, const uint8_t* src, int smode, int nbytes, int E) {
  uint32_t c[W];
  load_row<W>(src, nbytes, E, smode, c);
  if (W >= 4 && dmode == 2) {
#pragma unroll
    for (int q = 0; q < W / 4; ++q)
      if (16 * q + 16 <= nbytes) *reinterpret_cast<uint4*>(dst + 16 * q) = make_uint4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < W; ++i) put_word(dst, i, nbytes, dmode != 0, c[i]);
  }
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// THE codeword tiling of zs_code_assign and zs_code_scores: the codewords k0 .. k0 + nk - 1, W dwords each and masked to the columns
// < E, into s_code; between two barriers (the pass before has been read; the first time, every row is loaded)
template <int W, int NT>
__device__ __forceinline__ void stage_codes(uint32_t* s_code, const uint8_t* code, int code_bytes, int k0, int nk, int nbytes, int E,
                                            int cmode) {
  __syncthreads();
  for (int i = threadIdx.x; i < nk * W; i += NT) {
    const int k = i / W, w = i & (W - 1);
    s_code[i] = row_word(code + (int64_t)(k0 + k) * code_bytes, w, nbytes, cmode != 0) & word_mask(w, E);
  }
  __syncthreads();
}

// zs_code_scores: code_assign_kernel's rows and passes (one row per lane, 256 lanes); the distances of 4 consecutive codewords leave
// as one 16-byte store where `vec` (scores 16-byte aligned, ld_s a multiple of 4; a pass starts at a multiple of 4 codewords).
template <int W> __global__ void __launch_bounds__(256) code_scores_kernel(const ZsCodeScores p, const int umode, const int cmode, const int vec) {
  constexpr int NT = 256, TK = TILE_WORDS / W;
  static_assert(TK % 4 == 0, "a pass starts at a multiple of 4 codewords");
  __shared__ __attribute__((aligned(16))) uint32_t s_code[TILE_WORDS];
  const int nbytes = (p.E + 7) >> 3;
  const int64_t row = (int64_t)blockIdx.x * NT + threadIdx.x;
  const bool live = row < p.n;
  uint32_t u[W];
  if (live) {
    load_row<W>(p.units + row * p.row_bytes, nbytes, p.E, umode, u);
  } else {
#pragma unroll
    for (int i = 0; i < W; ++i) u[i] = 0;
  }
  float* out = p.scores + (live ? row : 0) * p.ld_s;
  for (int k0 = 0; k0 < p.K; k0 += TK) {
    const int nk = p.K - k0 < TK ? p.K - k0 : TK;
    stage_codes<W, NT>(s_code, p.code, p.code_bytes, k0, nk, nbytes, p.E, cmode);
    if (!live) continue;
    for (int k = 0; k < nk; k += 4) {
      float d[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t s = 0;
        if (k + q < nk) {
          const uint32_t* c = s_code + (k + q) * W;
#pragma unroll
          for (int i = 0; i < W; ++i) s += __popc(u[i] ^ c[i]);
        }
        d[q] = (float)s;
      }
      if (vec && k + 4 <= nk) {
        *reinterpret_cast<float4*>(out + k0 + k) = make_float4(d[0], d[1], d[2], d[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (k + q < nk) out[k0 + k + q] = d[q];
      }
    }
  }
}

template <int W, int R, int S> __global__ void __launch_bounds__(S > 1 ? 64 * S : 256)
code_assign_kernel(const ZsCodeAssign p, const int umode, const int cmode) {
  static_assert(S == 1 || R == 1, "shared rows: one row per lane");
  constexpr int NT = S > 1 ? 64 * S : 256;
  constexpr int TK = TILE_WORDS / W;                              // codewords per pass
  __shared__ __attribute__((aligned(16))) uint32_t s_code[TILE_WORDS];
  __shared__ uint32_t s_key[S > 1 ? S * 64 : 1];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int nbytes = (p.E + 7) >> 3;
  const int64_t row0 = S > 1 ? (int64_t)blockIdx.x * 64 : ((int64_t)blockIdx.x * (NT / 64) + wave) * (64 * R);
  uint32_t u[R][W], best[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + 64 * r + lane;
    best[r] = 0xffffffffu;
    if (row < p.n) {
      load_row<W>(p.units + row * p.row_bytes, nbytes, p.E, umode, u[r]);
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) u[r][i] = 0;
    }
  }
  for (int k0 = 0; k0 < p.K; k0 += TK) {
    const int nk = p.K - k0 < TK ? p.K - k0 : TK;
    stage_codes<W, NT>(s_code, p.code, p.code_bytes, k0, nk, nbytes, p.E, cmode);
    int ka = 0, kb = nk;
    if (S > 1) {
      const int per = (nk + S - 1) / S;
      ka = wave * per < nk ? wave * per : nk;
      kb = ka + per < nk ? ka + per : nk;
    }
    for (int k = ka; k < kb; ++k) {
      const uint32_t* c = s_code + k * W;
      uint32_t d[R];
#pragma unroll
      for (int r = 0; r < R; ++r) d[r] = 0;
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const uint32_t cw = c[i];
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] += __popc(u[r][i] ^ cw);
      }
      const uint32_t kk = (uint32_t)(k0 + k);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t key = (d[r] << 16) | kk;
        best[r] = key < best[r] ? key : best[r];
      }
    }
  }
  if (S > 1) {
    s_key[wave * 64 + lane] = best[0];
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < S; ++w) {
      const uint32_t key = s_key[w * 64 + lane];
      best[0] = key < best[0] ? key : best[0];
    }
  }
  int sum = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + 64 * r + lane;
    if (row >= p.n) continue;
    const int k = (int)(best[r] & 0xffffu), d = (int)(best[r] >> 16);
    sum += d;
    if (p.idx) p.idx[row] = k;
    if (p.dist) p.dist[row] = d;
    if (p.snapped) copy_row<W>(p.snapped + row * p.row_bytes, umode, p.code + (int64_t)k * p.code_bytes, cmode, nbytes, p.E);
  }
  if (p.total) {
    sum = wave_sum_i(sum);                                        // <= 128 rows of <= 1024 each
    if (lane == 0 && sum) atomicAdd(reinterpret_cast<unsigned long long*>(p.total), (unsigned long long)sum);
  }
}

constexpr int ACC_NT = 256, ACC_PER = 4, ACC_CHUNK = ACC_NT * ACC_PER;          // idx entries a workgroup looks at per round
constexpr int ACC_WORDS = 16384, ACC_MAX_KT = 1024, ACC_BATCH = 4;              // 64 KiB of private counters

// Workgroup (x, y) owns the codewords [x KT, x KT + KT) and the rows [y slice, y slice + slice): their counters live in LDS.  Per round
// it reads ACC_CHUNK entries of idx, lists those of its codewords (a slot from an LDS counter), and then G lanes per listed row, one
// per byte, add the row's bits to the LDS counters; ACC_BATCH rows' bytes are loaded before the first is added.
__global__ void __launch_bounds__(ACC_NT) code_accum_kernel(const ZsCodeAccum p, const int KT, const int G, const int64_t slice) {
  __shared__ int s_ones[ACC_WORDS];
  __shared__ int s_cnt[ACC_MAX_KT];
  __shared__ int s_list[ACC_CHUNK];
  __shared__ int s_n;
  const int tid = threadIdx.x, nbytes = (p.E + 7) >> 3;
  const int k0 = blockIdx.x * KT, kt = p.K - k0 < KT ? p.K - k0 : KT;
  const int64_t r0 = (int64_t)blockIdx.y * slice, r1 = r0 + slice < p.n ? r0 + slice : p.n;
  for (int i = tid; i < kt * p.E; i += ACC_NT) s_ones[i] = 0;
  for (int i = tid; i < kt; i += ACC_NT) s_cnt[i] = 0;
  const int b = tid & (G - 1), g = tid / G, groups = ACC_NT / G;
  int bad = 0;
  for (int64_t base = r0; base < r1; base += ACC_CHUNK) {
    __syncthreads();                                              // the round before is done with the list (first: the counters are zero)
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
    const int m = s_n;
    for (int j0 = g; j0 < m; j0 += groups * ACC_BATCH) {
      int kl[ACC_BATCH];
      uint32_t by[ACC_BATCH];
#pragma unroll
      for (int q = 0; q < ACC_BATCH; ++q) {
        const int j = j0 + q * groups;
        kl[q] = -1;
        by[q] = 0;
        if (j < m) {
          const int e = s_list[j];
          kl[q] = e & 1023;
          if (b < nbytes) by[q] = p.units[(base + (e >> 10)) * p.row_bytes + b];
        }
      }
#pragma unroll
      for (int q = 0; q < ACC_BATCH; ++q) {
        if (kl[q] < 0) continue;
        if (b == 0) atomicAdd(&s_cnt[kl[q]], 1);
        int* o = s_ones + kl[q] * p.E + 8 * b;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (((by[q] >> c) & 1u) && 8 * b + c < p.E) atomicAdd(o + c, 1);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kt * p.E; i += ACC_NT)
    if (const int v = s_ones[i]) atomicAdd(p.ones + (int64_t)k0 * p.E + i, v);
  for (int i = tid; i < kt; i += ACC_NT)
    if (const int v = s_cnt[i]) atomicAdd(p.cnt + k0 + i, v);
  if (bad) atomicAdd(p.bad, bad);
}

constexpr int UPD_NT = 128;                                       // >= the bytes of the widest row

__global__ void __launch_bounds__(UPD_NT) code_update_kernel(const ZsCodeUpdate p, const int vec) {
  const int k = blockIdx.x;
  const int64_t c = p.cnt[k];
  if (c <= 0) return;                                             // the whole workgroup: an empty cluster keeps its codeword
  const int nbytes = (p.E + 7) >> 3, b = threadIdx.x;
  int diff = 0;
  if (b < nbytes) {
    uint8_t* cw = p.code + (int64_t)k * p.code_bytes + b;
    const uint32_t old = *cw;
    const int ncols = p.E - 8 * b < 8 ? p.E - 8 * b : 8;
    const int32_t* o = p.ones + (int64_t)k * p.E + 8 * b;
    int v[8];
    if (vec && ncols == 8) {
      const int4 lo = *reinterpret_cast<const int4*>(o), hi = *reinterpret_cast<const int4*>(o + 4);
      v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = j < ncols ? o[j] : 0;
    }
    uint32_t nb = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j >= ncols) continue;
      const int64_t twice = 2 * (int64_t)v[j];
      const uint32_t bit = twice > c ? 1u : (twice < c ? 0u : ((old >> j) & 1u));
      nb |= bit << j;
    }
    diff = nb != (old & ((1u << ncols) - 1u));
    if (nb != old) *cw = (uint8_t)nb;
  }
  if (__syncthreads_or(diff) && threadIdx.x == 0) atomicAdd(p.changed, 1);
}

inline int align_mode(const void* base, int64_t pitch, int nbytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(base);
  if ((a & 15) == 0 && pitch % 16 == 0 && nbytes % 16 == 0) return 2;
  if ((a & 3) == 0 && pitch % 4 == 0) return 1;
  return 0;
}

template <int W> void launch_assign(const ZsCodeAssign& p, int umode, int cmode, hipStream_t st) {
  if (p.n >= ZS_CODE_BIG_N)
    hipLaunchKernelGGL((code_assign_kernel<W, 2, 1>), dim3((unsigned)((p.n + 511) / 512)), dim3(256), 0, st, p, umode, cmode);
  else if (p.n >= ZS_CODE_SPLIT_N)
    hipLaunchKernelGGL((code_assign_kernel<W, 1, 1>), dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, st, p, umode, cmode);
  else
    hipLaunchKernelGGL((code_assign_kernel<W, 1, 16>), dim3((unsigned)((p.n + 63) / 64)), dim3(1024), 0, st, p, umode, cmode);
}

const char* check_shape(const char* who, int64_t n, int K, int E, int64_t row_bytes, int64_t code_bytes) {
  (void)who;
  if (K < 1 || K > ZS_CODE_MAX_K) return "K must be in [1, 65536]";
  if (E < 1 || E > ZS_CODE_MAX_E) return "E must be in [1, 1024]";
  if (n < 0 || n >= ((int64_t)1 << 40)) return "n must be in [0, 2^40)";
  if (row_bytes < (E + 7) / 8 || code_bytes < (E + 7) / 8) return "a row pitch is below (E + 7) / 8";
  return nullptr;
}

}  // namespace

extern "C" int zs_code_assign(const ZsCodeAssign* p, void* stream) {
  ZS_REQUIRE(p, "zs_code_assign: null argument");
  const char* why = check_shape("zs_code_assign", p->n, p->K, p->E, p->row_bytes, p->code_bytes);
  ZS_REQUIRE(!why, "zs_code_assign: %s (n %lld, K %d, E %d, row_bytes %d, code_bytes %d)", why, (long long)p->n, p->K, p->E, p->row_bytes,
             p->code_bytes);
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->units && p->code, "zs_code_assign: null operand");
  ZS_REQUIRE(((reinterpret_cast<uintptr_t>(p->idx) | reinterpret_cast<uintptr_t>(p->dist)) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(p->total) & 7) == 0, "zs_code_assign: idx, dist or total is not aligned to its element");
  const int nbytes = (p->E + 7) / 8;
  int umode = align_mode(p->units, p->row_bytes, nbytes);
  if (p->snapped) {
    const int smode = align_mode(p->snapped, p->row_bytes, nbytes);
    umode = smode < umode ? smode : umode;
  }
  const int cmode = align_mode(p->code, p->code_bytes, nbytes);
  const hipStream_t st = (hipStream_t)stream;
  const int words = (p->E + 31) / 32;
  if (words <= 1) launch_assign<1>(*p, umode, cmode, st);
  else if (words <= 2) launch_assign<2>(*p, umode, cmode, st);
  else if (words <= 4) launch_assign<4>(*p, umode, cmode, st);
  else if (words <= 8) launch_assign<8>(*p, umode, cmode, st);
  else if (words <= 16) launch_assign<16>(*p, umode, cmode, st);
  else launch_assign<32>(*p, umode, cmode, st);
  return zs_check_launch("zs_code_assign");
}

extern "C" int zs_code_accum(const ZsCodeAccum* p, void* stream) {
  ZS_REQUIRE(p, "zs_code_accum: null argument");
  const char* why = check_shape("zs_code_accum", p->n, p->K, p->E, p->row_bytes, p->row_bytes);
  ZS_REQUIRE(!why, "zs_code_accum: %s (n %lld, K %d, E %d, row_bytes %d)", why, (long long)p->n, p->K, p->E, p->row_bytes);
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->units && p->idx && p->cnt && p->ones && p->bad, "zs_code_accum: null operand");
  ZS_REQUIRE(((reinterpret_cast<uintptr_t>(p->idx) | reinterpret_cast<uintptr_t>(p->cnt) | reinterpret_cast<uintptr_t>(p->ones) |
               reinterpret_cast<uintptr_t>(p->bad)) & 3) == 0, "zs_code_accum: an int32 operand is not 4-byte aligned");
  const int nbytes = (p->E + 7) / 8;
  int G = 1;
  while (G < nbytes) G *= 2;                                      // lanes per row, <= 128
  int KT = ACC_WORDS / p->E;                                      // codewords whose counters fit a workgroup's LDS: >= 16
  KT = KT > ACC_MAX_KT ? ACC_MAX_KT : KT;
  KT = KT > p->K ? p->K : KT;
  const int ktiles = (p->K + KT - 1) / KT;
  const int64_t chunks = (p->n + ACC_CHUNK - 1) / ACC_CHUNK;
  int64_t ns = 2048 / ktiles;                                     // row slices: about 2048 workgroups where the rows allow
  ns = ns < 1 ? 1 : (ns > chunks ? chunks : ns);
  const int64_t slice = (chunks + ns - 1) / ns * ACC_CHUNK;
  ns = (p->n + slice - 1) / slice;
  ZS_REQUIRE(ns <= 65535, "zs_code_accum: n is too large for K = %d (got %lld)", p->K, (long long)p->n);
  hipLaunchKernelGGL(code_accum_kernel, dim3((unsigned)ktiles, (unsigned)ns), dim3(ACC_NT), 0, (hipStream_t)stream, *p, KT, G, slice);
  return zs_check_launch("zs_code_accum");
}

extern "C" int zs_code_update(const ZsCodeUpdate* p, void* stream) {
  ZS_REQUIRE(p, "zs_code_update: null argument");
  const char* why = check_shape("zs_code_update", 0, p->K, p->E, p->code_bytes, p->code_bytes);
  ZS_REQUIRE(!why, "zs_code_update: %s (K %d, E %d, code_bytes %d)", why, p->K, p->E, p->code_bytes);
  ZS_REQUIRE(p->code && p->cnt && p->ones && p->changed, "zs_code_update: null operand");
  ZS_REQUIRE(((reinterpret_cast<uintptr_t>(p->cnt) | reinterpret_cast<uintptr_t>(p->ones) | reinterpret_cast<uintptr_t>(p->changed)) & 3) == 0,
             "zs_code_update: an int32 operand is not 4-byte aligned");
  const int vec = p->E % 8 == 0 && (reinterpret_cast<uintptr_t>(p->ones) & 15) == 0;
  hipLaunchKernelGGL(code_update_kernel, dim3((unsigned)p->K), dim3(UPD_NT), 0, (hipStream_t)stream, *p, vec);
  return zs_check_launch("zs_code_update");
}

extern "C" int zs_code_scores(const ZsCodeScores* p, void* stream) {
  ZS_REQUIRE(p, "zs_code_scores: null argument");
  const char* why = check_shape("zs_code_scores", p->n, p->K, p->E, p->row_bytes, p->code_bytes);
  ZS_REQUIRE(!why, "zs_code_scores: %s (n %lld, K %d, E %d, row_bytes %d, code_bytes %d)", why, (long long)p->n, p->K, p->E, p->row_bytes,
             p->code_bytes);
  ZS_REQUIRE(p->n <= 0x7fffffff, "zs_code_scores: n must be in [0, 2^31) (got %lld)", (long long)p->n);
  ZS_REQUIRE(p->K <= ZS_SEG_MAX_K, "zs_code_scores: K must be in [1, %d] (got %d)", ZS_SEG_MAX_K, p->K);
  ZS_REQUIRE(p->ld_s >= p->K, "zs_code_scores: ld_s %lld is below K %d", (long long)p->ld_s, p->K);
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->units && p->code && p->scores, "zs_code_scores: null operand");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->scores) & 3) == 0, "zs_code_scores: scores is not aligned to its element");
  const int nbytes = (p->E + 7) / 8;
  const int umode = align_mode(p->units, p->row_bytes, nbytes), cmode = align_mode(p->code, p->code_bytes, nbytes);
  const int vec = (reinterpret_cast<uintptr_t>(p->scores) & 15) == 0 && p->ld_s % 4 == 0;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((p->n + 255) / 256)), block(256);
  const int words = (p->E + 31) / 32;
  if (words <= 1) hipLaunchKernelGGL(code_scores_kernel<1>, grid, block, 0, st, *p, umode, cmode, vec);
  else if (words <= 2) hipLaunchKernelGGL(code_scores_kernel<2>, grid, block, 0, st, *p, umode, cmode, vec);
  else if (words <= 4) hipLaunchKernelGGL(code_scores_kernel<4>, grid, block, 0, st, *p, umode, cmode, vec);
  else if (words <= 8) hipLaunchKernelGGL(code_scores_kernel<8>, grid, block, 0, st, *p, umode, cmode, vec);
  else if (words <= 16) hipLaunchKernelGGL(code_scores_kernel<16>, grid, block, 0, st, *p, umode, cmode, vec);
  else hipLaunchKernelGGL(code_scores_kernel<32>, grid, block, 0, st, *p, umode, cmode, vec);
  return zs_check_launch("zs_code_scores");
}

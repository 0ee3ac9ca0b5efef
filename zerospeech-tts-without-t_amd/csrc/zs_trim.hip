// zs_trim.hip -- librosa.effects.trim on the device (zs_trim, include/zs_amd.h): the (start, stop) bounds convert.trim() gives,
// for a ragged batch of waveforms that stays in HBM (feature extraction: preprocess.py:238 before the STFT).
//
// Two launches:
//   trim_block_sums : one WAVE per (utterance, block of `hop` padded samples): S[u][b] = sum_i y[refl(b*hop + i - frame/2)]^2 in
//                     double.  The frames overlap frame/hop times (4 for 2048 / 512), so summing blocks first reads every sample
//                     once instead of four times; interior blocks are contiguous, 16-byte loads where the address allows.  The grid
//                     is (blocks / 4, utterances): a batch of 64 rows of 10^5 samples is 3 200 workgroups, not 64.
//   trim_finish     : one workgroup per utterance over its few hundred block sums: frame means, their maximum, the first and the
//                     last frame above the threshold, the bounds.
// Every sum has a fixed order that depends on nothing but the row itself (a lane's samples are 4*lane + k + 256*round whichever load
// width is used; the wave reduction is the xor butterfly; a frame adds its blocks in ascending order; maxima and minima are exact),
// so a launch is bitwise reproducible and a row's bounds do not depend on wav_ld, on its neighbours or on the grid.
#include "zs_common.h"

namespace {

constexpr int TRIM_WAVES = 4;                   // waves (blocks of hop samples) per workgroup of trim_block_sums
constexpr int TRIM_FIN = 256;                   // threads of trim_finish

__device__ __forceinline__ int trim_len(const ZsTrim& p, int u) {
  const int64_t n = p.n_samples[u];
  return (int)(n < 0 ? 0 : (n > p.wav_ld ? p.wav_ld : n));
}

__global__ __launch_bounds__(64 * TRIM_WAVES) void trim_block_sums(const ZsTrim p, const int64_t nb_ld) {
  const int u = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * TRIM_WAVES + (threadIdx.x >> 6);
  const int n = trim_len(p, u);
  if (n < 1) return;
  const int64_t nb = (int64_t)n / p.hop + p.frame_length / p.hop;            // frames + frame/hop - 1 blocks
  if (b >= nb) return;                                                        // uniform per wave
  const float* w = p.wav + (int64_t)u * p.wav_ld;
  const int64_t j0 = b * p.hop - p.frame_length / 2;                          // first sample of the block, before reflection
  const bool interior = j0 >= 0 && j0 + p.hop <= n;
  double acc = 0.0;
  for (int base = 4 * lane; base < p.hop; base += 256) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const float* q = w + j0 + base;
    if (interior && base + 4 <= p.hop && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
      const float4 t = *reinterpret_cast<const float4*>(q);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (base + k < p.hop) v[k] = w[interior ? j0 + base + k : zs_reflect_tri(j0 + base + k, n)];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += (double)v[k] * (double)v[k];           // samples past the block's end add an exact zero
  }
  acc = wave_sum_d(acc);
  if (lane == 0) p.work[(int64_t)u * nb_ld + b] = acc;
}

__device__ __forceinline__ double trim_frame_mse(const double* S, int64_t f, int r, double inv) {
  double s = 0.0;
  for (int k = 0; k < r; ++k) s += S[f + k];
  return s * inv;
}

__global__ __launch_bounds__(TRIM_FIN) void trim_finish(const ZsTrim p, const int64_t nb_ld) {
  __shared__ double red[TRIM_FIN];
  __shared__ int64_t lo[TRIM_FIN], hi[TRIM_FIN];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int n = trim_len(p, u);
  if (n < 1) {
    if (tid == 0) { p.bounds[2 * u] = 0; p.bounds[2 * u + 1] = 0; }
    return;
  }
  const double* S = p.work + (int64_t)u * nb_ld;
  const int r = p.frame_length / p.hop;
  const int64_t nf = 1 + (int64_t)n / p.hop;
  const double inv = 1.0 / (double)p.frame_length;                            // a power of two for the defaults: exact either way
  double mx = 0.0;                                                            // mean squares are >= 0
  for (int64_t f = tid; f < nf; f += TRIM_FIN) mx = fmax(mx, trim_frame_mse(S, f, r, inv));
  red[tid] = mx;
  __syncthreads();
  for (int s = TRIM_FIN / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  const double ref = 10.0 * log10(fmax(1e-10, red[0]));
  int64_t first = nf, last = -1;
  for (int64_t f = tid; f < nf; f += TRIM_FIN) {
    const double db = 10.0 * log10(fmax(1e-10, trim_frame_mse(S, f, r, inv))) - ref;
    if (db > -(double)p.top_db) {
      if (f < first) first = f;
      last = f;
    }
  }
  lo[tid] = first; hi[tid] = last;
  __syncthreads();
  for (int s = TRIM_FIN / 2; s > 0; s >>= 1) {
    if (tid < s) {
      if (lo[tid + s] < lo[tid]) lo[tid] = lo[tid + s];
      if (hi[tid + s] > hi[tid]) hi[tid] = hi[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (hi[0] < 0) { p.bounds[2 * u] = 0; p.bounds[2 * u + 1] = 0; }
    else {
      const int64_t stop = (hi[0] + 1) * p.hop;
      p.bounds[2 * u] = (int32_t)(lo[0] * p.hop);
      p.bounds[2 * u + 1] = (int32_t)(stop < n ? stop : n);
    }
  }
}

// block sums per row: the longest row the buffer can hold has 1 + wav_ld / hop frames
int64_t trim_nb_ld(int64_t wav_ld, int frame_length, int hop) { return wav_ld / hop + frame_length / hop; }

bool trim_shape_ok(int32_t n_utt, int64_t wav_ld, int32_t frame_length, int32_t hop) {
  return n_utt >= 0 && n_utt <= 65535 && wav_ld > 0 && wav_ld < (1ll << 31) && hop > 0 && frame_length >= hop &&
         frame_length % hop == 0 && frame_length % 2 == 0;
}

}  // namespace

extern "C" size_t zs_trim_workspace_bytes(int32_t n_utt, int64_t wav_ld, int32_t frame_length, int32_t hop) {
  if (!trim_shape_ok(n_utt, wav_ld, frame_length, hop)) return 0;
  return (size_t)n_utt * (size_t)trim_nb_ld(wav_ld, frame_length, hop) * sizeof(double);
}

extern "C" int zs_trim(const ZsTrim* p, void* stream) {
  ZS_REQUIRE(p, "zs_trim: null argument");
  ZS_REQUIRE(p->n_utt >= 0 && p->n_utt <= 65535, "zs_trim: n_utt must be within [0, 65535] (got %d)", p->n_utt);
  ZS_REQUIRE(p->hop > 0, "zs_trim: hop must be > 0 (got %d)", p->hop);
  ZS_REQUIRE(p->frame_length >= p->hop && p->frame_length % p->hop == 0 && p->frame_length % 2 == 0,
             "zs_trim: frame_length must be even and a positive multiple of hop (got %d / %d)", p->frame_length, p->hop);
  ZS_REQUIRE(p->wav_ld > 0 && p->wav_ld < (1ll << 31), "zs_trim: wav_ld must be within (0, 2^31)");
  ZS_REQUIRE(p->top_db == p->top_db && p->top_db > 0.f, "zs_trim: top_db must be > 0 (got %g)", (double)p->top_db);
  if (p->n_utt == 0) return ZS_OK;
  ZS_REQUIRE(p->wav && p->n_samples && p->bounds && p->work, "zs_trim: null operand");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->work) & 7) == 0, "zs_trim: work must be 8-byte aligned");
  const size_t need = zs_trim_workspace_bytes(p->n_utt, p->wav_ld, p->frame_length, p->hop);
  ZS_REQUIRE(p->work_bytes >= need, "zs_trim: workspace of %zu bytes is smaller than zs_trim_workspace_bytes = %zu", p->work_bytes, need);
  const int64_t nb_ld = trim_nb_ld(p->wav_ld, p->frame_length, p->hop);
  const int64_t gx = (nb_ld + TRIM_WAVES - 1) / TRIM_WAVES;
  ZS_REQUIRE(gx < (1ll << 31), "zs_trim: too many blocks per row");
  hipLaunchKernelGGL(trim_block_sums, dim3((unsigned)gx, (unsigned)p->n_utt), dim3(64 * TRIM_WAVES), 0, (hipStream_t)stream, *p, nb_ld);
  int rc = zs_check_launch("zs_trim.block_sums");
  if (rc) return rc;
  hipLaunchKernelGGL(trim_finish, dim3((unsigned)p->n_utt), dim3(TRIM_FIN), 0, (hipStream_t)stream, *p, nb_ld);
  return zs_check_launch("zs_trim.finish");
}

// zs_resample.hip -- band-limited sample-rate conversion of a ragged batch (zs_resample, include/zs_amd.h): the resampling
// inside librosa.load(sound_file, sr=hp.sr) of preprocess.py:227-258 / convert.py:377,431, and the opposite direction for --out_sr.
//
// Polyphase form.  Output t of a row reads the 2H + 1 input samples around q = floor(t * sr_in / sr_out) and the tap row of its
// phase; the host has laid the bank out by t mod n_phase (zs_amd/resample.py), so the kernel needs q and t mod n_phase only.
//
// Mapping.  One workgroup per (utterance, tile of NT * R consecutive outputs).  Outputs n_phase apart have the same phase, so with
// NT a multiple of n_phase, thread i takes the R outputs t0 + i + r * NT: they share every tap, which is loaded once per R
// multiply-adds, and their inputs lie a fixed NT * sr_in / sr_out samples apart (an integer).  NT is the first multiple of n_phase
// from 256 on and R = 4 (1024 outputs per workgroup at 48 -> 16 kHz, 1280 at 44.1 -> 16 kHz); banks of more than 512 phases, and
// ratios whose tile span would not fit 64 KB of LDS, run NT = 256, R = 1.  The tile's input span (at most
// ceil((NT * R - 1) * sr_in / sr_out) + 2H + 1 samples, zeros outside [0, n_in)) is staged in LDS once; at tap j the 64 lanes of a
// wave read 64 consecutive floats of bank row j through a wave-uniform row pointer (one or two cache lines, L2-resident: the bank is
// at most a few MB and every workgroup walks the same rows) and R LDS words each, q(t) apart between lanes (stride sr_in / sr_out:
// distinct banks for the odd stride of 48 -> 16 kHz, at most two-way conflicts otherwise).  Grouping the LANES by phase instead
// would make the tap a wave-uniform value but spread a wave's inputs over n_phase * sr_in / g samples, far more than LDS holds for
// 44.1 -> 16 kHz (160 phases); it is not built.  Accumulation is one fp32 FMA chain per output in the order j = -H..H, whatever
// R is.  Plain vector loads and stores only, no atomics.
#include "zs_common.h"

namespace {

constexpr int NT_MIN = 256;        // threads per workgroup: the first multiple of n_phase >= NT_MIN, or NT_MIN itself with R = 1
constexpr int R_MAX = 4;           // outputs per thread
constexpr int MAX_PHASE_BLOCK = 512;                   // n_phase above this: R = 1 (NT would pass 1024 threads)
constexpr int64_t MAX_LDS_FLOATS = 16 * 1024;          // 64 KB: what a workgroup gets without an opt-in attribute
constexpr int NZ = 64;             // zero crossings of the filter on either side
constexpr int MAX_RATIO = 32;      // sr_out / sr_in within [1/32, 32]

__host__ __device__ inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// step: NT * sr_in / sr_out, the distance between the inputs of a thread's consecutive outputs (exact; unused with R = 1)
template <int R>
__global__ __launch_bounds__(1024) void resample_kernel(const ZsResample p, const int H, const int span, const int step) {
  extern __shared__ float xs[];                                      // the tile's input span: src[q0 - H .. q0 - H + span)
  const int tid = threadIdx.x, u = blockIdx.y, NT = blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * NT * R, t = t0 + tid;
  float* out = p.dst + (int64_t)u * p.dst_ld;
  int64_t n_in = p.n_in[u];
  n_in = n_in < 0 ? 0 : (n_in > p.src_ld ? p.src_ld : n_in);
  int64_t n_out = ceil_div64(n_in * p.sr_out, p.sr_in);
  if (n_out > p.dst_ld) n_out = p.dst_ld;
  if (t0 >= n_out) {                                                 // a tile behind the row's end: zeros (uniform per workgroup)
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (t + r * NT < p.dst_ld) out[t + r * NT] = 0.f;
    return;
  }
  const float* x = p.src + (int64_t)u * p.src_ld;
  const int64_t lo = t0 * p.sr_in / p.sr_out - H;                    // q of the tile's first output, minus H
  for (int i = tid; i < span; i += NT) {
    const int64_t m = lo + i;
    xs[i] = (m >= 0 && m < n_in) ? x[m] : 0.f;
  }
  __syncthreads();
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  if (t < n_out) {
    // q(t) - H - lo, in [0, span - n_tap - (R - 1) * step]: every read below stays inside the span, whether or not t + r * NT is
    // still inside the row (such an output is computed from staged zeros and samples, and not stored)
    const float* xw = xs + (int)(t * p.sr_in / p.sr_out - lo) - H;
    const int k = (int)(t % p.n_phase);
    const float* row = p.bank;                                       // wave-uniform: bank row j
#pragma unroll 4
    for (int j = 0; j < p.n_tap; ++j, row += p.n_phase) {
      const float w = row[k];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = fmaf(w, xw[r * step + j], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t tr = t + r * NT;
    if (tr < p.dst_ld) out[tr] = tr < n_out ? acc[r] : 0.f;
  }
}

}  // namespace

extern "C" int zs_resample(const ZsResample* p, void* stream) {
  ZS_REQUIRE(p, "zs_resample: null argument");
  ZS_REQUIRE(p->n_utt >= 0 && p->n_utt <= 65535, "zs_resample: n_utt must be within [0, 65535] (got %d)", p->n_utt);
  ZS_REQUIRE(p->sr_in > 0 && p->sr_out > 0, "zs_resample: sample rates must be > 0 (got %d -> %d)", p->sr_in, p->sr_out);
  ZS_REQUIRE((int64_t)p->sr_out <= (int64_t)MAX_RATIO * p->sr_in && (int64_t)p->sr_in <= (int64_t)MAX_RATIO * p->sr_out,
             "zs_resample: sr_out / sr_in must be within [1/32, 32] (got %d -> %d)", p->sr_in, p->sr_out);
  int64_t a = p->sr_in, g = p->sr_out;
  while (a) { const int64_t r = g % a; g = a; a = r; }               // g = gcd(sr_in, sr_out)
  const int H = p->sr_in > p->sr_out ? (int)ceil_div64((int64_t)NZ * p->sr_in, p->sr_out) : NZ;    // ceil(64 / s)
  ZS_REQUIRE(p->n_tap == 2 * H + 1, "zs_resample: n_tap must be 2 ceil(64 / s) + 1 = %d (got %d)", 2 * H + 1, p->n_tap);
  ZS_REQUIRE(p->n_phase == p->sr_out / g, "zs_resample: n_phase must be sr_out / gcd = %d (got %d)", (int)(p->sr_out / g), p->n_phase);
  if (p->n_utt == 0) return ZS_OK;
  ZS_REQUIRE(p->src && p->n_in && p->bank && p->dst, "zs_resample: null operand");
  ZS_REQUIRE(p->src_ld > 0 && p->dst_ld > 0 && p->dst_ld < ((int64_t)1 << 31) && p->src_ld < ((int64_t)1 << 31),
             "zs_resample: src_ld and dst_ld must be within (0, 2^31)");
  ZS_REQUIRE(p->n_in_max >= 0, "zs_resample: n_in_max must be >= 0");
  if (p->n_in_max > 0) {
    ZS_REQUIRE(p->src_ld >= p->n_in_max, "zs_resample: src_ld %lld is smaller than the longest row (%d samples)", (long long)p->src_ld,
               p->n_in_max);
    const int64_t need = ceil_div64((int64_t)p->n_in_max * p->sr_out, p->sr_in);
    ZS_REQUIRE(p->dst_ld >= need, "zs_resample: dst_ld %lld is smaller than the longest row needs (%lld samples)", (long long)p->dst_ld,
               (long long)need);
  }
  // the tile: NT threads x R outputs (see the head of this file)
  int NT = NT_MIN, R = 1;
  if (p->n_phase <= MAX_PHASE_BLOCK) {
    const int nt = p->n_phase * (int)ceil_div64(NT_MIN, p->n_phase);
    if (ceil_div64((int64_t)(nt * R_MAX - 1) * p->sr_in, p->sr_out) + 2 * H + 2 <= MAX_LDS_FLOATS) { NT = nt; R = R_MAX; }
  }
  const int tile = NT * R;
  const int span = (int)ceil_div64((int64_t)(tile - 1) * p->sr_in, p->sr_out) + 2 * H + 2;       // R = 1: <= 255*32 + 4098 floats (49 KB)
  const int step = (int)((int64_t)NT * p->sr_in / p->sr_out);                                   // exact when NT % n_phase == 0
  const unsigned gx = (unsigned)ceil_div64(p->dst_ld, tile);
  const dim3 grid(gx, (unsigned)p->n_utt), block(NT);
  const size_t lds = (size_t)span * sizeof(float);
  if (R == R_MAX) hipLaunchKernelGGL(resample_kernel<R_MAX>, grid, block, lds, (hipStream_t)stream, *p, H, span, step);
  else hipLaunchKernelGGL(resample_kernel<1>, grid, block, lds, (hipStream_t)stream, *p, H, span, step);
  return zs_check_launch("zs_resample");
}

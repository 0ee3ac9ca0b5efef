// zs_voice.hip -- the two kernels of voice adaptation (zs_amd/voice.py; include/zs_amd.h): the five embedding rows of a new speaker
// fitted to a few utterances that lie in device memory, every other weight frozen.
//
// zs_voice_gather: one batch behind a device cursor.  Workgroup row b copies segment item(b) out of the pool into x (the copy of
// zs_pool_gather: 16-byte stores to the aligned destination, 16-byte loads that carry 4-byte alignment only from rows of F = 513
// floats) and expands the segment's seg_len / 8 packed unit rows into the Decoder's input operand (the expansion of
// zs_units_unpack: one lane per byte of a packed row, i.e. per 16-byte (bf16) or 32-byte (fp32) piece of the operand row).  Every
// block reads the cursor and nobody writes it in that launch; a one-thread launch behind it advances it.
//
// zs_voice_adam: ONE workgroup.  Lane i owns element i of the 5 x C gradient: it sums the B per-sample values in ascending b (the
// order of zs_emb_scatter), squares the sum into a double, the workgroup adds the doubles in a fixed order, and after one barrier
// every lane applies zs_adam_clip's update (zs_adam_upd.h) to its own elements.  Nothing is handed from one workgroup to another,
// so there is no counter, no fence and no atomic.
#include "zs_common.h"
#include "zs_adam_upd.h"

namespace {

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int NT = 256;        // threads per block of the gather
constexpr int UNROLL = 4;      // 16-byte loads in flight per thread before the first store
constexpr int NTA = 1024;      // threads of zs_voice_adam's one workgroup

template <typename T> __device__ __forceinline__ void store_bits8(T* p, uint32_t b);
template <> __device__ __forceinline__ void store_bits8<float>(float* p, uint32_t b) {
  *reinterpret_cast<float4*>(p) = make_float4((b & 1u) ? 1.f : 0.f, (b & 2u) ? 1.f : 0.f, (b & 4u) ? 1.f : 0.f, (b & 8u) ? 1.f : 0.f);
  *reinterpret_cast<float4*>(p + 4) = make_float4((b & 16u) ? 1.f : 0.f, (b & 32u) ? 1.f : 0.f, (b & 64u) ? 1.f : 0.f, (b & 128u) ? 1.f : 0.f);
}
template <> __device__ __forceinline__ void store_bits8<bf16_t>(bf16_t* p, uint32_t b) {
  constexpr uint32_t ONE = 0x3f80u;                               // bf16 1.0
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (((b >> (2 * i)) & 1u) ? ONE : 0u) | (((b >> (2 * i + 1)) & 1u) ? (ONE << 16) : 0u);
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}

template <typename T> __global__ void __launch_bounds__(NT) voice_gather_kernel(const ZsVoiceGather p) {
  const uint64_t k = (uint64_t)*p.cursor, n = (uint64_t)p.n;
  const int64_t len = (int64_t)p.seg_len * p.F;
  const int U = p.seg_len >> 3;                                   // unit rows of a segment
  const int groups = (int)(p.ld_bits >> 3);                       // 8-column groups of an operand row
  const int nbytes = (p.E + 7) >> 3;                              // bytes of a packed row that carry columns
  const uint32_t last_mask = (p.E & 7) ? ((1u << (p.E & 7)) - 1u) : 0xffu;
  const int64_t per = (int64_t)U * groups;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  for (int64_t b = blockIdx.y; b < p.B; b += gridDim.y) {
    const uint64_t item = (k * (uint64_t)p.B + (uint64_t)b) % n;
    // ---- the segment's frames ----
    const float* src = p.pool + p.first[item] * (int64_t)p.F;
    float* dst = p.x + b * len;
    const int64_t head = min((int64_t)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3), len);
    const int64_t nvec = (len - head) >> 2;
    const int64_t tail0 = head + (nvec << 2);
    if (tid < head) dst[tid] = src[tid];
    if (tid < len - tail0) dst[tail0 + tid] = src[tail0 + tid];
    const f32x4_a4* sv = reinterpret_cast<const f32x4_a4*>(src + head);
    f32x4* dv = reinterpret_cast<f32x4*>(dst + head);
    int64_t i = tid;
    for (; i + (UNROLL - 1) * nthr < nvec; i += UNROLL * nthr) {
      f32x4_a4 v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = sv[i + u * nthr];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) dv[i + u * nthr] = f32x4{v[u].x, v[u].y, v[u].z, v[u].w};
    }
    for (; i < nvec; i += nthr) {
      const f32x4_a4 v = sv[i];
      dv[i] = f32x4{v.x, v.y, v.z, v.w};
    }
    // ---- the segment's units ----
    const uint8_t* rows = p.packed + p.ufirst[item] * (int64_t)p.row_bytes;
    T* bits = static_cast<T*>(p.bits) + b * (int64_t)U * p.ld_bits;
    for (int64_t j = tid; j < per; j += nthr) {
      const int u = (int)(j / groups), g = (int)(j - (int64_t)u * groups);
      uint32_t v = 0;
      if (g < nbytes) {
        v = rows[(int64_t)u * p.row_bytes + g];
        if (g == nbytes - 1) v &= last_mask;
      }
      store_bits8<T>(bits + (int64_t)u * p.ld_bits + 8 * g, v);
    }
  }
}

__global__ void voice_cursor_kernel(int64_t* cursor) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *cursor += 1;
}

__global__ void __launch_bounds__(NTA) voice_adam_kernel(const ZsVoiceAdam p) {
  __shared__ double red[NTA / 64];
  __shared__ float sq_sh;
  const int tid = threadIdx.x;
  const int n = ZS_VOICE_ROWS * p.C;
  const int64_t slot = (int64_t)p.B * p.C;
  double s = 0.0;
  for (int i = tid; i < n; i += NTA) {
    const int k = i / p.C, c = i - k * p.C;
    const float* e = p.emb_sum + k * slot + c;
    float g = 0.f;
#pragma unroll 8
    for (int b = 0; b < p.B; ++b) g += e[(int64_t)b * p.C];      // ascending b: zs_emb_scatter's sum
    p.g[i] = g;
    s += (double)g * (double)g;
  }
  s = wave_sum_d(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < NTA / 64; ++w) t += red[w];
    const float sq = (float)t;
    *p.sumsq = sq;
    sq_sh = sq;
  }
  __syncthreads();
  ZsAdam a;
  memset(&a, 0, sizeof(a));
  a.lr = p.lr; a.beta1 = p.beta1; a.beta2 = p.beta2; a.eps = p.eps; a.bc1 = p.bc1; a.bc2 = p.bc2;
  a.max_norm = p.max_norm; a.step_ptr = p.step_ptr;
  const AdamCoef cf = adam_coef(a, &sq_sh);
  for (int i = tid; i < n; i += NTA) {
    const int k = i / p.C, c = i - k * p.C;
    float* wp = p.row[k] + c;
    float w = *wp, g = p.g[i], m = p.m[i], v = p.v[i];            // g[i]: this lane's own store above
    adam_upd(cf, w, g, m, v);
    *wp = w; p.m[i] = m; p.v[i] = v;
  }
}

}  // namespace

extern "C" int zs_voice_gather(const ZsVoiceGather* p, void* stream) {
  ZS_REQUIRE(p && p->pool && p->packed && p->first && p->ufirst && p->cursor && p->x && p->bits, "zs_voice_gather: null operand");
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_voice_gather: bad dtype");
  ZS_REQUIRE(p->B > 0 && p->F > 0 && p->E > 0 && p->n > 0, "zs_voice_gather: B, F, E and n must be > 0");
  ZS_REQUIRE(p->seg_len > 0 && p->seg_len % 8 == 0, "zs_voice_gather: seg_len must be a positive multiple of 8 (got %d)", p->seg_len);
  ZS_REQUIRE(p->ld_bits >= p->E && p->ld_bits % 8 == 0, "zs_voice_gather: ld_bits must be >= E and a multiple of 8");
  ZS_REQUIRE(p->row_bytes >= (p->E + 7) / 8, "zs_voice_gather: row_bytes must be >= (E + 7) / 8");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->pool) & 3) == 0 && (reinterpret_cast<uintptr_t>(p->x) & 3) == 0,
             "zs_voice_gather: pool and x must be 4-byte aligned");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->bits) & 15) == 0, "zs_voice_gather: bits must be 16-byte aligned");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->first) & 7) == 0 && (reinterpret_cast<uintptr_t>(p->ufirst) & 7) == 0 &&
             (reinterpret_cast<uintptr_t>(p->cursor) & 7) == 0, "zs_voice_gather: first, ufirst and cursor must be 8-byte aligned");
  const int64_t len = (int64_t)p->seg_len * p->F;
  int64_t bx = (len / 4 + UNROLL * NT - 1) / (UNROLL * NT);     // UNROLL 16-byte copies per thread
  if (bx < 1) bx = 1;
  if (bx > 64) bx = 64;
  const dim3 grid((unsigned)bx, (unsigned)(p->B < 65535 ? p->B : 65535));
  if (p->dtype == ZS_F32)
    hipLaunchKernelGGL(voice_gather_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL(voice_gather_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, *p);
  int rc = zs_check_launch("zs_voice_gather");
  if (rc || !p->advance) return rc;
  hipLaunchKernelGGL(voice_cursor_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p->cursor);
  return zs_check_launch("zs_voice_gather.cursor");
}

extern "C" int zs_voice_adam(const ZsVoiceAdam* p, void* stream) {
  ZS_REQUIRE(p && p->emb_sum && p->m && p->v && p->g && p->sumsq, "zs_voice_adam: null operand");
  for (int k = 0; k < ZS_VOICE_ROWS; ++k) ZS_REQUIRE(p->row[k], "zs_voice_adam: row %d is null", k);
  ZS_REQUIRE(p->B > 0 && p->C > 0 && (int64_t)ZS_VOICE_ROWS * p->C <= ZS_VOICE_ADAM_MAX,
             "zs_voice_adam: need B > 0 and 0 < 5 C <= %d (got B %d, C %d)", ZS_VOICE_ADAM_MAX, p->B, p->C);
  ZS_REQUIRE(p->step_ptr || (p->bc1 > 0.f && p->bc2 > 0.f), "zs_voice_adam: bias corrections");
  hipLaunchKernelGGL(voice_adam_kernel, dim3(1), dim3(NTA), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_voice_adam");
}

// zs_tclf.hip -- the batched --test_classify path (convert.py:364-414): the classifier's fragments gathered out of a batch of
// spectrograms in one launch, and the per-fragment argmax / accuracy count on the device.
#include "zs_common.h"

namespace {

constexpr int NBIN = 513;

// Four dwords with 4-byte alignment: the fragment's source starts at utt * utt_stride + start * 513 floats, so only a quarter of the
// fragments share the 16-byte phase of their destination.  gfx950 global loads of 16 bytes need dword alignment only (the
// compiler emits global_load_dwordx4 for this type); the stores stay 16-byte aligned.
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// Fragments f = blockIdx.y (+ gridDim.y ...); the gridDim.x blocks of a fragment stride its seg_len * 513 floats in 16-byte steps of the
// destination: a scalar head up to the first 16-byte-aligned destination float, dwordx4 copies, a scalar tail.
__global__ void __launch_bounds__(256) frag_gather_kernel(const ZsFragGather p) {
  const int64_t n = (int64_t)p.seg_len * NBIN;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  for (int64_t f = blockIdx.y; f < p.n_frag; f += gridDim.y) {
    float* dst = p.dst + f * n;
    const int utt = p.table[2 * f], start = p.table[2 * f + 1];
    const bool ok = utt >= 0 && utt < p.n_utt && start >= 0 && start <= p.T_max - p.seg_len;     // else: a zero fragment
    const float* src = ok ? p.src + (int64_t)utt * p.utt_stride + (int64_t)start * NBIN : nullptr;
    const int64_t head = min((int64_t)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3), n);
    const int64_t nvec = (n - head) >> 2;
    const int64_t tail0 = head + (nvec << 2);
    if (tid < head) dst[tid] = ok ? src[tid] : 0.f;
    if (tid < n - tail0) dst[tail0 + tid] = ok ? src[tail0 + tid] : 0.f;
    f32x4* dv = reinterpret_cast<f32x4*>(dst + head);
    if (!ok) {
      for (int64_t i = tid; i < nvec; i += nthr) dv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const f32x4_a4* sv = reinterpret_cast<const f32x4_a4*>(src + head);
    for (int64_t i = tid; i < nvec; i += nthr) {
      const f32x4_a4 v = sv[i];
      dv[i] = f32x4{v.x, v.y, v.z, v.w};
    }
  }
}

// numpy's argmax over the three columns: the first maximum, a NaN counts as the maximum (the first NaN wins).
__device__ __forceinline__ int argmax3(const float* l) {
  int am = 0;
  float mx = l[0];
  for (int j = 1; j < 3; ++j) {
    if (mx != mx) break;
    if (l[j] > mx || l[j] != l[j]) { mx = l[j]; am = j; }
  }
  return am;
}

__global__ void __launch_bounds__(256) tclf_score_kernel(const ZsTclfScore p) {
  __shared__ int red[4];
  int corr = 0, cnt = 0;
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < p.n_frag; f += (int64_t)gridDim.x * blockDim.x) {
    const int am = argmax3(p.logits + f * p.ld);
    if (p.pred) p.pred[f] = am;
    corr += (am == p.target[f]);
    cnt += 1;
  }
  for (int o = 32; o > 0; o >>= 1) {
    corr += __shfl_xor(corr, o);
    cnt += __shfl_xor(cnt, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = corr;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = red[0] + red[1] + red[2] + red[3];
    if (c) atomicAdd(p.correct, c);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = red[0] + red[1] + red[2] + red[3];
    if (c) atomicAdd(p.count, c);
  }
}

}  // namespace

extern "C" int zs_frag_gather(const ZsFragGather* p, void* stream) {
  ZS_REQUIRE(p && p->src && p->table && p->dst, "zs_frag_gather: null operand");
  ZS_REQUIRE(p->n_frag > 0, "zs_frag_gather: n_frag must be > 0");
  ZS_REQUIRE(p->seg_len > 0 && p->n_utt > 0 && p->T_max >= p->seg_len, "zs_frag_gather: need n_utt > 0 and 0 < seg_len <= T_max");
  ZS_REQUIRE(p->utt_stride >= (int64_t)p->T_max * NBIN, "zs_frag_gather: utt_stride must be >= T_max * 513");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->src) & 3) == 0 && (reinterpret_cast<uintptr_t>(p->dst) & 3) == 0,
             "zs_frag_gather: src and dst must be 4-byte aligned");
  const int64_t n = (int64_t)p->seg_len * NBIN;
  int64_t bx = (n / 4 + 4 * 256 - 1) / (4 * 256);           // about four 16-byte copies per thread
  if (bx < 1) bx = 1;
  if (bx > 64) bx = 64;
  const unsigned by = (unsigned)(p->n_frag < 65535 ? p->n_frag : 65535);
  hipLaunchKernelGGL(frag_gather_kernel, dim3((unsigned)bx, by), dim3(256), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_frag_gather");
}

extern "C" int zs_tclf_score(const ZsTclfScore* p, void* stream) {
  ZS_REQUIRE(p && p->logits && p->target && p->correct && p->count, "zs_tclf_score: null operand");
  ZS_REQUIRE(p->n_frag > 0, "zs_tclf_score: n_frag must be > 0");
  ZS_REQUIRE(p->ld >= 3, "zs_tclf_score: ld must be >= 3 (three classes)");
  int64_t nb = (p->n_frag + 255) / 256;
  if (nb > 256) nb = 256;
  hipLaunchKernelGGL(tclf_score_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_tclf_score");
}

// zs_autolocker.hip -- the two kernels of the stage-2 autolocker step (reference trainer.py:563-611) that the other passes do not
// have: the BCE re-encoding loss on the hard units fused with the MBV straight-through backward, and the fold of the encoder's
// input-gradient (conv bank data gradient over the 3/3-padded domain + the pass-through columns of the concatenation) into dx.
#include "zs_common.h"

namespace {

constexpr int NTA = 256;
constexpr int BCE_MAX_BLOCKS = 1024;      // = the partial buffer the caller provides (doubles)

inline unsigned blocks_for(int64_t total, int cap) {
  int64_t b = (total + NTA - 1) / NTA;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// torch.nn.BCELoss (mean) on x = re_enc, y = enc_act: l = -(y * max(log x, -100) + (1 - y) * max(log(1 - x), -100)),
// dl/dx = (x - y) / max(x (1 - x), 1e-12) / N (ATen binary_cross_entropy_backward), then the MBV backward of zs_mbv_bwd:
// dlogit_0 = dx * y0 (1 - y0) / tau, dlogit_1 = -dlogit_0.  One thread per (row, unit pair) of dlogits; a fixed grid, per-block
// double partials in a fixed order, summed by one thread in stage 2 -- the loss is deterministic.
template <typename T>
__global__ __launch_bounds__(NTA) void bce_mbv_stage1(const ZsBceMbvBwd p, double n_inv) {
  __shared__ double red[NTA / 64];
  const int half = p.fill_cols / 2;
  const int64_t total = p.rows * half;
  const float gs = p.grad_scale != 0.f ? p.grad_scale : 1.f;
  const float ninv = (float)n_inv;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / half;
    const int e = (int)(i - r * half);
    float d0 = 0.f;
    if (e < p.E) {
      const int64_t k = r * p.E + e;
      const float x = p.bits[k], y = p.target[k], y0 = p.y0[k];
      const float lx = fmaxf(logf(x), -100.f), l1x = fmaxf(logf(1.f - x), -100.f);
      s += (double)(-(y * lx + (1.f - y) * l1x));
      const float dx = __fmul_rn(__fdiv_rn(__fsub_rn(x, y), fmaxf(__fmul_rn(__fsub_rn(1.f, x), x), 1e-12f)), gs * ninv);
      d0 = dx * y0 * (1.f - y0) / p.tau;
    }
    Elem<T>::st((T*)p.dlogits + r * p.ld + 2 * e, d0);
    Elem<T>::st((T*)p.dlogits + r * p.ld + 2 * e + 1, -d0);
  }
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void bce_mbv_stage2(const double* partial, int nb, double n_inv, float* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < nb; ++i) t += partial[i];
    *out = (float)(t * n_inv);
  }
}

// dx[b, t, c] = g[b, t + pad, c] (+ the padding rows that read x[t]: reflect) + pass_through[b, t, c].  One thread per output element.
template <typename T>
__global__ __launch_bounds__(NTA) void enc_dx_fold_kernel(const ZsEncDxFold p) {
  const int64_t total = (int64_t)p.B * p.T * p.C;
  const int Tp = p.T + 2 * p.pad;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % p.C);
    const int64_t bt = i / p.C;
    const int t = (int)(bt % p.T), b = (int)(bt / p.T);
    const float* g = p.g + (int64_t)b * Tp * p.ldg + c;
    float v = g[(int64_t)(t + p.pad) * p.ldg];
    if (p.pad_mode == ZS_PAD_REFLECT) {
      if (t >= 1 && t <= p.pad) v += g[(int64_t)(p.pad - t) * p.ldg];                   // left rows u < pad read x[pad - u]
      const int q = 2 * p.T - 2 - t;                                                      // right rows read x[2(T-1) - (u - pad)]
      if (q >= p.T && q < p.T + p.pad) v += g[(int64_t)(q + p.pad) * p.ldg];
    }
    if (p.pass_through) v += Elem<T>::ld((const T*)p.pass_through + bt * p.ld_pass + c);
    p.dx[bt * p.ldx + c] = v;
  }
}

}  // namespace

extern "C" int zs_bce_mbv_bwd(const ZsBceMbvBwd* p, void* stream) {
  ZS_REQUIRE(p && p->bits && p->y0 && p->target && p->dlogits && p->partial && p->loss_out, "zs_bce_mbv_bwd: null operand");
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_bce_mbv_bwd: bad dtype");
  ZS_REQUIRE(p->rows > 0 && p->E > 0 && p->tau > 0.f && p->fill_cols >= 2 * p->E && p->fill_cols % 2 == 0 && p->ld >= p->fill_cols,
             "zs_bce_mbv_bwd: sizes (rows %lld E %d fill_cols %d ld %lld)", (long long)p->rows, p->E, p->fill_cols, (long long)p->ld);
  const unsigned nb = blocks_for(p->rows * (p->fill_cols / 2), BCE_MAX_BLOCKS);
  const double n_inv = 1.0 / ((double)p->rows * (double)p->E);
  if (p->dtype == ZS_F32) hipLaunchKernelGGL(bce_mbv_stage1<float>, dim3(nb), dim3(NTA), 0, (hipStream_t)stream, *p, n_inv);
  else hipLaunchKernelGGL(bce_mbv_stage1<bf16_t>, dim3(nb), dim3(NTA), 0, (hipStream_t)stream, *p, n_inv);
  int rc = zs_check_launch("zs_bce_mbv_bwd.stage1");
  if (rc) return rc;
  hipLaunchKernelGGL(bce_mbv_stage2, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)p->partial, (int)nb, n_inv, p->loss_out);
  return zs_check_launch("zs_bce_mbv_bwd.stage2");
}

extern "C" int zs_enc_dx_fold(const ZsEncDxFold* p, void* stream) {
  ZS_REQUIRE(p && p->g && p->dx, "zs_enc_dx_fold: null operand");
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_enc_dx_fold: bad dtype");
  ZS_REQUIRE(p->B > 0 && p->T > 0 && p->C > 0 && p->pad >= 0 && p->ldg >= p->C && p->ldx >= p->C && (!p->pass_through || p->ld_pass >= p->C),
             "zs_enc_dx_fold: sizes (B %d T %d C %d pad %d)", p->B, p->T, p->C, p->pad);
  ZS_REQUIRE(p->pad_mode == ZS_PAD_ZERO || (p->pad_mode == ZS_PAD_REFLECT && p->T > p->pad), "zs_enc_dx_fold: reflect pad %d needs T > %d (T = %d)",
             p->pad, p->pad, p->T);
  const unsigned nb = blocks_for((int64_t)p->B * p->T * p->C, 4096);
  if (p->dtype == ZS_F32) hipLaunchKernelGGL(enc_dx_fold_kernel<float>, dim3(nb), dim3(NTA), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL(enc_dx_fold_kernel<bf16_t>, dim3(nb), dim3(NTA), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_enc_dx_fold");
}

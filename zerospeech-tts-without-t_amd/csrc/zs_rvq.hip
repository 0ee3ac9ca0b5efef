// zs_rvq.hip -- the glue of a residual vector codebook (include/zs_amd.h): what a stage leaves over for the next one
// (zs_rvq_residual) and the Decoder's input operand from S planes of indices: of an inference chunk, one stage count for the launch
// (zs_rvq_gather), and of a training step under quantiser dropout, a stage count per fragment (zs_rvq_gather_frag,
// include/zs_amd_rvq_drop.h).  All are memory-bound and row-parallel; the nearest-codeword search of every stage is
// zs_vq_assign (zs_vq.hip), unchanged.
//   rvq_residual_kernel   vq_commit_kernel's layout: a row is owned by a team of 2^t <= 64 lanes of one wave, one 16-byte piece of r per
//                         lane and round.  A lane reads the piece of x it writes in r, so r may be x itself.
//   rvq_gather_kernel     vq_gather_kernel's layout: one lane per 16-byte piece of the operand.  A lane reads the s_use indices of its
//                         row first: one of them outside [0, K) and no codeword is read.  One text for both entry points: where the
//                         count comes from is a template parameter, so zs_rvq_gather_frag with every count at s is zs_rvq_gather at s
//                         by construction.
// The row accesses are zs_quant.h's.
#include "zs_quant.h"
#include "../../include/zs_amd_rvq_drop.h"

// the definitions are one fp32 subtraction, and fp32 adds in increasing stage: nothing in this file may be fused or reassociated
#pragma clang fp contract(off)

namespace {

constexpr int RQ_NT = 256;

// ---- residual ----------------------------------------------------------------------------------------------------------------------
template <typename S> __global__ void __launch_bounds__(RQ_NT)
rvq_residual_kernel(const ZsRvqResidual p, const int tl, const int groups, const int xvec, const int cvec, const int rvec) {
  const int tid = threadIdx.x, tlane = tid & (tl - 1);
  const int64_t n_teams = (int64_t)gridDim.x * (RQ_NT / tl);
  const S* x = static_cast<const S*>(p.x);
  int bad = 0;
  for (int64_t row = (int64_t)blockIdx.x * (RQ_NT / tl) + tid / tl; row < p.n; row += n_teams) {
    const int k = p.idx[row];
    const bool ok = k >= 0 && k < p.K;                            // else never an index: the row is copied
    bad += !ok && tlane == 0;
    const S* xr = x + row * p.ld_x;
    const float* cr = p.code + (int64_t)(ok ? k : 0) * p.ld_code;
    float* rr = p.r + row * p.ld_r;
    for (int g = tlane; g < groups; g += tl) {
      const int c = 4 * g;
      float xv[4], cv[4] = {0.f, 0.f, 0.f, 0.f};
      q_load4<S>(xr, c, p.E, xvec != 0, xv);
      if (ok) {
        q_load4<float>(cr, c, p.E, cvec != 0, cv);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = xv[j] - cv[j];        // one IEEE subtraction
      }
      if (rvec && c + 4 <= p.E) {                                 // (not q_store4: the kernel's instruction stream is kept as it was)
        *reinterpret_cast<float4*>(rr + c) = make_float4(xv[0], xv[1], xv[2], xv[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c + j < p.E) rr[c + j] = xv[j];
      }
    }
  }
  if (bad) atomicAdd(p.bad, bad);
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------
// FRAG (zs_rvq_gather_frag): p.s_use is a count per fragment, read once per fragment and the same for every lane of the workgroup;
// else one count for the whole launch, checked on the host.
template <typename T, bool FRAG, typename P> __global__ void __launch_bounds__(RQ_NT) rvq_gather_kernel(const P p, const int cvec) {
  constexpr int PER = 16 / (int)sizeof(T);                        // columns of a 16-byte piece
  const int groups = (int)(p.ld_dst / PER);
  const int64_t per_frag = (int64_t)p.T * groups;
  const int64_t tid = (int64_t)blockIdx.x * RQ_NT + threadIdx.x, nthr = (int64_t)gridDim.x * RQ_NT;
  int bad = 0;
  for (int64_t f = blockIdx.y; f < p.n_frag; f += gridDim.y) {
    const int64_t start = p.start[f];
    const int len = p.len[f];
    int su;
    if constexpr (FRAG) su = p.s_use[f];
    else su = p.s_use;
    const bool ok = len >= 0 && len <= p.T && start >= 0 && start <= p.n_idx - len;          // else: a zero fragment, nothing read
    const bool counted = !FRAG || (su >= 1 && su <= p.S);           // else: zero rows, a bad frame each, no index read
    T* dst = static_cast<T*>(p.dst) + f * p.T * p.ld_dst;
    for (int64_t i = tid; i < per_frag; i += nthr) {
      const int t = (int)(i / groups), g = (int)(i - (int64_t)t * groups);
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (ok && t < len) {
        int k[ZS_RVQ_MAX_S];
        bool in = counted;
#pragma unroll
        for (int s = 0; s < ZS_RVQ_MAX_S; ++s) {
          k[s] = (counted && s < su) ? p.idx[(int64_t)s * p.ld_idx + start + t] : 0;
          in = in && k[s] >= 0 && k[s] < p.K;
        }
        if (!in) {
          bad += g == 0;                                          // once per row, however many of its indices are out of range
        } else if (PER * g < p.E) {
          q_load_code<PER>(p.code + (int64_t)k[0] * p.ld_code, PER * g, p.E, cvec != 0, v);
#pragma unroll
          for (int s = 1; s < ZS_RVQ_MAX_S; ++s)
            if (s < su) {
              float w[8];
              q_load_code<PER>(p.code + (int64_t)s * p.plane_code + (int64_t)k[s] * p.ld_code, PER * g, p.E, cvec != 0, w);
#pragma unroll
              for (int j = 0; j < PER; ++j) v[j] = v[j] + w[j];   // in increasing stage, a rounding each
            }
        }
      }
      q_store_piece<T>(dst + (int64_t)t * p.ld_dst + PER * g, v);
    }
  }
  if (bad) atomicAdd(p.bad, bad);
}

const char* rvq_shape(int K, int E, int64_t n, int64_t ld_a, int64_t ld_b) {
  if (K < 1 || K > ZS_CODE_MAX_K) return "K must be in [1, 65536]";
  if (E < 1 || E > ZS_CODE_MAX_E) return "E must be in [1, 1024]";
  if (n < 0 || n > 0x7fffffff) return "n must be in [0, 2^31)";
  if (ld_a < E || ld_b < E) return "a leading dimension is below E";
  return nullptr;
}

// zs_rvq_gather (P = ZsRvqGather) and zs_rvq_gather_frag (FRAG, P = ZsRvqGatherFrag): the checks, the grid and the launch
template <bool FRAG, typename P> int gather_launch(const P* p, void* stream, const char* name) {
  ZS_REQUIRE(p, "%s: null argument", name);
  ZS_REQUIRE(p->n_frag >= 0 && p->n_frag <= ZS_UNITS_MAX_FRAG, "%s: n_frag must be in [0, %d] (got %d)", name, ZS_UNITS_MAX_FRAG, p->n_frag);
  const char* why = rvq_shape(p->K, p->E, p->n_idx, p->ld_dst, p->ld_code);
  ZS_REQUIRE(!why, "%s: %s (n_idx %lld, K %d, E %d, ld_dst %lld, ld_code %lld)", name, why, (long long)p->n_idx, p->K, p->E,
             (long long)p->ld_dst, (long long)p->ld_code);
  const void* s_use = nullptr;                                    // FRAG: an operand like the others
  if constexpr (FRAG) {
    ZS_REQUIRE(p->S >= 1 && p->S <= ZS_RVQ_MAX_S, "%s: S must be in [1, %d] (got %d)", name, ZS_RVQ_MAX_S, p->S);
    s_use = p->s_use;
  } else {
    ZS_REQUIRE(p->S >= 1 && p->S <= ZS_RVQ_MAX_S && p->s_use >= 1 && p->s_use <= p->S,
               "%s: S must be in [1, %d] and s_use in [1, S] (got S %d, s_use %d)", name, ZS_RVQ_MAX_S, p->S, p->s_use);
  }
  ZS_REQUIRE(p->ld_idx >= p->n_idx, "%s: the index planes are ld_idx = %lld apart and hold n_idx = %lld entries", name,
             (long long)p->ld_idx, (long long)p->n_idx);
  ZS_REQUIRE(p->plane_code >= (int64_t)(p->K - 1) * p->ld_code + p->E,
             "%s: the codebooks are plane_code = %lld apart, K = %d rows of ld_code = %lld need %lld", name, (long long)p->plane_code, p->K,
             (long long)p->ld_code, (long long)((int64_t)(p->K - 1) * p->ld_code + p->E));
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "%s: bad dtype", name);
  ZS_REQUIRE(p->T > 0 && p->ld_dst % 8 == 0, "%s: T must be > 0 and ld_dst a multiple of 8", name);
  if (p->n_frag == 0) return ZS_OK;
  ZS_REQUIRE(p->dst && p->start && p->len && p->code && p->bad && (!FRAG || s_use) && (p->idx || p->n_idx == 0), "%s: null operand", name);
  ZS_REQUIRE(!misaligned(p->dst, 16) && !misaligned(p->code, 4) && !misaligned(p->idx, 4) && !misaligned(p->bad, 4) &&
                 !misaligned(p->start, 8) && !misaligned(p->len, 4) && !misaligned(s_use, 4),
             "%s: an operand is misaligned (dst: 16 bytes)", name);
  const int cvec = !misaligned(p->code, 16) && p->ld_code % 4 == 0 && p->plane_code % 4 == 0;
  const int per = p->dtype == ZS_F32 ? 4 : 8;
  int64_t bx = ((int64_t)p->T * (p->ld_dst / per) + RQ_NT - 1) / RQ_NT;
  bx = bx > 64 ? 64 : bx;
  const dim3 grid((unsigned)bx, (unsigned)(p->n_frag < 65535 ? p->n_frag : 65535));
  if (p->dtype == ZS_F32)
    hipLaunchKernelGGL((rvq_gather_kernel<float, FRAG, P>), grid, dim3(RQ_NT), 0, (hipStream_t)stream, *p, cvec);
  else
    hipLaunchKernelGGL((rvq_gather_kernel<bf16_t, FRAG, P>), grid, dim3(RQ_NT), 0, (hipStream_t)stream, *p, cvec);
  return zs_check_launch(name);
}

}  // namespace

extern "C" int zs_rvq_residual(const ZsRvqResidual* p, void* stream) {
  ZS_REQUIRE(p, "zs_rvq_residual: null argument");
  const char* why = rvq_shape(p->K, p->E, p->n, p->ld_x, p->ld_code);
  ZS_REQUIRE(!why && p->ld_r >= p->E, "zs_rvq_residual: %s (n %lld, K %d, E %d, ld_x %lld, ld_code %lld, ld_r %lld)",
             why ? why : "a leading dimension is below E", (long long)p->n, p->K, p->E, (long long)p->ld_x, (long long)p->ld_code,
             (long long)p->ld_r);
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_rvq_residual: bad dtype");
  if (p->n == 0) return ZS_OK;
  ZS_REQUIRE(p->x && p->idx && p->code && p->r && p->bad, "zs_rvq_residual: null operand");
  const bool f32 = p->src_f32 || p->dtype == ZS_F32;
  ZS_REQUIRE(!misaligned(p->x, f32 ? 4 : 2) && !misaligned(p->idx, 4) && !misaligned(p->code, 4) && !misaligned(p->r, 4) &&
                 !misaligned(p->bad, 4), "zs_rvq_residual: an operand is not aligned to its element");
  ZS_REQUIRE(static_cast<const void*>(p->r) != p->x || (f32 && p->ld_r == p->ld_x),
             "zs_rvq_residual: in place (r == x) needs fp32 x and ld_r == ld_x (ld_x %lld, ld_r %lld)", (long long)p->ld_x, (long long)p->ld_r);
  const int xvec = !misaligned(p->x, f32 ? 16 : 8) && p->ld_x % 4 == 0;
  const int cvec = !misaligned(p->code, 16) && p->ld_code % 4 == 0;
  const int rvec = !misaligned(p->r, 16) && p->ld_r % 4 == 0;
  const int groups = (p->E + 3) / 4, tl = team_lanes(groups);
  const dim3 grid(team_wgs(p->n, tl, RQ_NT, 4096));
  if (f32)
    hipLaunchKernelGGL(rvq_residual_kernel<float>, grid, dim3(RQ_NT), 0, (hipStream_t)stream, *p, tl, groups, xvec, cvec, rvec);
  else
    hipLaunchKernelGGL(rvq_residual_kernel<bf16_t>, grid, dim3(RQ_NT), 0, (hipStream_t)stream, *p, tl, groups, xvec, cvec, rvec);
  return zs_check_launch("zs_rvq_residual");
}

extern "C" int zs_rvq_gather(const ZsRvqGather* p, void* stream) {
  return gather_launch<false>(p, stream, "zs_rvq_gather");
}

extern "C" int zs_rvq_gather_frag(const ZsRvqGatherFrag* p, void* stream) {
  return gather_launch<true>(p, stream, "zs_rvq_gather_frag");
}

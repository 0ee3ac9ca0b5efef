// zs_units.hip -- bit-packed discrete units at the device boundary: the encoder's 0/1 rows packed eight columns to the byte for the
// one copy to the host (zs_units_pack), and packed units written straight into the Decoder's input operand of an inference chunk
// (zs_units_unpack).  Bit j of byte k of a row is column 8k + j (numpy's packbits(bitorder='little')).
// One lane owns one byte of the packed side, i.e. eight consecutive columns of the wide side: every output byte and every 16-byte
// store is produced whole by one lane, so there is no read-modify-write, no atomic, and a launch is bitwise reproducible.
#include "zs_common.h"

namespace {

constexpr int NT = 256;

// ---- unpack ----------------------------------------------------------------------------------------------------------------------
// Fragment f = blockIdx.y (+ gridDim.y ...); its T * (ld_dst / 8) column groups are strided by the gridDim.x blocks.  Consecutive
// lanes take consecutive groups of a row: consecutive bytes of the packed row in, consecutive 16-byte (bf16) or 32-byte (fp32)
// pieces of the operand row out.
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

template <typename T> __global__ void __launch_bounds__(NT) units_unpack_kernel(const ZsUnitsUnpack p) {
  const int groups = (int)(p.ld_dst >> 3);                        // 8-column groups of an operand row
  const int nbytes = (p.E + 7) >> 3;                              // bytes of a packed row that carry columns
  const uint32_t last_mask = (p.E & 7) ? ((1u << (p.E & 7)) - 1u) : 0xffu;
  const int64_t per_frag = (int64_t)p.T * groups;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  for (int64_t f = blockIdx.y; f < p.n_frag; f += gridDim.y) {
    const int64_t start = p.start[f];
    const int len = p.len[f];
    const bool ok = len >= 0 && len <= p.T && start >= 0 && start <= p.n_units - len;        // else: a zero fragment, nothing read
    T* dst = static_cast<T*>(p.dst) + f * p.T * p.ld_dst;
    for (int64_t i = tid; i < per_frag; i += nthr) {
      const int t = (int)(i / groups), g = (int)(i - (int64_t)t * groups);
      uint32_t b = 0;
      if (ok && t < len && g < nbytes) {
        b = p.packed[(start + t) * p.row_bytes + g];
        if (g == nbytes - 1) b &= last_mask;
      }
      store_bits8<T>(dst + (int64_t)t * p.ld_dst + 8 * g, b);
    }
  }
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------
// One lane per byte of a packed row: the eight source columns 8k .. 8k + 7 (those below E) of row t of fragment f, read in place.
template <typename S> __device__ __forceinline__ uint32_t bits_of8(const S* p, int n, bool vec) {
  uint32_t b = 0;
  if (vec && n == 8) {
    float v[8];
    load8<S>(p, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) b |= (v[j] != 0.f) ? (1u << j) : 0u;
  } else {
    for (int j = 0; j < n; ++j) b |= (Elem<S>::ld(p + j) != 0.f) ? (1u << j) : 0u;
  }
  return b;
}

template <typename S> __global__ void __launch_bounds__(NT) units_pack_kernel(const ZsUnitsPack p, const int vec) {
  const int nbytes = (p.E + 7) >> 3;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  for (int64_t f = blockIdx.y; f < p.n_frag; f += gridDim.y) {
    const int64_t start = p.start[f];
    const int len = p.len[f];
    if (!(len >= 0 && len <= p.T && start >= 0 && start <= p.n_units - len)) continue;       // nothing read, nothing written
    const S* src = static_cast<const S*>(p.src) + f * p.T * p.ld_src;
    const int64_t n = (int64_t)len * p.row_bytes;                 // rows t >= len are not read
    for (int64_t i = tid; i < n; i += nthr) {
      const int t = (int)(i / p.row_bytes), k = (int)(i - (int64_t)t * p.row_bytes);
      uint32_t b = 0;
      if (k < nbytes) {
        const int cols = p.E - 8 * k < 8 ? p.E - 8 * k : 8;
        b = bits_of8<S>(src + (int64_t)t * p.ld_src + 8 * k, cols, vec != 0);
      }
      p.packed[(start + t) * p.row_bytes + k] = (uint8_t)b;
    }
  }
}

inline unsigned blocks_x(int64_t work) {                          // a fragment's work items over at most 64 blocks of 256 lanes
  int64_t bx = (work + NT - 1) / NT;
  return (unsigned)(bx < 1 ? 1 : (bx > 64 ? 64 : bx));
}

}  // namespace

extern "C" int zs_units_unpack(const ZsUnitsUnpack* p, void* stream) {
  ZS_REQUIRE(p, "zs_units_unpack: null argument");
  ZS_REQUIRE(p->n_frag >= 0 && p->n_frag <= ZS_UNITS_MAX_FRAG, "zs_units_unpack: n_frag must be in [0, %d] (got %d)", ZS_UNITS_MAX_FRAG,
             p->n_frag);
  if (p->n_frag == 0) return ZS_OK;
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_units_unpack: bad dtype");
  ZS_REQUIRE(p->E > 0 && p->T > 0, "zs_units_unpack: E and T must be > 0");
  ZS_REQUIRE(p->ld_dst >= p->E && p->ld_dst % 8 == 0, "zs_units_unpack: ld_dst must be >= E and a multiple of 8");
  ZS_REQUIRE(p->row_bytes >= (p->E + 7) / 8, "zs_units_unpack: row_bytes must be >= (E + 7) / 8");
  ZS_REQUIRE(p->n_units >= 0, "zs_units_unpack: n_units must be >= 0");
  ZS_REQUIRE(p->dst && p->start && p->len && (p->packed || p->n_units == 0), "zs_units_unpack: null operand");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->dst) & 15) == 0, "zs_units_unpack: dst must be 16-byte aligned");
  const dim3 grid(blocks_x((int64_t)p->T * (p->ld_dst / 8)), (unsigned)(p->n_frag < 65535 ? p->n_frag : 65535));
  if (p->dtype == ZS_F32)
    hipLaunchKernelGGL(units_unpack_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL(units_unpack_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, *p);
  return zs_check_launch("zs_units_unpack");
}

extern "C" int zs_units_pack(const ZsUnitsPack* p, void* stream) {
  ZS_REQUIRE(p, "zs_units_pack: null argument");
  ZS_REQUIRE(p->n_frag >= 0 && p->n_frag <= ZS_UNITS_MAX_FRAG, "zs_units_pack: n_frag must be in [0, %d] (got %d)", ZS_UNITS_MAX_FRAG,
             p->n_frag);
  if (p->n_frag == 0) return ZS_OK;
  ZS_REQUIRE(p->dtype == ZS_F32 || p->dtype == ZS_BF16, "zs_units_pack: bad dtype");
  ZS_REQUIRE(p->E > 0 && p->T > 0, "zs_units_pack: E and T must be > 0");
  ZS_REQUIRE(p->ld_src >= p->E, "zs_units_pack: ld_src must be >= E");
  ZS_REQUIRE(p->row_bytes >= (p->E + 7) / 8, "zs_units_pack: row_bytes must be >= (E + 7) / 8");
  ZS_REQUIRE(p->n_units >= 0, "zs_units_pack: n_units must be >= 0");
  ZS_REQUIRE(p->src && p->start && p->len && (p->packed || p->n_units == 0), "zs_units_pack: null operand");
  const bool f32 = p->src_f32 || p->dtype == ZS_F32;
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->src) & (f32 ? 3 : 1)) == 0, "zs_units_pack: src is not aligned to its element");
  // 16-byte reads where every 8-column group of every row is 16-byte aligned; otherwise element by element
  const int vec = (reinterpret_cast<uintptr_t>(p->src) & 15) == 0 && p->ld_src % (f32 ? 4 : 8) == 0;
  const dim3 grid(blocks_x((int64_t)p->T * p->row_bytes), (unsigned)(p->n_frag < 65535 ? p->n_frag : 65535));
  if (f32)
    hipLaunchKernelGGL(units_pack_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, *p, vec);
  else
    hipLaunchKernelGGL(units_pack_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, *p, vec);
  return zs_check_launch("zs_units_pack");
}

// zs_pool.hip -- training batches gathered out of a dataset held in device memory (zs_pool_gather, include/zs_amd.h): B segments
// of seg_len * F floats copied out of the pool into the step's x input, their speaker ids into c, and the batch cursor advanced
// on the device so that a replayed launch with frozen arguments serves the next batch.
//
// Alignment.  A pool row is F floats (513: 2 052 bytes), so a segment's source starts on a 4-byte boundary and only one segment in
// four shares the 16-byte phase of its destination.  The wide, 16-byte-aligned side is the DESTINATION (b * seg_len * F * 4 bytes into
// a 16-byte-aligned x: aligned whenever seg_len * F is a multiple of 4; a scalar head and tail cover every other case).  The SOURCE
// is read with 16-byte loads that carry 4-byte alignment only: gfx950 global loads of four dwords need dword alignment, no more
// (the same choice as zs_frag_gather).  No LDS, no atomics; every store is a plain vector store.
#include "zs_common.h"

namespace {

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int NT = 256;        // threads per block
constexpr int UNROLL = 4;      // 16-byte loads in flight per thread before the first store

// Block (bx, b): segment b = blockIdx.y (+ gridDim.y ...), its floats strided over the gridDim.x blocks in 16-byte steps of the
// destination.  Every block reads the cursor; nobody writes it in this launch (cursor_bump_kernel runs behind it on the stream).
__global__ void __launch_bounds__(NT) pool_gather_kernel(const ZsPoolGather p) {
  const uint64_t k = (uint64_t)*p.cursor;
  const uint64_t S = (uint64_t)p.world * (uint64_t)p.B, n = (uint64_t)p.n;
  const uint64_t passes = (n + S - 1) / S;
  const uint64_t P = passes > 2 ? passes - 1 : 1;
  const uint64_t base = (k % P) * S + (uint64_t)p.rank * (uint64_t)p.B;
  const int64_t len = (int64_t)p.seg_len * p.F;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  for (int64_t b = blockIdx.y; b < p.B; b += gridDim.y) {
    const uint64_t item = (base + (uint64_t)b) % n;
    const float* src = p.pool + p.first[item] * (int64_t)p.F;
    float* dst = p.x + b * len;
    if (tid == 0) p.c[b] = (int64_t)p.speaker[item];
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
  }
}

__global__ void cursor_bump_kernel(int64_t* cursor) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *cursor += 1;
}

}  // namespace

extern "C" int zs_pool_gather(const ZsPoolGather* p, void* stream) {
  ZS_REQUIRE(p && p->pool && p->speaker && p->first && p->cursor && p->x && p->c, "zs_pool_gather: null operand");
  ZS_REQUIRE(p->B > 0 && p->seg_len > 0 && p->F > 0, "zs_pool_gather: B, seg_len and F must be > 0");
  ZS_REQUIRE(p->world > 0 && p->rank >= 0 && p->rank < p->world, "zs_pool_gather: need 0 <= rank < world");
  ZS_REQUIRE(p->n >= (int64_t)p->world * p->B, "zs_pool_gather: the item table is shorter than one global batch (n < world * B)");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->pool) & 3) == 0 && (reinterpret_cast<uintptr_t>(p->x) & 3) == 0,
             "zs_pool_gather: pool and x must be 4-byte aligned");
  ZS_REQUIRE((reinterpret_cast<uintptr_t>(p->c) & 7) == 0 && (reinterpret_cast<uintptr_t>(p->first) & 7) == 0 &&
             (reinterpret_cast<uintptr_t>(p->cursor) & 7) == 0, "zs_pool_gather: c, first and cursor must be 8-byte aligned");
  const int64_t len = (int64_t)p->seg_len * p->F;
  int64_t bx = (len / 4 + UNROLL * NT - 1) / (UNROLL * NT);     // UNROLL 16-byte copies per thread
  if (bx < 1) bx = 1;
  if (bx > 64) bx = 64;
  const unsigned by = (unsigned)(p->B < 65535 ? p->B : 65535);
  hipLaunchKernelGGL(pool_gather_kernel, dim3((unsigned)bx, by), dim3(NT), 0, (hipStream_t)stream, *p);
  int rc = zs_check_launch("zs_pool_gather");
  if (rc || !p->advance) return rc;
  hipLaunchKernelGGL(cursor_bump_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p->cursor);
  return zs_check_launch("zs_pool_gather.cursor");
}

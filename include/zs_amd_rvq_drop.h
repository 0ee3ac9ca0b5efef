/* zs_amd_rvq_drop.h -- quantiser dropout for training through the residual codebook (--rvq_dropout): zs_rvq_drop_draw,
 * zs_rvq_commit_drop and zs_rvq_gather_frag.  The conventions are include/zs_amd.h's (error codes, dtypes, caller-owned buffers,
 * stream-ordered launches), and zs_amd._lib derives the ctypes signatures of this header exactly as it derives those of zs_amd.h.  A
 * header of its own: zs_amd.h is the ABI the earlier parts of the project count on as it stands. */
#ifndef ZS_AMD_RVQ_DROP_H
#define ZS_AMD_RVQ_DROP_H
#include "zs_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Quantiser dropout (zs_amd.rvq_train with dropout, --rvq_dropout P): every sample (fragment) b of the batch is decoded from its own
 * number of stages s_use[b] in [1, S], drawn on the device, so that every coarser bitrate of a residual unit file is a trained
 * operating point.  One training iteration is zs_rvq_drop_draw, then for every stage s in increasing order zs_vq_assign ->
 * zs_rvq_commit_drop -> zs_vq_accum -> zs_vq_ema (-> zs_vq_restart), all but the second unchanged, then zs_rvq_loss (unchanged) and
 * zs_rvq_gather_frag in the forward and zs_rvq_st_bwd (unchanged) in the backward.  A null struct, a size out of range, a leading
 * dimension below E, a null operand with work to do, a misaligned operand or a forbidden overlap return ZS_EINVAL and launch nothing.
 * Caller-owned buffers, no allocation, no synchronisation, stream-ordered; no launch argument depends on the iteration, so a captured
 * graph replays them, and the draw reads the step's seed word from the device, so a replay draws anew.  No float atomics and no fused
 * multiply-add: every result is bitwise equal from run to run.
 *
 * zs_rvq_drop_draw: the stage counts of n_frag samples.  With wrapping unsigned 64-bit arithmetic, mix64 as zs_vq_restart states it
 * (zs_amd.h) and seed_ptr optional (8-byte aligned):
 *   u_b       = mix64(seed + *seed_ptr + ZS_RVQ_DROP_SALT + b * 0x9E3779B97F4A7C15)
 *   drop_b    = (u_b >> 40) < thr                      thr = floor(P * 2^24), an integer the caller computes; P = 1: every sample
 *   s_use[b]  = drop_b ? 1 + (u_b & 0xFFFFFFFF) % S : S                                             (int32 [n_frag])
 *   active[s] = rows_per_frag * #{b : s_use[b] > s}    written, not accumulated                     (int32 [S])
 * 1 <= S <= ZS_RVQ_MAX_S, 1 <= thr <= ZS_RVQ_DROP_THR_ONE, 1 <= n_frag <= ZS_UNITS_MAX_FRAG, rows_per_frag >= 1 and n_frag *
 * rows_per_frag < 2^31.  One workgroup of 256 lanes: lane t draws b = t, t + 256, .. and the integer counts are added over the
 * workgroup (integers: any order gives the same words). */
#define ZS_RVQ_DROP_SALT 5933019028717195088         /* 0x5256515F44524F50, the bytes of "RVQ_DROP" */
#define ZS_RVQ_DROP_THR_ONE 16777216
typedef struct {
  uint64_t seed;
  const uint64_t* seed_ptr;
  int32_t thr, S, n_frag, rows_per_frag;
  int32_t* s_use; int32_t* active;
} ZsRvqDropDraw;
int zs_rvq_drop_draw(const ZsRvqDropDraw* p, void* stream);
/* zs_rvq_commit_drop: zs_rvq_commit of stage `stage` where only some rows take part.  Every field of ZsRvqCommit with its meaning
 * and its checks, plus s_use int32 [ceil(n / rows_per_frag)] (required, 4-byte aligned), rows_per_frag >= 1 and 0 <= stage <
 * ZS_RVQ_MAX_S; `first` must be (stage == 0).  Row i belongs to fragment b(i) = i / rows_per_frag, act(i) = stage < s_use[b(i)]:
 *   act(i):   r, x_f32, idx_acc, a, the row's terms of partial, *bad and *over are zs_rvq_commit's, bit for bit
 *   !act(i):  r[i][j] = (float) x[i][j] for j < E (the value copied, no arithmetic), x_f32[i] likewise when given, a[i] is neither read
 *             nor written, idx_acc[i] = -1, the row adds nothing to partial and bumps neither *bad nor *over, and idx[i] is not read
 * A count s_use[b] <= 0 makes every stage of that fragment inactive (stage 0 too: a[i] is then not initialised), one above S every
 * stage active; the caller's counts come from zs_rvq_drop_draw, which writes neither.  partial[w] as zs_rvq_commit states it, tail
 * zeroed.  zs_rvq_commit's layout: a row is owned by a team of 2^t <= 64 lanes of one wave, four columns per lane and round, 16-byte
 * pieces where alignment and pitch allow, one pass over the row; a wave may hold teams of different fragments, active and not, and
 * every lane runs the same number of rounds and takes part in every shuffle. */
typedef struct {
  int32_t dtype, src_f32, first;
  const void* x; int64_t n, ld_x;
  const int32_t* idx;
  const float* code; int64_t ld_code; int32_t K, E;
  float* r; int64_t ld_r;
  float* x_f32; int64_t ld_xf;
  int32_t* idx_acc;
  float* a; int64_t ld_a;
  double* partial;
  int32_t* bad; int32_t* over;
  const int32_t* s_use;
  int32_t rows_per_frag, stage;
} ZsRvqCommitDrop;
int zs_rvq_commit_drop(const ZsRvqCommitDrop* p, void* stream);
/* zs_rvq_gather_frag: zs_rvq_gather with a stage count per fragment.  Every field of ZsRvqGather with its meaning and its checks,
 * s_use being int32 [n_frag] on the device (required, 4-byte aligned) in place of the scalar:
 *   dst[f][t][c] = cast(((code[0][k_0][c] + code[1][k_1][c]) + ..) + code[s_use[f] - 1][k_{s_use[f] - 1}][c])     t < len[f], c < E
 * and zero elsewhere, as there; the planes s >= s_use[f] are not read for fragment f.  A fragment whose count is outside [1, S]
 * writes zero rows and *bad += 1 for each of its len[f] frames (when its start and len are a range of the planes; a fragment that is
 * none is a zero fragment and counts nothing, as in zs_rvq_gather); no index of such a fragment is read.  With every s_use[f] == s the
 * operand and *bad are zs_rvq_gather(s_use = s)'s, bit for bit. */
typedef struct {
  int32_t dtype;
  const int32_t* idx; int64_t n_idx, ld_idx; int32_t S;
  const int32_t* s_use;
  const float* code; int64_t ld_code, plane_code; int32_t K, E;
  const int64_t* start; const int32_t* len; int32_t n_frag, T;
  void* dst; int64_t ld_dst; int32_t* bad;
} ZsRvqGatherFrag;
int zs_rvq_gather_frag(const ZsRvqGatherFrag* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif

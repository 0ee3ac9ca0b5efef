/* zs_amd_segment.h -- the segmentation entry points of libzs_amd.so (--segment): zs_vq_scores, zs_code_scores and
 * zs_seg_viterbi.  The conventions are include/zs_amd.h's (error codes, dtypes, caller-owned buffers, stream-ordered launches), and
 * zs_amd._lib derives the ctypes signatures of this header exactly as it derives those of zs_amd.h.  A header of its own: zs_amd.h is
 * the ABI the earlier parts of the project count on as it stands. */
#ifndef ZS_AMD_SEGMENT_H
#define ZS_AMD_SEGMENT_H
#include "zs_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Segmentation (zs_amd.segment, --segment): the index sequence of a whole utterance chosen at once under a codebook,
 *   minimise  sum_t score(t, k_t) + lambda * #{ t >= 1 : k_t != k_(t-1) },
 * an exact dynamic programme over T frames and K <= ZS_SEG_MAX_K codewords whose output is a sequence of runs (codeword, duration).
 * The scores of a batch are kept by zs_vq_scores (vector codebook) or zs_code_scores (bit codebook); zs_seg_viterbi chooses the paths.
 * All three follow the zs_vq_* conventions: caller-owned buffers, no allocation, no synchronisation, stream-ordered; a null struct, a
 * size out of range, a pitch below K (below E for the operands), a misaligned operand or a null operand with work to do return
 * ZS_EINVAL and launch nothing; n == 0 (n_utt == 0) succeeds and launches nothing.
 *
 * zs_vq_scores: the operands of zs_vq_assign (x of `dtype`, fp32 when src_f32; code, cnorm, K, E) ->
 *   scores[i][k] = the score s(i, k) zs_vq_assign computes for that pair, bitwise: cnorm[k] - 2 acc, -0 written as +0
 * scores fp32 [n][ld_s], ld_s >= K; the columns k >= K are never written.  The kernel is zs_vq_assign's tile loop (one device
 * function compiled into both, over the same zero-padded columns) with a store epilogue: a lane holds 4 consecutive codewords of one
 * row per accumulator group and stores them as one 16-byte piece where scores and ld_s allow (single elements otherwise).
 * 1 <= K <= ZS_SEG_MAX_K. */
#define ZS_SEG_MAX_K 4096
typedef struct {
  int32_t dtype, src_f32;
  const void* x; int64_t n, ld_x;
  const float* code; int64_t ld_code; const float* cnorm; int32_t K, E;
  float* scores; int64_t ld_s;
} ZsVqScores;
int zs_vq_scores(const ZsVqScores* p, void* stream);
/* zs_code_scores: the operands and masking rules of zs_code_assign (bit-packed units and codewords, columns >= E ignored) ->
 *   scores[i][k] = (float) Hamming distance of unit i and codeword k over the columns < E       (exact: <= 1024)
 * scores fp32 [n][ld_s], ld_s >= K, columns k >= K never written; 0 <= n < 2^31, 1 <= K <= ZS_SEG_MAX_K.  One unit row per lane in
 * registers, the codewords through LDS in zs_code_assign's tiles (one staging function compiled into both). */
typedef struct {
  const uint8_t* units; int64_t n; int32_t row_bytes;
  const uint8_t* code; int32_t K, code_bytes, E;
  float* scores; int64_t ld_s;
} ZsCodeScores;
int zs_code_scores(const ZsCodeScores* p, void* stream);
/* zs_seg_viterbi.  Utterance u is the units uoffs[u] .. uoffs[u + 1] - 1 (uoffs int64 [n_utt + 1], 0 <= uoffs[u] <= uoffs[u + 1] <=
 * n_units); the score row of unit i is row[i] (int64 [n_units]), or i when row is NULL (then n_rows >= n_units).  scores fp32
 * [n_rows][ld_s], ld_s >= K; columns >= K are never read.  lam is fp32, finite and >= 0.  For one utterance of T >= 1 frames with the
 * scores s[t][k] of its rows (fl32: one fp32 rounding):
 *   c_0[k] = s[0][k]
 *   m_t = min_k c_t[k],   a_t = the lowest k that attains it
 *   for t >= 1:
 *       d       = fl32(c_(t-1)[k] - m_(t-1))                                   (>= 0)
 *       (p, sw) = the lexicographically smaller of (d, k) [stay, sw = 0] and (lam, a_(t-1)) [switch, sw = 1]
 *       c_t[k]  = fl32(s[t][k] + p)
 *   k_(T-1) = a_(T-1);   k_(t-1) = sw_t[k_t] ? a_(t-1) : k_t
 *   cost    = sum_t (double) m_t                                               (added in increasing t, in double)
 *   n_seg   = 1 + #{ t >= 1 : k_t != k_(t-1) }
 * One rounding per written operation, no fused multiply-add.  The renormalisation by m keeps the costs bounded for utterances of any
 * length.  The tie rule is lexicographic (-0 and +0 are one value), so at lam == 0 the path is the per-frame lowest-index argmin:
 * what the assign kernels return.  Outputs:
 *   idx[uoffs[u] + t] = k_t        (int32 [n_units])
 *   n_seg[u], cost[u]              (int32 / double [n_utt], optional)
 * T == 0 writes no idx and gives n_seg 0, cost 0.  A row[] entry outside [0, n_rows) is never used as an index: every idx entry of
 * that utterance becomes -1, its n_seg 0 and cost 0, and *bad += 1 (int32); an utterance whose uoffs are not a range of units has
 * nothing written to idx and is counted in *bad as well.  With scores that are not finite the indices written still lie in [0, K)
 * and nothing is read or written out of bounds; which path comes out is unspecified.
 * `work` (8-byte aligned, ZS_SEG_WORK_BYTES(n_units, K) bytes; its layout is private) holds the switch bits and a_t.
 * One workgroup per utterance (the grid strides beyond 1024); a lane keeps at most 16 states in registers, which is what
 * ZS_SEG_MAX_K = 16 x 256 lanes means.  The kernel is LATENCY-BOUND by construction -- one barrier-separated reduction per frame, and
 * a frame depends on the frame before -- so its measure is microseconds per frame: measured on one long utterance 0.67 - 0.89 at K = 64,
 * 1.20 - 1.43 at K = 1024 and 2.98 - 3.24 at K = 4096, the lower figure where lambda joins frames.  Bitwise reproducible. */
#define ZS_SEG_WORK_BYTES(n_units, K) ((int64_t)(n_units) * (8 * (((int64_t)(K) + 63) / 64) + 4))
typedef struct {
  const float* scores; int64_t n_rows, ld_s;
  const int64_t* uoffs; int64_t n_utt;
  const int64_t* row; int64_t n_units;
  float lam; int32_t K;
  void* work; int64_t work_bytes;
  int32_t* idx; int32_t* n_seg; double* cost; int32_t* bad;
} ZsSegViterbi;
int zs_seg_viterbi(const ZsSegViterbi* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif

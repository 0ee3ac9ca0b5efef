/* zs_amd_abx.h -- the scoring entry points of libzs_amd.so (--score_units): zs_abx_rownorm, zs_abx_dtw and zs_abx_count.
 * The conventions are include/zs_amd.h's (error codes, caller-owned buffers, stream-ordered launches), and zs_amd._lib derives the
 * ctypes signatures of this header exactly as it derives those of zs_amd.h.  A header of its own: zs_amd.h and the two headers beside
 * it are the ABI the earlier parts of the project count on as they stand. */
#ifndef ZS_AMD_ABX_H
#define ZS_AMD_ABX_H
#include "zs_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * ABX scoring (zs_amd.abx, --score_units).  A token is a run of at most ZS_ABX_MAX_LEN unit rows; the distance of two tokens is a
 * dynamic time warp over the frame distances of their rows, and a triplet (A, B, X) is won when d(A, X) < d(B, X).  The frame scores
 * of a tile of rows come from zs_code_scores / zs_vq_scores (zs_amd_segment.h); zs_abx_dtw turns rectangles of that tile into
 * distances and zs_abx_count counts the triplets won from rows of the distance matrix.  All three follow the zs_seg_viterbi
 * conventions: caller-owned buffers, no allocation, no synchronisation, stream-ordered; a null struct, a size out of range, a pitch
 * below the width, a misaligned operand or a null operand with work to do return ZS_EINVAL and launch nothing; zero work succeeds
 * and launches nothing.  (fl32: one fp32 rounding; nothing below is fused into a multiply-add.)
 *
 * zs_abx_rownorm: x fp32 [n][ld_x], ld_x >= E >= 1 ->
 *   rinv[i] = fl32(1 / fl32(sqrt(s_i))),  s_i = the fp32 sum of x[i][e]^2 over the columns e < E (summation order unspecified);
 *   rinv[i] = 0 where s_i == 0.
 * One wave per row, the grid strides over the rows. */
#define ZS_ABX_MAX_LEN 64
#define ZS_ABX_HAMMING 0
#define ZS_ABX_ANGULAR 1
typedef struct {
  const float* x; int64_t n, ld_x; int32_t E;
  float* rinv;
} ZsAbxRownorm;
int zs_abx_rownorm(const ZsAbxRownorm* p, void* stream);

/* zs_abx_dtw.  scores S fp32 [n_rows][ld_s], ld_s >= n_cols; columns >= n_cols are never read.  Record r names the rectangle of token
 * p (rows row0 .. row0 + La - 1 of S) against token q (columns col0 .. col0 + Lb - 1).  The frame distance of row i of p and row j
 * of q, with s = S[row0 + i][col0 + j]:
 *   metric ZS_ABX_HAMMING:  g = fl32(s / (float) E)
 *   metric ZS_ABX_ANGULAR:  c = clamp(fl32(fl32(fl32(-0.5 * s) * rinv_row[row0 + i]) * rinv_col[col0 + j]), -1, 1)
 *                           g = fl32(acosf(c) * (1 / pi))         (rinv_row fp32 [n_rows], rinv_col fp32 [n_cols]; S = -2 x.c)
 * The distance is built over (cost, len) pairs in lexicographic order, cost fp32, len an integer:
 *   C[0][0] = (g(0,0), 1)
 *   C[i][j] = (fl32(g(i,j) + m.cost), m.len + 1),   m = the least of C[i-1][j-1], C[i-1][j], C[i][j-1] that exist
 *   d       = fl32(C[La-1][Lb-1].cost / (float) len)
 * Every cell has one value and no reduction order is open: given S, d is bitwise reproducible (tests/abx_ref.py restates it in numpy
 * float32).  A tie in cost goes to the shorter path.  d is written to out[dst0] and, unless dst1 == -1, to out[dst1] (out fp32
 * [n_out]).  A record is invalid when a length is outside [1, ZS_ABX_MAX_LEN], its rectangle leaves S, dst0 is outside [0, n_out) or
 * dst1 outside [-1, n_out): it reads nothing of S, writes NaN to those of its destinations that lie inside out, and adds 1 to *bad
 * (int32).  With scores that are not finite the results are unspecified and every access stays in bounds.
 * A wave holds 64 / width records, one lane per column of q: width is 4, 8, 16, 32 or 64 (0: 64) and says how the caller bucketed
 * the records of this call.  It changes no result: a record whose Lb exceeds width is run by its whole wave behind the others.  The
 * rectangle is staged through LDS row by row (a group reads Lb consecutive floats of a row), the sweep runs along anti-diagonals
 * and takes the left neighbour's value by a one-lane shift: __shfl_up, or DPP wave_shr when `dpp` is not 0 (the same results).
 * 0 <= n_pairs < 2^31, n_rows and n_cols < 2^31, 1 <= E. */
typedef struct { int32_t row0, La, col0, Lb; int64_t dst0, dst1; } ZsAbxPair;
typedef struct {
  const float* scores; int64_t n_rows, n_cols, ld_s;
  const float* rinv_row; const float* rinv_col;
  int32_t metric, E, width, dpp;
  const ZsAbxPair* pairs; int64_t n_pairs;
  float* out; int64_t n_out;
  int32_t* bad;
} ZsAbxDtw;
int zs_abx_dtw(const ZsAbxDtw* p, void* stream);

/* zs_abx_count.  d fp32 [n][ld_d], ld_d >= n_cols.  Job j = {x, a0, a1, b0, b1, skip} ->
 *   wins2[j] = sum over A in [a0, a1), A != skip, and B in [b0, b1) of  2 * [d[x][A] < d[x][B]] + [d[x][A] == d[x][B]]      (uint64)
 * twice the score of the triplets (A, B, X = x), an exact integer; a comparison with a NaN adds 0.  An empty set gives 0.  A job is
 * invalid when x is outside [0, n) or a range is not inside [0, n_cols] (0 <= a0 <= a1 <= n_cols, the same for b): wins2[j] = 0 and
 * *bad += 1 (int32).  One workgroup per job (the grid strides beyond 65535 x 16): the B values go through LDS in tiles of 1024, a
 * thread keeps one A per round. 0 <= n_jobs < 2^31. */
typedef struct { int32_t x, a0, a1, b0, b1, skip; } ZsAbxJob;
typedef struct {
  const float* d; int64_t n, n_cols, ld_d;
  const ZsAbxJob* jobs; int64_t n_jobs;
  uint64_t* wins2; int32_t* bad;
} ZsAbxCount;
int zs_abx_count(const ZsAbxCount* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif

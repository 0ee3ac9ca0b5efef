/* zs_amd.h -- C ABI of libzs_amd.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * ASR-TTS autoencoder hot path of andi611/ZeroSpeech-TTS-without-T.
 *
 * The reference has no FFI / plugin seam (it is pure Python on torch.nn); this ABI is the inner
 * seam of the drop-in Python surface (zs_amd.model / zs_amd.trainer / zs_amd.convert).  Each entry
 * point states which reference arithmetic it replaces (file:line into the reference repository).
 *
 * Conventions
 *  - Every function returns 0 on success or a negative ZS_E* code; zs_last_error() gives text.
 *    Nothing is thrown across the boundary.
 *  - The caller owns every buffer (including workspaces).  The library never allocates, frees or
 *    synchronises; every call only enqueues kernels on `stream` (hipStream_t passed as void*), so
 *    calls are stream-ordered, re-entrant and hipGraph-capturable.
 *  - Activations are channels-last: a tensor [B, T, C] is stored as B*T rows of `ld` elements
 *    (ld >= C, ld a multiple of 32 elements unless stated).  Columns [C, ld) of an activation that
 *    feeds a GEMM must hold zeros; every kernel here writes them as zeros.
 *  - dtype: ZS_F32 (exact-fp32 path on v_mfma_f32_32x32x2_f32) or ZS_BF16 (bf16 storage,
 *    v_mfma_f32_32x32x16_bf16, fp32 accumulate).  Statistics, gradients of parameters, optimizer
 *    state and losses are always fp32.
 */
#ifndef ZS_AMD_H
#define ZS_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_ABI_VERSION 1

enum { ZS_F32 = 0, ZS_BF16 = 1 };
enum { ZS_OK = 0, ZS_EINVAL = -1, ZS_ELAUNCH = -2, ZS_EWORKSPACE = -3 };
enum { ZS_PAD_ZERO = 0, ZS_PAD_REFLECT = 1 };
enum { ZS_ACT_NONE = 0, ZS_ACT_LRELU = 1, ZS_ACT_SIGMOID = 2, ZS_ACT_TANH = 3 };
enum { ZS_STORE_ROWS = 0, ZS_STORE_SPLIT2 = 1 };   /* SPLIT2 = pixel_shuffle_1d by 2 (see below) */
enum { ZS_RES_NONE = 0, ZS_RES_IDENTITY = 1, ZS_RES_AVGPOOL2 = 2, ZS_RES_UPSAMPLE2 = 3 };

int zs_abi_version(void);
const char* zs_last_error(void);
/* Kernel-selection knobs, one line each: "key" (environment variable that gives the default at first use, or -; default): effect.
 *   "gemm_dma" (ZS_GEMM_DMA, 1): zs_gemm_conv stages operands by LDS-DMA; 0 = the register-staged kernel
 *   "gemm_ring" (ZS_GEMM_RING, 1): allow the 256x128 3-stage-ring kernel
 *   "gemm_ring_min_tiles" (ZS_GEMM_RING_MIN_TILES, 256): ... when the problem has at least that many 256x128 tiles
 *   "gemm_pp" (ZS_GEMM_PP, 1): ping-pong schedule of the ring kernel (two wave groups one barrier apart)
 *   "gemm_p8" (ZS_GEMM_P8, 1): 256x256 quadrant ping-pong kernel when the packed weight has a multiple of 256 rows
 *   "gemm_p8_min_tiles" (ZS_GEMM_P8_MIN_TILES, 200): ... and the problem has at least that many 256x256 tiles
 *   "gemm_dma64" (ZS_GEMM_DMA64, 1): 64-row tiles of the LDS-DMA kernel for under-filled grids
 *   "gemm_dma64_max_tiles" (ZS_GEMM_DMA64_MAX_TILES, 256): ... when twice the 128-row tile count is at most this
 *   "wgrad_p8" (ZS_WGRAD_P8, 1): bf16 weight gradients by the 256x256 ping-pong kernel where the plan accepts the shape; 0 = never, 2 = always
 *   "wgrad_p8_waste" (ZS_WGRAD_P8_WASTE, 135): ... only while the padded output area is at most this / 100 of the real one
 *   "wgrad_wgs" (ZS_WGRAD_WGS, 256): workgroups the split-K plan of the 256x256 weight-gradient kernel aims for
 *   "wgrad_wgs128" (ZS_WGRAD_WGS128, 448): workgroups the split-K plan of the 128x128 weight-gradient kernels aims for
 *   "wgrad_slab_cost" (ZS_WGRAD_SLAB_COST, 13): cost of one split's slab write + re-read in K-tile times (256x256 split-K plan)
 *   "wgrad_alone" (ZS_WGRAD_ALONE, 0): weight gradients run alone on the chip (set by the context): the plan uses the two "_alone" knobs
 *   "wgrad_wgs128_alone" (ZS_WGRAD_WGS128_ALONE, 448): "wgrad_wgs128" while "wgrad_alone" is set
 *   "wgrad_slab_cost_alone" (ZS_WGRAD_SLAB_COST_ALONE, 13): "wgrad_slab_cost" while "wgrad_alone" is set
 *   "wgrad_dma" (ZS_WGRAD_DMA, 1): bf16 128x128 weight-gradient tiles by LDS-DMA; 0 = register-staged (bit-identical at equal splits)
 *   "wgrad_reduce_taps" (ZS_WGRAD_REDUCE_TAPS, 1): Conv1d weight gradients reduced with stores in dW order; 0 = per-(co, tap) rows (bit-identical)
 *   "gru_persist" (ZS_GRU_PERSIST, 1): one persistent launch per GRU pass where H allows and the grid fits one workgroup per CU
 *   "gru_wide" (ZS_GRU_WIDE, 1): bf16, H in {128, 256, 512}: the persistent kernels' 16-row x 64-unit tiling
 *   "gru_spin_limit" (ZS_GRU_SPIN_LIMIT, 2097152): granule sweeps a persistent GRU wave waits for its group (see ZsGruFwd.status); 0 = timeout
 *   "gru_xcd_groups" (ZS_GRU_XCD_GROUPS, 1): WIDE hand-off BPTT launches whose (row groups x 2) is a multiple of 8 order their grid
 *       so that the H/64 workgroups of a group share an XCD (placement only, bit-identical results); 0 = unit chunk fastest
 *   "gru_solo_max_h" (ZS_GRU_SOLO_MAX_H, 128): WIDE launches with H = 128 <= this run the one-workgroup kernels (see zs_gru_solo); 0 = the
 *       hand-off kernels.  Not planned while "gru_spin_limit" is 0: that setting exists to force the hand-off's timeout
 *   "norm_wide" (-, 1): InstanceNorm kernels in 8 row groups x 256 channels for short bf16 samples
 *   "norm_lim0" (-, 64): longest T that zs_instnorm_fwd runs in the 8 x 256 decomposition
 *   "norm_lim1" (-, 32): longest T that zs_instnorm_bwd runs in the 8 x 256 decomposition
 *   "norm_lim2" (-, 64): longest T that zs_grad_combine runs in the 8 x 256 decomposition
 *   "gl_prefetch" (-, 1): Griffin-Lim waves request the next inverse frame's spectrum behind the current transform
 *   "gl_chains" (-, 3): independent launch chains of zs_griffin_lim (see there)
 *   "adam_pack" (ZS_ADAM_PACK, 1): the counted optimizer step (NetOpt.device_step) runs zs_adam_pack; 0 = zs_adam_clip + re-pack
 * Stored values are normalised: gru_persist, gru_wide, norm_wide and gl_prefetch store v ? 1 : 0, gl_chains is clamped to [1, 4],
 * norm_lim0..2 store v, every other knob stores max(v, 0).  The knobs are process-wide atomics: they may be set from any thread; a
 * launch reads each knob once.  Returns the previous value, or ZS_EINVAL for an unknown key. */
int zs_set_option(const char* key, int value);
int zs_get_option(const char* key);                /* the stored value, or ZS_EINVAL for an unknown key */

/* ---------------------------------------------------------------------------------------------
 * zs_gemm_conv: implicit-GEMM Conv1d / Linear / transposed-conv (data gradient) on MFMA.
 *   out[m, n] = epilogue( sum_{j<taps} sum_{ci<cin_pad} A[row(m, j), ci] * W[n, j*cin_pad + ci] )
 *   m = b*T_out + t.  gather 0 (forward):  row = reflect_or_zero(t*stride + j - pad_left) in [0,T_in)
 *                     gather 1 (dgrad):    u = t; s = u - j; row = s/stride if s>=0, s%stride==0,
 *                                          s/stride < T_in, else a zero row.
 * Replaces: pad_layer()+nn.Conv1d (model/model.py:20-40), linear() (model/model.py:69-78), the GRU
 * input/recurrent products of nn.GRU (model/model.py:59-66), and their autograd data gradients.
 * Epilogue order: +bias[n] -> +pre_vec[vec_idx[b]][n] -> act (-> colsum) -> *lrelu'(dact_src[m][n]) ->
 *                 +add_src[m][n] -> store out (-> out2 = value + vec2[vec_idx[b]][col]).
 * ZS_STORE_SPLIT2 realises pixel_shuffle_1d (model/model.py:43-51) for weights whose output
 * channels were packed as n' = r*(N/2) + c:  (m, n') -> row 2m + (n' >= N/2), col n' mod (N/2).
 * `groups` > 1 launches independent problems that differ by the *_gstride element offsets.
 */
typedef struct {
  int32_t dtype;
  const void* A; int64_t lda; int64_t a_batch_stride;
  int32_t B, T_in, T_out;
  int32_t taps, stride, pad_left, pad_mode, gather;
  int32_t cin_pad;                 /* K per tap: a whole number of 128-byte chunks (multiple of 64 bf16 / 32 fp32).
                                      A rows are read up to cin_pad columns: bytes past C must be finite (zeros or the
                                      next row), the matching W columns are zero */
  const void* W; int64_t ldw;      /* packed [n_pad][ldw], ldw >= taps*cin_pad, zero padded */
  int32_t N, n_pad;                /* valid columns; packed rows (multiple of 128) */
  const float* bias;
  const float* pre_vec; int64_t pre_vec_ld; const int64_t* vec_idx;
  int32_t act; float slope;
  const void* dact_src; int64_t dact_ld;
  const void* add_src; int64_t add_ld; int32_t add_f32;
  void* out; int64_t ldc; int32_t out_f32; int32_t out_cols; int32_t store_mode;
  void* out2; int64_t ldc2; int32_t out2_cols; int32_t store_mode2;
  const float* vec2; int64_t vec2_ld;
  int32_t groups; int64_t a_gstride, w_gstride, out_gstride, bias_gstride;
  /* optional per-sample column sums of the value BEFORE dact_src / add_src (the per-sample part of nn.Embedding's backward
   * where an embedding row was added to this GEMM's input, model/model.py:319,336,353; finished by zs_emb_scatter):
   *   colsum[b][n - colsum_col0] += sum_t value[b*T_out + t][n]      for colsum_col0 <= n < N   (colsum_post: of `out`)
   * One owner per (b, n): plain read-modify-write, no atomics.  Needs T_out | 128 (whole samples per tile). */
  float* colsum; int64_t colsum_ld; int32_t colsum_col0;
  int32_t colsum_post;             /* 1: sum the STORED value (after dact_src / add_src) instead */
  /* ragged batch (inference: the tail fragments of convert.py:154-165 have 128..254 frames each and the reference runs them one
   * by one): sample b has lengths[b] <= T_in valid input rows and (lengths[b] + pad_left + pad_right - taps) / stride + 1 valid
   * output rows; the padding (reflect / zero) is applied at EACH sample's own end, exactly as if the sample ran alone.  Output
   * rows past a sample's length are computed from zero rows (finite, never read by a length-aware consumer).  T_in / T_out stay
   * the row strides of the batch.  gather 0 only; B < 65536, T_in < 32768.  null = every sample has T_in rows. */
  const int32_t* lengths; int32_t pad_right;
  /* 2-D convolution (w_in > 0; nn.Conv2d of the stage-2 critic, model/model.py:113-173, on channels-last [B, H*W, C] rows): a
   * sample's T_in rows are an (T_in / w_in) x w_in image, its T_out output rows an (T_out / w_out) x w_out image, tap
   * j = kw*taps_h + kh (kw = j / taps_h along the row, kh = j % taps_h across rows: the order of nn.Conv2d's weight [co][ci][kw][kh]
   * when W is the frequency axis); the gather rule above applies per axis with the same stride, pad_left and pad_mode.
   * 0 = the 1-D convolution over T.  Not with lengths. */
  int32_t w_in, w_out, taps_h;
} ZsGemmConv;
int zs_gemm_conv(const ZsGemmConv* p, void* stream);
/* zs_gemm_conv_path: the kernel a zs_gemm_conv launch of *p would take now, under the current knobs -- the same plan function the
 * launch calls (argument checks and dispatch; tile counts below are of M = B*T_out rows by N columns).  Returns
 * path | regs_epilogue << 8, or the negative code zs_gemm_conv would return for these arguments.  It reads the struct and the
 * knobs only: A, W, out, ... are tested for null and alignment, never dereferenced, and no GPU call is made.
 *   P8:      256x256 quadrant ping-pong kernel: "gemm_dma", "gemm_p8", n_pad % 256 == 0, at least "gemm_p8_min_tiles" 256x256 tiles;
 *   RING_PP / RING: 256x128 3-stage ring, ping-pong ("gemm_pp") or lock-step: else, with "gemm_dma" and "gemm_ring", at least
 *            "gemm_ring_min_tiles" 256x128 tiles;
 *   DMA64:   LDS-DMA kernel, 64-row tiles: else, with "gemm_dma" and "gemm_dma64", twice the 128x128 tile count at most
 *            "gemm_dma64_max_tiles" and, for a colsum launch, T_out | 64;
 *   DMA128:  LDS-DMA kernel, 128x128 tiles: every other launch with "gemm_dma";   REG: register-staged 128x128 kernel ("gemm_dma" 0).
 * regs_epilogue (bit 8): a P8 bf16 launch finishes its tile in the register epilogue, which stages the tile as bf16 BEFORE the
 * dact_src mask / add_src (two roundings) and sums colsum over the staged bf16 values; it needs bf16 `out` (no out_f32) with
 * out_cols % 8 == 0, 16-byte aligned out / out2 / dact_src / add_src rows, no add_f32, no out2 together with dact_src / add_src,
 * T_out % 16 == 0 with pre_vec / vec2, (N / 2) % 8 == 0 with SPLIT2, act NONE or LRELU, T_out | 256 and no out2 with colsum.
 * 0 on every other path and for fp32.
 * `groups` > 1: no Python caller passes it; the library's own STEP_GEMM GRU path does (2 directions) and tests it there. */
enum { ZS_GEMM_PATH_P8 = 0, ZS_GEMM_PATH_RING_PP = 1, ZS_GEMM_PATH_RING = 2, ZS_GEMM_PATH_DMA64 = 3, ZS_GEMM_PATH_DMA128 = 4,
       ZS_GEMM_PATH_REG = 5 };
int zs_gemm_conv_path(const ZsGemmConv* p);

/* ---------------------------------------------------------------------------------------------
 * zs_gemm_wgrad: weight gradient of the same convolution,
 *   dW[co, ci, j] = sum_m dY[m, co] * X[row(m, j), ci]        (row() as gather 0 above)
 * computed as split-K partial slabs [split][co][j][ci_pad] in `workspace` (plain coalesced stores),
 * then reduced in a fixed order (bitwise reproducible) into dW with element strides (so, si, sj):
 * Conv1d weight [Cout,Cin,k]: (Cin*k, k, 1); Linear weight [out,in]: (in, 1, 0).
 * co_split2 un-permutes the SPLIT2 output-channel packing.  accumulate != 0 adds to dW / db.
 * No atomics anywhere: results are bitwise reproducible run to run.
 * Replaces: autograd's convolution_backward / addmm weight gradients under loss.backward()
 * (trainer.py:330).
 */
typedef struct {
  int32_t dtype;
  const void* dY; int64_t ldy; int32_t y_cols;     /* y_cols: readable columns of dY rows (<= ldy) */
  const void* X; int64_t ldx; int64_t x_batch_stride; int32_t x_cols;
  int32_t B, T_in, T_out;
  int32_t taps, stride, pad_left, pad_mode;
  int32_t Cout, Cin;
  float* dW; int64_t so, si, sj;
  float* db;                       /* optional bias gradient [Cout]: db[co] (+)= sum_m dY[m, co], same slab/reduce path */
  int32_t co_split2; int32_t accumulate;
  int32_t splits;                  /* 0 = choose */
  void* workspace; size_t workspace_bytes;
  int32_t w_in, w_out, taps_h;     /* 2-D convolution: as in ZsGemmConv (dW[co, ci, j], j = kw*taps_h + kh); 0 = 1-D */
} ZsGemmWgrad;
size_t zs_gemm_wgrad_workspace_bytes(const ZsGemmWgrad* p);
int zs_gemm_wgrad(const ZsGemmWgrad* p, void* stream);
/* zs_gemm_wgrad_path: the kernels a zs_gemm_wgrad launch of *p would take now, under the current knobs -- the same plan function
 * the launch calls (argument checks, K-loop kernel, split-K plan, slab reduce).  Returns kernel | reduce << 8, or the negative code
 * zs_gemm_wgrad would return for these arguments (the workspace SIZE is checked by the launch only: ask
 * zs_gemm_wgrad_workspace_bytes); *splits and *rows_per_split (each may be null) receive the split-K plan: split k sums output rows
 * [k * rows_per_split, min(M, (k + 1) * rows_per_split)), M = B*T_out, an empty range gives a slab of zeros.  It reads the struct
 * and the knobs only: dY, X, dW, workspace are tested for null and alignment, never dereferenced, and no GPU call is made.
 *   P8:   gemm_wgrad_p8_kernel, 256x256 tiles, bf16: "wgrad_p8" 2; or "wgrad_p8" 1, padded / real output area of the 256-wide
 *         tiles at most "wgrad_p8_waste" / 100, M >= 2048 and (256x256 tiles x taps) * M >= 131072;  rows_per_split % 64 == 0
 *   DMA:  gemm_wgrad_dma_kernel, 128x128 tiles, bf16: every other bf16 launch with "wgrad_dma";  rows_per_split % 32 == 0
 *   REG:  gemm_wgrad_kernel, 128x128 tiles: fp32 always, bf16 with "wgrad_dma" 0;  rows_per_split % 32 == 0
 * splits: p->splits when > 0, else the plan's choice (under "wgrad_alone", "wgrad_wgs", "wgrad_wgs128*", "wgrad_slab_cost*").
 * reduce (bit 8): 1 = wgrad_reduce_taps_kernel (stores in dW order): "wgrad_reduce_taps", 1 < taps <= 256, si == taps and
 * sj == 1 (a Conv1d weight; so may exceed Cin*taps); 0 = wgrad_reduce_kernel (any so / si / sj).
 * Columns [Cout, y_cols) of dY and [Cin, x_cols) of X are read by the K-loop kernels and may hold anything (a neighbouring
 * problem's data, NaN): they reach only slab rows / columns from which neither reduce stores anything. */
enum { ZS_WGRAD_PATH_P8 = 0, ZS_WGRAD_PATH_DMA = 1, ZS_WGRAD_PATH_REG = 2 };
int zs_gemm_wgrad_path(const ZsGemmWgrad* p, int32_t* splits, int32_t* rows_per_split);

/* ---------------------------------------------------------------------------------------------
 * zs_pack_weight: fp32 parameter (PyTorch layout, strides so/si/sj as above) -> GEMM operand.
 * Writes the n_rows x n_cols block of dst that starts at (row_offset, col_offset), dst pitch ldw:
 *   transpose 0 (forward):  block[n][j*inner_pad + ci] = W[co(n)][ci][j]
 *   transpose 1 (dgrad):    block[ci][j*inner_pad + n] = W[co(n)][ci][j]
 * co(n) = n, or with co_split2: n < Cout/2 ? 2n : 2(n - Cout/2) + 1.  Everything else in the block is
 * zero (rows >= Cout|Cin, inner index >= Cin|Cout, taps >= taps).
 */
typedef struct {
  int32_t dtype;
  const float* W; int64_t so, si, sj;
  int32_t Cout, Cin, taps;
  int32_t transpose, co_split2;
  int32_t inner_pad;               /* cin_pad (transpose 0) or cout_pad (transpose 1) */
  void* dst; int64_t ldw;
  int32_t n_rows, n_cols, row_offset, col_offset;
  const int32_t* row_perm;         /* optional: output row n reads parameter row row_perm[n] (overrides co_split2) */
} ZsPackWeight;
int zs_pack_weight(const ZsPackWeight* p, void* stream);
/* the same for n jobs (one dtype) in ceil(n/32) launches: the per-step repack of a whole net after the optimiser step.
 * max_blocks > 0 caps the grid (the workgroups then walk the tile list): a re-pack that runs on a side stream beside a chain of
 * small kernels must leave them wave slots (about two workgroups per CU still stream at the HBM rate); 0 = one workgroup per tile */
int zs_pack_weight_batch(const ZsPackWeight* jobs, int32_t n, int32_t max_blocks, void* stream);

/* zs_copy_vec_batch: n small fp32 vector copies in ONE launch, dst[i*dst_stride] = src[i*src_stride] for i < len: the bias
 * re-ordering that goes with the pixel-shuffle packing (co_split2) and the stacked nn.GRU biases, issued with the re-pack. */
typedef struct {
  const float* src; float* dst;
  int32_t len, src_stride, dst_stride;
} ZsVecCopy;
int zs_copy_vec_batch(const ZsVecCopy* jobs, int32_t n, void* stream);

/* zs_cast_rows: dst[r][col_off + c] = f(src[r][c]) for c < cols, zeros for cols <= c < fill_cols.
 * f = identity or leaky_relu (model/model.py:446).  src fp32 or T (src_f32), dst T or fp32. */
typedef struct {
  int32_t dtype;
  const void* src; int64_t ld_src; int32_t src_f32;
  void* dst; int64_t ld_dst; int32_t dst_f32; int32_t col_off;
  int64_t rows; int32_t cols, fill_cols;
  int32_t act; float slope;
  /* optional second destination from the same read (type T): dst2[r][col_off2 + c] = f2(src[r][c]), zeros up to fill_cols2
   * (the encoder's input goes to the conv bank raw and to the concatenation through leaky_relu, model/model.py:441-446) */
  void* dst2; int64_t ld_dst2; int32_t col_off2, fill_cols2; int32_t act2; float slope2;
} ZsCastRows;
int zs_cast_rows(const ZsCastRows* p, void* stream);

/* zs_add_rowvec: out[b,t,c] = x[b,t,c] + vec[idx[b]][c]  (x + emb.view(B,C,1), model/model.py:319,336,353)
 * x may be null: broadcast (append_emb, model/model.py:81-85). */
typedef struct {
  int32_t dtype;
  const void* x; int64_t ldx;
  const float* vec; int64_t vec_ld; const int64_t* idx;
  void* out; int64_t ldo; int32_t B, T, C, fill_cols;   /* C: valid columns of vec; fill_cols: columns written */
} ZsAddRowvec;
int zs_add_rowvec(const ZsAddRowvec* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * zs_instnorm_fwd: nn.InstanceNorm1d (no affine, biased var, eps) over T for every (b, c), fused with
 * nn.Dropout and the block residual (model/model.py:416-438, 317-342):
 *   out = dropout(xhat) + residual ;  out2 = out + vec2[idx[b]]   (optional)
 * Dropout keep-mask: `mask` (uint8 [B,T,mask_ld]) if given, else counter-hash RNG(seed, stream_id)
 * that zs_instnorm_bwd regenerates.  T <= 256.
 */
typedef struct {
  int32_t dtype;
  const void* x; int64_t ldx;
  void* out; int64_t ldo;
  void* out2; int64_t ldo2; const float* vec2; int64_t vec2_ld; int32_t vec2_cols; const int64_t* idx;
  float* mean; float* rstd;       /* [B][C] fp32, saved for backward (may be null) */
  int32_t B, T, C; float eps;
  float drop_p; uint64_t seed; uint32_t stream_id; const uint8_t* mask; int64_t mask_ld;
  int32_t res_mode; const void* res; int64_t ldres; int32_t T_res; int32_t res_pad_mode;
  const uint64_t* seed_ptr;      /* optional device scalar added to `seed` (graph replay: see zs_step_counters) */
  /* ragged batch: the statistics of sample b run over its first lengths[b] <= T rows (T stays the row stride); rows past the
   * length are written as zeros.  res_lengths[b] <= T_res: valid rows of the ZS_RES_AVGPOOL2 residual (its odd-length
   * reflect / zero pad, model/model.py:424, happens at the sample's own end).  null = T / T_res for every sample. */
  const int32_t* lengths; const int32_t* res_lengths;
  /* 1: mean / rstd are INPUTS (statistics computed elsewhere, e.g. by the producing kernel): the two reductions over T are skipped */
  int32_t stats_given;
} ZsInstNormFwd;
int zs_instnorm_fwd(const ZsInstNormFwd* p, void* stream);

/* zs_instnorm_bwd: gradient w.r.t. the PRE-activation of the leaky_relu that feeds the norm:
 *   g = dout * keep/(1-p);  dx = rstd*(g - mean_t(g) - xhat*mean_t(g*xhat));  dz = dx * lrelu'(x). */
typedef struct {
  int32_t dtype;
  const void* dout; int64_t ldd;
  const void* x; int64_t ldx;
  const float* mean; const float* rstd;
  void* dz; int64_t ldz;
  int32_t B, T, C;
  float drop_p; uint64_t seed; uint32_t stream_id; const uint8_t* mask; int64_t mask_ld;
  float slope;
  const uint64_t* seed_ptr;
} ZsInstNormBwd;
int zs_instnorm_bwd(const ZsInstNormBwd* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * zs_grad_combine: everything autograd does between two GEMMs on the backward path:
 *   v[b,t,c]  = fold(gp)[b,t,c]                 gp = zs_gemm_conv(gather=1) output over the padded
 *                                                length T+pad_left+pad_right; reflect pads fold back
 *   emb_sum[b][c] += sum_t v[b,t,c]              (optional; per-sample part of nn.Embedding backward,
 *                                                 finished by zs_emb_scatter -- no atomics)
 *   v += residual term of `res` (IDENTITY: res[t]; AVGPOOL2: 0.5*res[t/2]; UPSAMPLE2: res[2t]+res[2t+1])
 *   v *= lrelu'(dact_src)                         (optional)
 *   store: rows, or un-pixel-shuffle (unshuffle=1): (b,t,c) -> row (b, t/2), col (t&1)*C + c
 */
typedef struct {
  int32_t dtype;
  const void* gp; int64_t ldg; int32_t pad_left, pad_right, pad_mode;
  int32_t B, T, C;
  float* emb_sum; int64_t emb_ld; int32_t emb_cols;
  int32_t res_mode; const void* res; int64_t ldres;
  const void* dact_src; int64_t dact_ld; float slope;
  void* out; int64_t ldo; int32_t unshuffle;
} ZsGradCombine;
int zs_grad_combine(const ZsGradCombine* p, void* stream);
/* zs_norm_decomposition: 1 if zs_instnorm_fwd (kernel 0), zs_instnorm_bwd (1) or zs_grad_combine (2) launched now with this dtype,
 * T and C would run the 8 x 256 decomposition, 0 for 32 x 64 (the same test the launch makes, under the current knobs). */
int zs_norm_decomposition(int32_t kernel, int32_t dtype, int32_t T, int32_t C);

/* zs_emb_scatter: nn.Embedding weight gradient from per-sample sums, in fixed sample order:
 *   demb[r][c] (+)= sum_{b : idx[b] == r} emb_sum[b][c]      (model/model.py:310-314 lookups) */
typedef struct {
  const float* emb_sum; int64_t emb_ld; const int64_t* idx; int32_t B;
  float* demb; int64_t demb_ld; int32_t n_rows, C; int32_t accumulate;
} ZsEmbScatter;
int zs_emb_scatter(const ZsEmbScatter* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * zs_mbv_fwd / zs_mbv_bwd: Multilabel-Binary-Vector discretiser (model/model.py:93-110, 474-480).
 * logits rows [B*T'][ld] hold E (l0,l1) pairs.  noise_kind 0: Gumbel noise G given (bit-exact
 * contract); 1: uniform U given, g = -log(-log(U+1e-20)+1e-20) on device; 2: U from the
 * counter-hash RNG(seed).  bits = ((hard - y0) + y0) with y = softmax((l+g)/tau), ties -> 1.0
 * (index 0).  y0 is saved for backward: dl0 = dbits*y0*(1-y0)/tau, dl1 = -dl0.
 */
typedef struct {
  int32_t dtype;
  const void* logits; int64_t ld; int32_t logits_f32;
  const float* noise; int32_t noise_kind; uint64_t seed;
  int64_t rows; int32_t E; float tau;
  void* bits; int64_t ld_bits; int32_t bits_fill_cols;
  float* bits_f32;               /* optional compact [rows][E] fp32 copy (API output) */
  float* y0;                     /* optional [rows][E] */
  const uint64_t* seed_ptr;      /* optional device scalar added to `seed` */
} ZsMbvFwd;
int zs_mbv_fwd(const ZsMbvFwd* p, void* stream);
typedef struct {
  int32_t dtype;
  const void* dbits; int64_t ld_dbits;
  const float* y0; int64_t rows; int32_t E; float tau;
  void* dlogits; int64_t ld; int32_t fill_cols;
} ZsMbvBwd;
int zs_mbv_bwd(const ZsMbvBwd* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * zs_gumbel_st_fwd / zs_gumbel_st_bwd: the other encoder discretisers (model/model.py:93-110, 457-472).
 * logits rows [B*T'][ld] hold n_lin columns: n_lin = E (ONE_HOT, CONTINUES) or E*E (BINARY).
 *  ONE_HOT:   one softmax group of E: enc = (hard - y) + y, y = softmax((l+g)/tau), hard = one-hot of
 *             argmax(y) (first index on ties).  dl_j = y_j (d_j - sum_k d_k y_k) / tau.
 *  BINARY:    E groups i of E (column i*E + j), softmax over j; s_j = sum_i out_{i,j} (fp32, increasing i),
 *             enc_j = clamp(s_j, 0, 1).  d_{i,j} = denc_j * [0 <= s_j <= 1], then the ONE_HOT formula per
 *             group.  Requires E <= 64.
 *  CONTINUES: enc = leaky_relu(l, slope), no noise.  dl = denc * (l > 0 ? 1 : slope).
 * Noise as in ZsMbvFwd (kind 0: Gumbel G, 1: uniform U, 2: counter-hash RNG(seed + *seed_ptr), its own
 * stream tag), laid out [rows][n_lin] (the reference's torch.rand shape).  Outputs: bits (compute dtype,
 * columns [E, bits_fill_cols) zeroed), optional compact fp32 bits_f32 [rows][E], y = the fp32 softmax
 * [rows][n_lin] (ONE_HOT / BINARY, for the backward), s = the unclamped sums [rows][E] (BINARY).
 * Backward: y / ld_y is the saved softmax (ONE_HOT / BINARY) or the fp32 logits (CONTINUES); writes
 * dlogits (compute dtype, ld) for columns [0, fill_cols), zeros past n_lin.
 */
enum { ZS_ENC_ONE_HOT = 0, ZS_ENC_BINARY = 1, ZS_ENC_CONTINUES = 2 };
typedef struct {
  int32_t dtype; int32_t mode;
  const void* logits; int64_t ld; int32_t logits_f32;
  const float* noise; int32_t noise_kind; uint64_t seed;
  int64_t rows; int32_t E; float tau; float slope;
  void* bits; int64_t ld_bits; int32_t bits_fill_cols;
  float* bits_f32;               /* optional compact [rows][E] fp32 copy (API output) */
  float* y;                      /* [rows][n_lin], ONE_HOT / BINARY (needed by the backward) */
  float* s;                      /* [rows][E], BINARY (needed by the backward) */
  const uint64_t* seed_ptr;      /* optional device scalar added to `seed` */
} ZsGumbelStFwd;
int zs_gumbel_st_fwd(const ZsGumbelStFwd* p, void* stream);
typedef struct {
  int32_t dtype; int32_t mode;
  const void* dbits; int64_t ld_dbits;
  const float* y; int64_t ld_y;
  const float* s;
  int64_t rows; int32_t E; float tau; float slope;
  void* dlogits; int64_t ld; int32_t fill_cols;
} ZsGumbelStBwd;
int zs_gumbel_st_bwd(const ZsGumbelStBwd* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * zs_gru_fwd / zs_gru_bwd: bidirectional single-layer nn.GRU with zero initial state
 * (model/model.py:59-66, 389, 299), gate order r,z,n.  gi = X W_ih^T + b_ih for BOTH directions
 * ([B*T][ldgi], columns dir*3H + {r,z,n}*H) comes from zs_gemm_conv.  Per time step the library
 * enqueues one grouped recurrent product (zs_gemm_conv kernel, 2 directions) and one gate kernel.
 * out[b,t, out_col + dir*H + j] = h_t.  gates saves r,z,n,(W_hn h + b_hn) for backward.
 * Persistent path (default when (H/32)*ceil(B/32)*2 <= #CUs and H is a multiple of 128 (bf16) / 64 (fp32), H <= 512 /
 * 256): ONE launch per pass, see gru_persist_fwd_kernel; needs the interleaved packing below.
 * Fast path (H % 32 == 0 and whh_interleaved): ONE launch per step -- a 16-rows-per-wave MFMA product whose
 * fragments come straight from L2 (no LDS, no barrier) with the gate math fused in its epilogue.  It needs the
 * rows of whh packed gate-interleaved per 32 hidden units: row hc*96 + g*32 + u = W_hh[g*H + hc*32 + u].
 */
typedef struct {
  int32_t dtype;
  int32_t B, T, H;
  const void* gi; int64_t ldgi;
  const void* whh; int64_t ldw; int32_t n_pad; int64_t w_gstride;   /* packed fwd [2][n_pad][ldw], N=3H, K=H */
  const float* bhh; int64_t bhh_gstride;                           /* [2][3H] */
  void* out; int64_t ldo; int32_t out_col;
  void* gates; /* T dtype [B][T][2][4H] or null (inference) */
  float* work; size_t work_bytes;   /* >= zs_gru_work_bytes */
  int32_t whh_interleaved;
  uint32_t* status;              /* optional caller-owned device word, STICKY: a persistent pass whose bounded spin expires ORs
                                    bit 0 (forward) / bit 1 (BPTT) into it and goes on with invalid data; the library never
                                    clears it.  The caller reads it at its own host sync points (Trainer.train: every logged
                                    loss; convert/encode: the end of a batch) and raises. */
  /* optional broadcast riding on the recurrence's stores (append_emb, model/model.py:81-85,357: the third block of the
   * concatenation the GRU output goes into): out[b][t][bcast_col + c] = bcast_vec[bcast_idx[b]][c] for c < 2H and every t.
   * The persistent kernel is latency-bound and leaves HBM idle, so these 64 MB cost nothing there. */
  const float* bcast_vec; int64_t bcast_ld; const int64_t* bcast_idx; int32_t bcast_col;
  /* 1: direction 1 also steps through t = 0 .. T-1 (instead of T-1 .. 0).  Ragged batches: the caller reverses the rows of
   * every sample over ITS OWN length (zs_rows_reverse) in the direction-1 columns of gi before and of out after this call, so
   * both directions are forward recurrences whose first lengths[b] steps are exactly the sample's own sequence. */
  int32_t dir1_forward;
} ZsGruFwd;
size_t zs_gru_work_bytes(int32_t B, int32_t H);
int zs_gru_fwd(const ZsGruFwd* p, void* stream);
/* test / debug hook (synchronises the stream): ZS_OK unless the last persistent pass over `work` had a workgroup give up
 * waiting for its group -- bounded spins instead of a hang; the results of that pass are then invalid */
int zs_gru_check(const float* work, int32_t B, int32_t H, void* stream);

/* zs_rows_reverse: in-place reversal of the rows of every sample over its own length, restricted to a column block:
 *   x[b][t][col0 + c] <-> x[b][lengths[b] - 1 - t][col0 + c]   for t < lengths[b] / 2, c < cols   (rows b*T + t, pitch ld elements)
 * (nn.GRU's reverse direction on a ragged batch, see ZsGruFwd.dir1_forward).  cols * element size must be a multiple of 4. */
typedef struct {
  int32_t dtype;
  void* x; int64_t ld; int32_t col0, cols;
  int32_t B, T; const int32_t* lengths;
} ZsRowsReverse;
int zs_rows_reverse(const ZsRowsReverse* p, void* stream);
typedef struct {
  int32_t dtype;
  int32_t B, T, H;
  const void* dout; int64_t ldd; int32_t dout_col;   /* gradient w.r.t. out columns */
  const void* out; int64_t ldo; int32_t out_col;     /* forward outputs (h_t) */
  const void* gates;
  const void* whh_t; int64_t ldw; int32_t n_pad; int64_t w_gstride; /* packed transposed [2][n_pad][ldw], N=H, K=3H */
  void* dgi; int64_t ldgi;       /* [B*T][ldgi] cols dir*3H.. : grad w.r.t. gi (input projections) */
  void* dgh; int64_t ldgh;       /* same shape: grad w.r.t. (h W_hh^T + b_hh) */
  float* work; size_t work_bytes;
  uint32_t* status;              /* sticky status word, see ZsGruFwd */
} ZsGruBwd;
int zs_gru_bwd(const ZsGruBwd* p, void* stream);
/* zs_gru_path: the plan a zs_gru_fwd (pass 0) or zs_gru_bwd (pass 1) launch with these sizes would take now, under the current
 * knobs and the device's CU count -- the same function the launches call.  Returns path | per << 8: the path is ZS_GRU_PATH_*,
 * per is PER in {1, 2, 4} (forward) / PERB in {3, 6, 12} (BPTT) of the PERSIST kernels and 0 otherwise; negative on bad arguments.
 *   WIDE: one persistent launch, 16-row x 64-unit tiles (bf16, H in {128, 256, 512}, "gru_wide", 16-byte operand layout);
 *   PERSIST: one persistent launch, 32 x 32 (forward) / 16 x 64 (BPTT) tiles;  STEP_FUSED: one launch per step, product and gate
 *   math fused;  STEP_GEMM: a zs_gemm_conv product and a gate kernel per step (H % 32 != 0, or W_hh not interleaved).
 * Both persistent paths need T > 1, "gru_persist" and a grid of at most one workgroup per CU.  whh_interleaved is
 * ZsGruFwd.whh_interleaved (ignored by pass 1); wide_aligned is 1 when the launch's operands meet the WIDE kernels' 16-byte
 * layout: forward: out_col, ldo, ldgi (and bcast_col) multiples of 8 elements, out, gi, gates 16-byte aligned; BPTT: also
 * dout_col, ldd and ldgh multiples of 8, dout, out, gates, dgi, dgh 16-byte aligned (zs_gru_fwd / zs_gru_bwd test it themselves). */
enum { ZS_GRU_PATH_WIDE = 0, ZS_GRU_PATH_PERSIST = 1, ZS_GRU_PATH_STEP_FUSED = 2, ZS_GRU_PATH_STEP_GEMM = 3 };
int zs_gru_path(int32_t pass, int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t whh_interleaved, int32_t wide_aligned);
/* zs_gru_solo: 1 when that launch would run the one-workgroup variant of WIDE now, else 0; negative on bad arguments (the arguments
 * and the plan function of zs_gru_path, whose value the variant does not change).  H = 128 only: W_hh of one direction (96 KB in
 * bf16) fits the registers of ONE workgroup, which then owns all units of its 16 batch rows: h_{t-1} goes through LDS and nothing
 * is handed between CUs.  Such a launch issues no memset, neither reads nor writes `work` (zs_gru_check keeps reporting what was
 * there), cannot time out and never touches `status`; its results are bit-equal to the hand-off kernels'.  Needs WIDE, H <=
 * "gru_solo_max_h" and "gru_spin_limit" != 0. */
int zs_gru_solo(int32_t pass, int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t whh_interleaved, int32_t wide_aligned);

/* ---------------------------------------------------------------------------------------------
 * zs_l1_loss: loss = mean|x_dec - x| over rows*F (trainer.py:328) and the gradient w.r.t. the
 * pre-sigmoid logits: g = sign(x_dec - x)/(rows*F) * x_dec*(1-x_dec).
 * loss_out receives the scalar (two-pass, fixed order).  partial: >= 1024 floats.
 */
typedef struct {
  int32_t dtype;
  const float* x_dec; int64_t ld_dec;
  const float* x; int64_t ldx;
  int64_t rows; int32_t F;
  void* dlogits; int64_t ldg; int32_t fill_cols;   /* may be null (loss only) */
  float* partial; float* loss_out; float grad_scale;
} ZsL1Loss;
int zs_l1_loss(const ZsL1Loss* p, void* stream);

/* zs_sqnorm: out[0] = sum g[i]^2 (double accumulation, fixed order).  partial: >= 1024 doubles. */
int zs_sqnorm(const float* g, int64_t n, double* partial, float* out_sq, void* stream);

/* zs_adam_clip: nn.utils.clip_grad_norm_(max_norm) (utils.py:53-55) fused with torch.optim.Adam's
 * single-tensor update (trainer.py:66,332): coef = min(1, max_norm/(sqrt(sumsq)+1e-6)); g *= coef;
 * m = m + (g-m)(1-b1); v = v*b2 + g*g*(1-b2); p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps).
 * sumsq is a device scalar (from zs_sqnorm); max_norm <= 0 disables clipping.
 * grad_scale (0 = 1): g holds grad_scale^-1 times the gradient -- the SUM over `world` data-parallel ranks with
 * grad_scale = 1/world -- so the average is never materialised: norm = grad_scale*sqrt(sumsq), g_eff = g*grad_scale*coef.
 * ema (optional): the exponential moving average of the weights, updated in the same pass from the new p while it is in a
 * register: ema = fma(p_new - ema, 1 - ema_decay, ema), i.e. ema.lerp_(p, 1 - ema_decay) with p_new - ema rounded once and
 * 1 - ema_decay formed in fp32.  It changes no bit of p, g, m or v.  ema not 16-byte aligned: the one-element loop runs
 * (the same bits). */
typedef struct {
  float* p; float* g; float* m; float* v; int64_t n;
  float lr, beta1, beta2, eps, bc1, bc2;
  const float* sumsq; float max_norm; int32_t write_clipped_grad;
  const int32_t* step_ptr;       /* optional device step count t: bc1 = 1-beta1^t, bc2 = 1-beta2^t computed on device */
  float grad_scale;
  int32_t max_blocks;            /* > 0: grid cap (see zs_pack_weight_batch); 0 = default */
  float* ema;                    /* optional weight average, n floats indexed like p; null = off (a zeroed struct is off) */
  float ema_decay;               /* with ema: 0 <= ema_decay < 1, else ZS_EINVAL */
} ZsAdam;
int zs_adam_clip(const ZsAdam* p, void* stream);

/* zs_sqnorm_stage1: the first half of zs_sqnorm alone (per-workgroup double partials); returns how many partials it wrote
 * (1..1024), or a negative error code.  zs_adam_pack can finish the sum itself (sq_partial). */
int zs_sqnorm_stage1(const float* g, int64_t n, double* partial, void* stream);

/* zs_adam_pack: zs_adam_clip over a net's whole flat buffer AND the re-pack of its GEMM operands, in one launch over one
 * flat work list: every parameter is read once, updated, and its new value written to p and, rounded to the operand
 * type, to every packed view of it -- zs_adam_clip + zs_pack_weight_batch + zs_copy_vec_batch without the re-read.  Only
 * elements that come from a parameter are written to a view: the zero padding of an operand is written once by a full
 * zs_pack_weight and stays.  The update is the expression zs_adam_clip compiles (bit-identical results).
 * Jobs (sorted by `off`; together they must cover [0, a->n) exactly once -- the caller's plan checks that):
 *   ZS_APJ_WEIGHT: the parameter W[Cout][Cin][taps] at p + off, dense (element strides (Cin*taps, taps, 1), taps <= 7).
 *       A workgroup takes a block of 64 x 64 (taps 1) or 32 x 32|16 (bf16|fp32) x all taps (output rows x input channels)
 *       through LDS.  co_split2: tile row n is parameter row co(n) as in ZsPackWeight (n is the row / inner index every
 *       view is written at).  Views (n_views <= 2), for element (n, ci, j):
 *         transpose 0: dst[(row + row_offset) * ldw + col_offset + slot(j) * inner_pad + ci], row = row_inv ? row_inv[co] : n
 *         transpose 1: dst[(ci  + row_offset) * ldw + col_offset + slot(j) * inner_pad + n]
 *       slot(j) = j, or with `parity` the stride-2 data gradient's tap order: j even ? j/2 : (taps+1)/2 + j/2.
 *       row_inv (int32 [Cout], device) is the inverse of ZsPackWeight.row_perm.  dst_elems = elements of the operand type
 *       that may be written from dst on (checked on the host against the largest index of the view).
 *   ZS_APJ_VECTOR: Adam over [off, off + len) and up to two strided copies of the new values (re-ordered biases):
 *       view c: dst (fp32) [i * ldw] = p[off + src_offset + i * src_stride] for i < vlen.
 *   ZS_APJ_RANGE: plain Adam over [off, off + len), the code of zs_adam_clip.
 * tile_start: the prefix sum of zs_adam_pack_tiles() over the jobs before this one (the caller fills it; checked).
 * `jobs` is the list in host memory (checked on every call), `jobs_dev` the same bytes in device memory (read by the
 * kernel: the list is too long for launch arguments); both stay alive and unchanged while launches may run or replay.
 * sq_partial / n_partial: the partials of zs_sqnorm_stage1; every workgroup then sums them in the order of zs_sqnorm's
 * second stage (the same float) and workgroup 0 stores it to a->sumsq; null: a->sumsq is read as zs_adam_clip reads it.
 * a->max_blocks caps the grid as in zs_adam_clip.  dtype (ZS_F32 / ZS_BF16, of every view) is one for all jobs.
 * a->ema / a->ema_decay: the weight average of zs_adam_clip, by the same device function in every kind of tile (bit-identical
 * to zs_adam_clip's); no launch is added.  The packed views always hold the raw new p, never the average. */
enum { ZS_APJ_WEIGHT = 0, ZS_APJ_VECTOR = 1, ZS_APJ_RANGE = 2 };
typedef struct {
  void* dst; int64_t ldw; int64_t dst_elems;
  int32_t transpose, inner_pad, row_offset, col_offset, parity;
  int32_t vlen, src_offset, src_stride;
  const int32_t* row_inv;
} ZsAdamPackView;
typedef struct {
  int32_t kind, dtype;
  int64_t off, len;
  int32_t Cout, Cin, taps, co_split2;
  int32_t n_views, tile_start;
  ZsAdamPackView view[2];
} ZsAdamPackJob;
int zs_adam_pack_tiles(const ZsAdamPackJob* job);
int zs_adam_pack(const ZsAdam* a, const ZsAdamPackJob* jobs, const ZsAdamPackJob* jobs_dev, int32_t n, const double* sq_partial,
                 int32_t n_partial, void* stream);

/* zs_host_fetch: dst[0..bytes) = src[0..bytes) by a KERNEL that reads pinned (device-accessible) host memory over PCIe with
 * 16-byte loads, on a deliberately small grid (`workgroups`, 0 = 32; 8 loads in flight per lane cover the link's
 * bandwidth-latency product).  It replaces the H2D memcpy of the next batch (trainer.py:238-244) inside the captured step: on
 * this stack a memcpy node of a hipGraph is not overlapped with the graph's kernel nodes, a kernel node on a forked stream is.
 * bytes must be a multiple of 16, both pointers 16-byte aligned. */
int zs_host_fetch(const void* src, void* dst, size_t bytes, int32_t workgroups, void* stream);

/* zs_pool_gather: one training batch out of a dataset that lies in device memory (the reference builds it on the host,
 * dataloader.py:34-52, and copies it over, trainer.py:238-244).  pool fp32 [frames_total][F], utterances back to back; the item table
 * of n entries: speaker int32 [n], first int64 [n] = first frame of the item's segment in the pool.  With k = *cursor, S = world * B
 * and P = max(1, ceil(n / S) - 1), batch k serves the items
 *   item(b) = ((k mod P) * S + rank * B + b) mod n,   b < B       (dataloader.py:48-51's sliding index and wrap rule in closed form;
 *                                                                  the mod n only ever acts when world > 1)
 *   x[b][t][f] = pool[first[item(b)] + t][f]   t < seg_len, f < F      x fp32 [B][seg_len][F] contiguous
 *   c[b]       = speaker[item(b)]                                      c int64 [B]
 * advance != 0: a one-thread launch behind the gather then does *cursor += 1, so a captured launch with frozen arguments serves
 * the next batch at every replay.  The cursor is an int64 in device memory that the host may set (>= 0) between launches.
 * n >= world * B is required.  The kernel trusts the table: the caller checks 0 <= first and first + seg_len <= frames_total
 * for every entry on the host before it uploads it.  pool and x need 4-byte alignment only.  No allocation, no synchronisation. */
typedef struct {
  const float* pool; const int32_t* speaker; const int64_t* first;
  int64_t* cursor;
  int64_t n; int32_t B, seg_len, F, rank, world;
  float* x; int64_t* c;
  int32_t advance;
} ZsPoolGather;
int zs_pool_gather(const ZsPoolGather* p, void* stream);

/* zs_step_counters: per-step device-side state for hipGraph replay (kernel arguments are frozen in a graph):
 * *seed += 0x9E3779B97F4A7C15, *step += 1.  Either pointer may be null. */
int zs_step_counters(uint64_t* seed, int32_t* step, void* stream);

/* zs_softmax_ce: nn.CrossEntropyLoss (mean) + gradient (trainer.py:297-304). logits fp32 [B][ld]. */
typedef struct {
  const float* logits; int64_t ld; const int64_t* target; int32_t B, n_class;
  float* loss_out; float* dlogits; int64_t ldg; float grad_scale; int32_t* correct_out;
} ZsSoftmaxCE;
int zs_softmax_ce(const ZsSoftmaxCE* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Vocoder (convert.py:39-62): batched Griffin-Lim on 1024-point real FFTs held in LDS.
 * mag: fp32 [n_utt][T_max][513] linear magnitudes (zero rows past each utterance's length).
 * zs_gl_istft: frames of spec (complex64 [n_utt][T_max][513]) -> windowed irfft -> overlap-add /
 *              window-sum-square -> wav [n_utt][wav_ld] (200*(T-1) samples, centre-trimmed).
 * zs_gl_stft_project: wav -> reflect-padded frames -> rfft -> spec = mag * E/max(1e-8,|E|).
 * Utterances with lengths[u] < 4 frames are skipped by zs_gl_istft, zs_gl_stft_project and zs_gl_iter alike: nothing of their
 * rows is read or written (the reflect padding of 512 samples needs 200*(T-1) > 512).
 */
typedef struct {
  const float* spec; const float* mag; const int32_t* lengths; int32_t n_utt, T_max;
  float* wav; int64_t wav_ld; float* frames_ws;    /* frames_ws: [n_utt][T_max][1024] fp32 scratch */
} ZsGlIstft;
int zs_gl_istft(const ZsGlIstft* p, void* stream);
typedef struct {
  const float* wav; int64_t wav_ld; const float* mag; const int32_t* lengths; int32_t n_utt, T_max;
  float* spec;
} ZsGlStft;
int zs_gl_stft_project(const ZsGlStft* p, void* stream);
/* zs_gl_iter: ONE Griffin-Lim iteration (convert.py:46-50) as one fused kernel per utterance tile:
 *     x = istft(spec_in);  E = stft(x);  spec_out = mag * E / max(1e-8, |E|)
 * (the windowed frames and the waveform never leave LDS; 512-point complex FFT per wave for the real 1024-point transforms).
 * spec_out == NULL: the final pass -- only x = istft(spec_in), written to wav [n_utt][wav_ld] (200*(T-1) samples each).
 * spec_in / spec_out: complex64 [n_utt][T_max][513], distinct buffers (neighbouring tiles read spec_in while spec_out is
 * written).  Utterances need lengths[u] >= 4 frames (the reflect padding of 512 samples must fit; shorter ones are skipped:
 * the reference's decoder never emits fewer than 16).
 * zs_griffin_lim: the whole loop of convert.py:39-52 from one call: spec_a holds X0 = S (zero phase) on entry; n_iter
 * iterations ping-pong spec_a / spec_b; then the final inverse pass into wav. */
typedef struct {
  const float* spec_in; float* spec_out;
  const float* mag; const int32_t* lengths; int32_t n_utt, T_max;
  float* wav; int64_t wav_ld;
  int32_t tile_frames;           /* STFT frames per workgroup tile (4..42), 0 = default 10 */
  const int32_t* host_lengths;   /* optional copy of `lengths` in HOST memory: zs_griffin_lim then cuts its launch chains at equal frame
                                    counts instead of equal utterance counts (utterances stay in order) */
  float momentum;                /* FGLA alpha in [0, 1); 0 = the plain loop (spec_prev ignored) */
  float* spec_prev;              /* complex64 [n_utt][T_max][513]: E of the previous iteration at each frame */
} ZsGlIter;
int zs_gl_iter(const ZsGlIter* p, void* stream);
int zs_griffin_lim(const ZsGlIter* p, float* spec_a, float* spec_b, int32_t n_iter, void* stream);
/* spec_a / spec_b are SCRATCH for zs_griffin_lim ([n_utt][T_max][513] complex64 each, contents on entry ignored): the loop starts
 * from X0 = S with zero phase (convert.py:41), which the first iteration reads from `mag` itself. */
/* zs_griffin_lim issues the loop as up to `gl_chains` (zs_set_option, default 3) independent launch chains over contiguous utterance
 * ranges, on internal streams measured (once per process) to execute side by side, joined back into `stream` before it returns:
 * utterances do not depend on each other, and a chain's partly filled last round of workgroups is filled by the others.  One chain
 * for small batches (< 8192 frames per chain) and under stream capture.  zs_gl_chains_used: chains of the last call (reporting). */
int zs_gl_chains_used(void);
/* Fast Griffin-Lim (Perraudin et al. 2013; librosa / torchaudio `momentum`): with momentum = alpha > 0 an iteration projects
 *     A_n = E_n - beta E_{n-1},  beta = alpha / (1 + alpha)       X_n = mag * A_n / max(1e-8, |A_n|)
 * instead of E_n (A_1 = E_1).  alpha = 0 is the plain loop above, bit for bit.  spec_prev holds E of the previous iteration at
 * every frame; each iteration reads and rewrites it at the utterances' frames (rows past lengths[u] are never touched):
 *   zs_griffin_lim: spec_prev is SCRATCH like spec_a / spec_b (contents on entry ignored: the first iteration initialises it);
 *                   the chains use it at the same utterance offsets as spec_a / spec_b.
 *   zs_gl_iter:     spec_prev is read and written; a zero-filled buffer means "first iteration" (A = E - beta 0 = E exactly), so a
 *                   caller that drives the loop itself gets FGLA by zero-filling it once.  The final pass (spec_out == NULL)
 *                   neither reads nor writes it.
 * Errors (nothing is launched): momentum not finite or outside [0, 1); momentum > 0 with spec_prev == NULL or with spec_prev
 * overlapping spec_in / spec_out (zs_gl_iter) or spec_a / spec_b (zs_griffin_lim). */
/* spectrogram2wav pre/post (convert.py:56-60): de-normalise to amplitude; de-preemphasis IIR. */
/* ---------------------------------------------------------------------------------------------
 * Feature extraction feeding the path (preprocess.py:227-258 get_spectrograms after the host-side
 * librosa.effects.trim): wav [n_utt][wav_ld] fp32, n_samples[u] valid samples ->
 *   mag[u][t][0..513) = clip((20 log10(max(1e-5, |STFT(preemph(y))|)) - ref_db + max_db) / max_db, 1e-8, 1), t < 1 + n_samples/200
 *   amp (optional, [n_utt][T_max][513]): the linear magnitudes, input of zs_pre_mel.
 * STFT as in the vocoder: n_fft 1024, hop 200, hann(800) centred, reflect-padded centre frames.  The padding is numpy's
 * mode='reflect' for ANY window length n >= 2, the triangle wave zs_trim documents below (P = 2 (n - 1), m = j mod P taken
 * non-negative, refl(j) = m if m < n else P - m): a window shorter than the padding of 512 folds back and forth as numpy's does.
 * Rows with n_samples[u] < 2 and frames t >= 1 + n_samples[u]/200 are not written.
 */
typedef struct {
  const float* wav; int64_t wav_ld; const int32_t* n_samples; int32_t n_utt, T_max;
  float preemph, ref_db, max_db;
  float* mag; int64_t mag_ld;      /* [n_utt][T_max][mag_ld], mag_ld >= 513 */
  float* amp;
  const int32_t* start;            /* optional [n_utt], device (appended; NULL = 0 for every row): utterance u is the window
                                      wav[u][start[u] .. start[u] + n_samples[u]) */
} ZsPreSpec;
int zs_pre_spectrogram(const ZsPreSpec* p, void* stream);
/* ZsPreSpec.start: the window is the utterance, exactly as a host-sliced copy of it would be: the reflect padding and the
 * pre-emphasis predecessor stay inside it (frame 0 / sample 0 uses w[0] of the window) and nothing outside it is read, so the
 * bounds zs_trim leaves on the device are applied in place.  start[u] is clamped to [0, wav_ld] and the window to the row. */
/* zs_trim: librosa.effects.trim (preprocess.py:238) for a ragged batch on the device; the definition is zs_amd.convert.trim().
 * wav fp32 [n_utt][wav_ld], n = n_samples[u] (device, clamped to wav_ld) -> bounds int32 [n_utt][2] = (start, stop) on the device:
 *   frames      f = 0 .. n / hop                                               (1 + n / hop of them, centred)
 *   mse[f]      = mean_{i < frame_length} y[refl(f * hop + i - frame_length / 2)]^2, accumulated in double
 *   refl        numpy's mode='reflect' for ANY pad width, a triangle wave: P = 2 (n - 1), m = j mod P taken non-negative,
 *               refl(j) = m if m < n else P - m; n == 1 maps every j to 0 (so n <= frame_length / 2 is covered, which
 *               zs_gl_frame_mse does not)
 *   kept        10 log10(max(1e-10, mse[f])) - 10 log10(max(1e-10, max_f mse[f])) > -top_db   (both floors: an all-zero or very
 *               quiet row keeps every frame and gives (0, n))
 *   bounds      start = first_kept * hop, stop = min(n, (last_kept + 1) * hop); (0, 0) when no frame is kept
 *   n <= 0      (0, 0), nothing of the row is read.  Samples at or past n_samples[u] are never read (the slack may hold anything).
 * Two launches: one wave per (utterance, block of hop samples) writes the block's sum of squares into `work` (every sample read
 * once; 16-byte loads where the address allows), then one workgroup per utterance forms the frame means from frame_length / hop
 * consecutive block sums, their maximum and the bounds.  Every sum has a fixed order that depends on the row alone: a launch is
 * bitwise reproducible and a row's bounds do not depend on the rows around it, on wav_ld or on the load width.  No atomics.
 * work: caller-owned, 8-byte aligned, zs_trim_workspace_bytes(n_utt, wav_ld, frame_length, hop) bytes (n_utt * (wav_ld / hop +
 * frame_length / hop) doubles; 0 for arguments zs_trim would refuse); contents on entry ignored.  No allocation, stream-ordered.
 * Errors (nothing is launched): a null pointer with n_utt > 0; n_utt < 0 or > 65535; hop <= 0; frame_length odd or not a positive
 * multiple of hop; wav_ld outside (0, 2^31); top_db not > 0; work_bytes too small.  n_utt == 0 succeeds and launches nothing. */
typedef struct {
  const float* wav; int64_t wav_ld;      /* [n_utt][wav_ld] */
  const int32_t* n_samples;              /* [n_utt], device */
  int32_t n_utt, frame_length, hop;
  float top_db;
  int32_t* bounds;                       /* [n_utt][2], device */
  double* work; size_t work_bytes;
} ZsTrim;
size_t zs_trim_workspace_bytes(int32_t n_utt, int64_t wav_ld, int32_t frame_length, int32_t hop);
int zs_trim(const ZsTrim* p, void* stream);
/* mel[r][m] = clip((20 log10(max(1e-5, sum_k basis[m][k] amp[r][k])) - ref_db + max_db) / max_db, 1e-8, 1); basis [n_mels][513]
 * (librosa.filters.mel(sr, n_fft, n_mels), preprocess.py:243-252) */
int zs_pre_mel(const float* amp, const float* basis, float* mel, int64_t rows, int32_t n_mels, float ref_db, float max_db, void* stream);
int zs_gl_denormalize(const float* mag_norm, float* mag_amp, int64_t n, void* stream);
/* zs_gen_scatter: the stage-2 converted spectrogram of one inference chunk, straight into the vocoder's padded amplitude input
 * (trainer.py:206-213 combine, then convert.py:56-58 when denorm is set).  xd, m: fp32 rows [rows][ld_xd] / [rows][ld_m], e.g. the
 * decoder's and the generator's outputs of a chunk (r = b*T + t), read in place:
 *   amp[dst[r]][f] = denorm(combine(xd[r][f], m[r][f]))     f < 513, for every r with 0 <= dst[r] < amp_rows (dst < 0: skip)
 *   combine: mode 0  xd;  mode 1  xd + m;  mode 2  xd + xd*m, the product rounded before the add (no FMA contraction, as torch)
 *   denorm:  the expression of zs_gl_denormalize (one shared device function: the same bits for the same input) or, if 0, none.
 * ld_xd == 0 reads the same row for every r (mode 0 over a zero row: the padding rows of the vocoder input).  m may be null in
 * mode 0.  One wave per row, no allocation, no synchronisation. */
typedef struct {
  const float* xd; int64_t ld_xd;
  const float* m; int64_t ld_m;
  const int32_t* dst; int64_t rows;
  float* amp; int64_t amp_ld, amp_rows;
  int32_t mode, denorm;
} ZsGenScatter;
int zs_gen_scatter(const ZsGenScatter* p, void* stream);
/* zs_frag_gather: the fragments --test_classify sends through the TargetClassifier (convert.py:379-397), out of a batch of
 * spectrograms, in one launch.  src fp32 [n_utt][T_max][513] (utterance u at src + u * utt_stride, rows of 513 floats: only
 * 4-byte alignment), table int32 [n_frag][2] = (utt, start):
 *   dst[f][t][k] = src[utt_f][start_f + t][k]      t < seg_len, k < 513;   dst fp32 [n_frag][seg_len][513], contiguous
 * An entry outside 0 <= utt < n_utt, 0 <= start <= T_max - seg_len writes a zero fragment and reads nothing (the caller plans the
 * table on the host and checks it there).  No allocation, no synchronisation. */
typedef struct {
  const float* src; int64_t utt_stride; int32_t n_utt, T_max;
  const int32_t* table; int32_t n_frag, seg_len;
  float* dst;
} ZsFragGather;
int zs_frag_gather(const ZsFragGather* p, void* stream);
/* Bit-packed units.  A unit is one encoded frame of E columns of 0 / 1 (what write_encodings stores as a line of text); packed, it is
 * a row of row_bytes >= (E + 7) / 8 bytes: bit j of byte k is column 8k + j (numpy.packbits(bitorder='little') along the columns),
 * the unused high bits of the last byte zero.  `packed` is one device buffer [n_units][row_bytes] holding every utterance of a batch;
 * start (int64 [n_frag], a row of `packed`) and len (int32 [n_frag]) are device tables planned on the host.  In both kernels one lane
 * produces each output byte / 16-byte piece whole: no read-modify-write, no atomics, a launch is bitwise reproducible and fragment f
 * touches its own rows only.  No allocation, no synchronisation.  n_frag == 0 succeeds and launches nothing; n_frag outside
 * [0, ZS_UNITS_MAX_FRAG] (the fragments of a launch are strided over at most 65535 grid rows), a null operand with work to do,
 * E <= 0, T <= 0, ld < E or row_bytes < (E + 7) / 8 launch nothing and return ZS_EINVAL.
 *
 * zs_units_unpack: packed units straight into the Decoder's input operand of one inference chunk (what permute + contiguous + float
 * + zs_cast_rows(fill_cols = ld_dst) build from fp32 [B, E, T'], model/model.py:346).  dst [n_frag][T][ld_dst] of `dtype`, 16-byte
 * aligned, ld_dst a multiple of 8, written with 16-byte stores:
 *   dst[f][t][c] = bit(packed[start[f] + t], c) ? 1 : 0      t < len[f], c < E
 *   dst[f][t][c] = 0                                         len[f] <= t < T, or E <= c < ld_dst
 * An entry with len < 0, len > T, start < 0 or start + len > n_units writes a zero fragment and reads nothing (as zs_frag_gather). */
#define ZS_UNITS_MAX_FRAG 1048576
typedef struct {
  int32_t dtype;
  const uint8_t* packed; int64_t n_units; int32_t row_bytes, E;
  const int64_t* start; const int32_t* len; int32_t n_frag, T;
  void* dst; int64_t ld_dst;
} ZsUnitsUnpack;
int zs_units_unpack(const ZsUnitsUnpack* p, void* stream);
/* zs_units_pack: the inverse, for the encoder's output rows.  src [n_frag][T][ld_src], read in place: fp32 when src_f32, else `dtype`
 * (the engine's own `bits` buffer); 16-byte loads when src is 16-byte aligned and ld_src a multiple of 8 (4 for fp32).
 *   packed[start[f] + t] = the bits (src[f][t][c] != 0), c < E; every byte of the row's row_bytes is written      t < len[f]
 * Rows t >= len[f] are not read and nothing is written for them (the MIN_LEN truncation of convert.py:148-149 is a shorter len).
 * An entry out of range (as above) reads and writes nothing. */
typedef struct {
  int32_t dtype, src_f32;
  const void* src; int64_t ld_src; int32_t n_frag, T, E;
  const int64_t* start; const int32_t* len;
  uint8_t* packed; int64_t n_units; int32_t row_bytes;
} ZsUnitsPack;
int zs_units_pack(const ZsUnitsPack* p, void* stream);
/* Voice adaptation (zs_amd/voice.py): the five embedding rows of a new speaker are fitted to a few utterances with every other weight
 * frozen.  The utterances' spectrograms lie in device memory as a pool (zs_pool_gather's layout) and their units, encoded once, as
 * bit-packed rows (zs_units_unpack's layout).
 *
 * zs_voice_gather: one adaptation batch per call, behind a device cursor -- zs_pool_gather and zs_units_unpack in one kernel, with the
 * item chosen on the device, so that a captured call serves the next batch at every replay (zs_units_unpack alone reads its `start`
 * table through launch arguments that a graph freezes).  pool fp32 [frames_total][F]; packed uint8 [n_units][row_bytes]; the item
 * table of n >= 1 entries, planned on the host: first int64 [n] = first frame of the segment in the pool (a multiple of 8 is what
 * the planner makes; the kernel does not need it) and ufirst int64 [n] = the row of `packed` that holds the unit of that frame.  With
 * k = *cursor:
 *   item(b)       = (k * B + b) mod n                                          b < B
 *   x[b][t][f]    = pool[first[item(b)] + t][f]                                t < seg_len, f < F; x fp32 [B][seg_len][F] contiguous
 *   bits[b][u][c] = bit(packed[ufirst[item(b)] + u], c) ? 1 : 0                u < seg_len / 8, c < E
 *   bits[b][u][c] = 0                                                          E <= c < ld_bits
 * bits [B][seg_len / 8][ld_bits] of `dtype` (ZS_F32 / ZS_BF16) is the Decoder's input operand: 16-byte aligned, ld_bits a multiple
 * of 8, written with 16-byte stores.  advance != 0: a one-thread launch behind the gather then does *cursor += 1.  One lane produces
 * each output piece whole: no atomics, no read-modify-write, a call is bitwise reproducible.  pool and x need 4-byte alignment only
 * (F = 513); first, ufirst and cursor 8-byte.  The kernel trusts the table: the caller checks 0 <= first, first + seg_len <=
 * frames_total, 0 <= ufirst and ufirst + seg_len / 8 <= n_units for every entry on the host before it uploads it.  A null operand,
 * B, F, E or n <= 0, seg_len <= 0 or no multiple of 8, ld_bits < E or no multiple of 8, row_bytes < (E + 7) / 8, a dtype other than
 * the two or a misaligned pointer return ZS_EINVAL and launch nothing.  No allocation, no synchronisation. */
typedef struct {
  int32_t dtype;
  const float* pool; const uint8_t* packed; int32_t row_bytes;
  const int64_t* first; const int64_t* ufirst; int64_t n;
  int64_t* cursor;
  int32_t B, seg_len, F, E;
  float* x; void* bits; int64_t ld_bits;
  int32_t advance;
} ZsVoiceGather;
int zs_voice_gather(const ZsVoiceGather* p, void* stream);
/* zs_voice_adam: the end of an adaptation step in one launch -- the five zs_emb_scatter (all samples to row 0), zs_sqnorm and
 * zs_adam_clip over the five rows.  emb_sum fp32 [5][B][C], contiguous: the decoder's per-sample embedding sums (slots 0..4 of
 * DecoderEngine's buffer).  With i = k * C + c over the 5 C elements:
 *   g[i]   = sum_b emb_sum[k][b][c], an fp32 sum in ascending b from 0.f (the order and the bits of zs_emb_scatter);  g fp32 [5][C]
 *   *sumsq = (float) sum_i (double) g[i]^2, in a fixed order
 *   row[k][c], m[i], v[i]: the update of zs_adam_clip (the same device function: bit-identical to zs_adam_clip over p = row k,
 *   g, m, v given this *sumsq), with max_norm <= 0 = no clipping and step_ptr (optional device step count t, else bc1 / bc2) as there.
 * row: five device pointers to C floats each (the rows need not be adjacent); m, v fp32 [5][C].  One workgroup: the work is
 * 5 B C floats read once (320 KB at B = 16, C = 1024).  No atomics, no host synchronisation, capturable.  A null operand, B or
 * C <= 0, 5 C > ZS_VOICE_ADAM_MAX, or bias corrections <= 0 without step_ptr return ZS_EINVAL and launch nothing. */
#define ZS_VOICE_ROWS 5
#define ZS_VOICE_ADAM_MAX 65536
typedef struct {
  const float* emb_sum; int32_t B, C;
  float* row[5]; float* m; float* v; float* g;
  float lr, beta1, beta2, eps, bc1, bc2;
  float* sumsq; float max_norm;
  const int32_t* step_ptr;
} ZsVoiceAdam;
int zs_voice_adam(const ZsVoiceAdam* p, void* stream);
/* zs_tclf_score: the scoring loop of target_classify (convert.py:400-413) on the device.  logits fp32 [n_frag][ld] (3 valid columns),
 * target int32 [n_frag] (0 V001, 1 V002, 2 'None', -1 any other speaker: never correct):
 *   pred[f] = argmax_j logits[f][j] (first maximum, NaN as the maximum: numpy's rule; pred may be null)
 *   *correct += #{f : pred[f] == target[f]},   *count += n_frag          (device int32 counters, added with atomics) */
typedef struct {
  const float* logits; int64_t ld;
  const int32_t* target; int32_t n_frag;
  int32_t* pred; int32_t* correct; int32_t* count;
} ZsTclfScore;
int zs_tclf_score(const ZsTclfScore* p, void* stream);
int zs_gl_deemphasis(float* wav, int64_t wav_ld, const int32_t* lengths, int32_t n_utt, float coef, void* stream);
/* zs_gl_frame_mse: the frame statistics of librosa.effects.trim (convert.py:61; librosa's rms on the centred, reflect-padded
 * signal): mse[u][f] = mean_{i < frame_length} y_u[reflect(f*hop + i - frame_length/2)]^2, f <= L_u / hop, L_u = 200 *
 * (lengths[u] - 1) samples of wav row u (needs L_u > frame_length / 2), accumulated in double.  The caller thresholds at
 * top_db below the maximum and slices: only these few hundred values per utterance are examined on the host. */
int zs_gl_frame_mse(const float* wav, int64_t wav_ld, const int32_t* lengths, int32_t n_utt, int32_t frame_length, int32_t hop,
                    double* mse, int64_t mse_ld, void* stream);
/* zs_resample: band-limited sample-rate conversion of a ragged batch, the resampling inside librosa.load(sound_file, sr=hp.sr)
 * (preprocess.py:227-258, convert.py:377,431; librosa <= 0.7: resampy 'kaiser_best', scale=False, then fix_length).  The filter is
 * the Kaiser-windowed sinc h(u) defined in zs_amd/resample.py (64 zero crossings, 512 table steps each, linear interpolation), and
 * with s = min(1, sr_out / sr_in):
 *   dst[u][t] = s * sum_{m < n_in[u]} src[u][m] * h(s * (t * sr_in / sr_out - m))     t < n_out[u] = ceil(n_in[u] * sr_out / sr_in)
 *   dst[u][t] = 0                                                                      n_out[u] <= t < dst_ld
 * executed in polyphase form: t * sr_in = q * sr_out + r exactly (int64), H = ceil(64 / s),
 *   dst[u][t] = sum_{j = -H..H} tap(r / g, j) * src[u][q + j],     tap(p, j) = s * h(s * (p * g / sr_out - j)),  g = gcd(sr_in, sr_out),
 * samples outside [0, n_in[u]) counting as zero: src[u][m] is never read for m >= n_in[u] (the slack of a row may hold anything).
 * bank: the taps, computed by the caller in fp64 and rounded once to fp32, n_tap = 2 H + 1 rows of n_phase = sr_out / g floats in
 * OUTPUT order:   bank[(j + H) * n_phase + k] = tap((k * (sr_in / g)) mod n_phase, j)      k = t mod n_phase,
 * so that the lanes of a wave, which take consecutive outputs t, read consecutive floats of a row at every tap (the phases of
 * consecutive outputs are a strided permutation of 0..n_phase-1; the permutation is applied once, on the host).
 * One workgroup per (utterance, tile of consecutive outputs), its input span staged in LDS; a thread takes up to four outputs of
 * one phase (a multiple of n_phase apart), which share every tap it loads; fp32 FMA accumulation in the fixed order j = -H..H for
 * every output: a launch is bitwise reproducible and a row's result does not depend on the rows around it.  n_in[u] is clamped to
 * [0, src_ld] and n_out[u] to dst_ld on the device.
 * Errors (nothing is launched): a null pointer with n_utt > 0; n_utt < 0 or > 65535; sr_in <= 0 or sr_out <= 0; sr_out / sr_in
 * outside [1/32, 32]; n_tap != 2 ceil(64 / s) + 1; n_phase != sr_out / g; src_ld or dst_ld <= 0; n_in_max < 0, and with
 * n_in_max > 0 (the host's maximum of n_in, 0 = not known): src_ld < n_in_max or dst_ld < ceil(n_in_max * sr_out / sr_in).
 * n_utt == 0 succeeds and launches nothing. */
typedef struct {
  const float* src; int64_t src_ld;      /* [n_utt][src_ld] */
  const int32_t* n_in;                   /* [n_utt], device */
  int32_t n_utt, sr_in, sr_out;
  const float* bank; int32_t n_phase, n_tap;
  float* dst; int64_t dst_ld;            /* [n_utt][dst_ld], every element written */
  int32_t n_in_max;
} ZsResample;
int zs_resample(const ZsResample* p, void* stream);


/* ---------------------------------------------------------------------------------------------
 * Stage 2 (model/model.py:113-228, trainer.py:257-294, 467-560, utils.py:58-77): PatchDiscriminator /
 * TargetClassifier and the WGAN-GP penalty.
 * Activations of the 2-D nets are channels-last [B, H, W, C] = B*H*W rows of ld elements with H = time and W = frequency, so
 * the loader's [B, T, F] spectrogram IS the input [B, H=T, W=F, C=1] (the reference's Conv2d sees [B, 1, F, T]: its kernel
 * index along F is the tap axis here, the one along T the gather axis).  A k x k / stride-s Conv2d (pad_layer is_2d) runs as
 *   zs_conv2d_gather  : im2col along H only, Xh[(b,ho), w, kh*C + c] = X[b, pad(s*ho + kh - pad), w, c]   (k/s x the input)
 *   zs_gemm_conv      : the existing implicit GEMM over W (taps along W, "batch" = (b, ho)) on the weight viewed as a Conv1d
 *                       weight [Cout, k*C, k];  weight gradient = zs_gemm_wgrad on the same view
 *   data gradient     : zs_gemm_conv(gather=1) into the W-padded domain, then zs_conv2d_fold (reflect folds along W, the
 *                       transpose of the H gather) -- a gather-formulated sum in fixed order, no atomics. */
typedef struct {
  int32_t dtype;
  const void* x; int64_t ldx; int32_t x_f32;     /* [B][H_in][Wd] rows of ldx elements, C valid; fp32 or T */
  void* out; int64_t ldo;                         /* [B][H_out][Wd] rows of ldo >= k*C elements (T dtype; zeros past k*C) */
  int32_t B, H_in, H_out, Wd, C;
  int32_t k, stride, pad, pad_mode;
  /* full != 0: im2col along BOTH axes (the first layer, C = 1: the H-only gather pads its 5 columns per tap to a whole 128-byte
   * K chunk, 12.8 x the input; all 25 taps fit ONE chunk).  Output rows (b, ho, wo), wo < W_out = (Wd + 2 pad - k) / stride + 1,
   * columns (kh*k + kw)*C + c = x[b, pad(stride*ho + kh - pad), pad(stride*wo + kw - pad), c]; the convolution is then a
   * 1-tap zs_gemm_conv over these rows.  zs_conv2d_fold(full) is its transpose. */
  int32_t full;
} ZsConv2dGather;
int zs_conv2d_gather(const ZsConv2dGather* p, void* stream);
typedef struct {
  int32_t dtype;
  const void* gp; int64_t ldg;                    /* [B*H_out][Wd + 2*pad] rows, columns kh*C + c (zs_gemm_conv gather=1 output) */
  void* out; int64_t ldo; int32_t out_f32;        /* [B][H_in][Wd] rows; T dtype: zero filled to fill_cols */
  int32_t fill_cols;
  const void* add; int64_t ldadd;                 /* optional rows added (T dtype, same shape as out) */
  int32_t B, H_in, H_out, Wd, C;
  int32_t k, stride, pad, pad_mode;
  int32_t gp_rows;                                /* rows of gp per (b, h_out) block; 0 = Wd + 2*pad (a stride-2 data gradient is
                                                     computed by output parity and keeps an even number of rows per block) */
  int32_t full;                                   /* transpose of zs_conv2d_gather(full): gp rows (b, ho, wo), columns (kh*k + kw)*C + c */
  /* Refused: 0 < gp_rows < Wd + 2*pad; out_f32 with ldo < C; REFLECT with pad >= H_in or pad >= Wd (as zs_conv2d_gather).
   * Columns [C, fill_cols) of a T-dtype row are written as zeros and read nothing: ldg >= k*C is all that gp needs. */
} ZsConv2dFold;
int zs_conv2d_fold(const ZsConv2dFold* p, void* stream);
/* zs_conv1_fwd: the critic's FIRST Conv2d (one input channel, k x k taps, k*k <= 32, stride 2, padding k/2) computed directly from
 * the fp32 image: every lane of a wave builds its 8 bf16 im2col values (tap order kh*k + kw, as zs_conv2d_gather(full)) from the
 * image and one 16x16x32 MFMA per 16 output channels does the rest -- the [B*Ho*Wo][64] im2col buffer (12.8 x the image) is
 * neither written nor read:  out[(b, ho, wo)][co] = act(bias[co] + sum_{kh, kw} W[co][kh*k + kw] * bf16(x[b][refl(2ho + kh - k/2)][refl(2wo + kw - k/2)])).
 * bf16 only (the fp32 path keeps zs_conv2d_gather(full) + zs_gemm_conv); Cout a multiple of 16, <= 64 per launch column block. */
typedef struct {
  const float* x;                                 /* [B][H][W] */
  const void* W; int64_t ldw;                     /* bf16 [>= Cout][ldw], ldw >= 32, columns >= k*k are zeros (ConvLayer.wf of the layer) */
  const float* bias; int32_t act; float slope;    /* bias may be null; ZS_ACT_NONE / ZS_ACT_LRELU */
  void* out; int64_t ldo;                         /* bf16 [B*Ho*Wo][ldo] */
  int32_t B, H, Wd, Cout, k, pad_mode;
} ZsConv1Fwd;
int zs_conv1_fwd(const ZsConv1Fwd* p, void* stream);
/* zs_conv1_wgrad: weight and bias gradient of the same layer, again straight from the image (the im2col column of a position is
 * rebuilt in registers as the MFMA's B operand, the A operand is gz transposed):
 *   dW[co][kh*k + kw] (+)= sum_m gz[m][co] * bf16(x[...]),  db[co] (+)= sum_m gz[m][co]        (m over all B*Ho*Wo positions)
 * Positions are dealt to the waves of a fixed grid in a fixed order, each workgroup leaves one partial [64][32] in `workspace`,
 * a second kernel sums them in workgroup order: no atomics, bitwise reproducible.  bf16 gz; Cout a multiple of 16, <= 64. */
typedef struct {
  const float* x;                                 /* [B][H][W] */
  const void* gz; int64_t ldg;                    /* bf16 [B*Ho*Wo][ldg] */
  float* dW; int64_t lddw;                        /* fp32 [Cout][lddw], lddw >= k*k */
  float* db;                                      /* optional fp32 [Cout] */
  int32_t accumulate;
  int32_t B, H, Wd, Cout, k, pad_mode;
  float* workspace; size_t workspace_bytes;       /* >= zs_conv1_wgrad_workspace() bytes */
} ZsConv1Wgrad;
size_t zs_conv1_wgrad_workspace(void);
int zs_conv1_wgrad(const ZsConv1Wgrad* p, void* stream);
/* zs_conv2d_unpad: the last step of a stride-2 Conv2d's data gradient computed by output parity (ZsGemmConv with w_in > 0,
 * gather 1): class (ph, pw) holds the gradient at the positions (2 h2 + ph, 2 w2 + pw) of the PADDED input domain
 * [Hp][Wp] as rows [B][Hc(ph) * Wc(pw)], Hc(ph) = (Hp - ph + 1) / 2, Wc(pw) = (Wp - pw + 1) / 2.  This kernel removes the
 * padding -- reflect pads fold back onto the interior positions they mirrored (model/model.py pad_layer_2d), zero pads are
 * dropped -- and interleaves the classes:
 *   out[b][h*W + w][c] = sum over (h', w') in {(h, w) and its reflection partners} of g<(h'+pad)&1><(w'+pad)&1>[...] (+ add) */
typedef struct {
  int32_t dtype;
  const void* g00; const void* g01; const void* g10; const void* g11; int64_t ldg;      /* g<ph><pw> */
  int32_t B, H, W, C, Hp, Wp, pad, pad_mode;
  const void* add; int64_t ldadd;                 /* optional rows added (T dtype, same shape as out) */
  void* out; int64_t ldo; int32_t fill_cols;      /* [B][H*W] rows, zero filled to fill_cols */
} ZsConv2dUnpad;
int zs_conv2d_unpad(const ZsConv2dUnpad* p, void* stream);

/* zs_row_moments: per (b, c) sums over the T rows of a sample, two-stage in a fixed order (no atomics):
 *   u' = u - center_sum[b][c]*center_scale (if center_sum);  m = y ? lrelu'(y) : 1
 *   s1 = sum u'*m;  s2 = sum u'*m*v' (v' = u' when v == u; skipped if s2 == NULL);  s3 = sum u*w (if w)
 * Serves InstanceNorm2d forward (mean, then the centred second moment), its backward (sum g, sum g*a) and the three moments of
 * its double backward. */
typedef struct {
  int32_t dtype;
  const void* u; int64_t ldu;
  const void* v; int64_t ldv;
  const void* y; int64_t ldy; float slope;
  const void* w; int64_t ldw;
  const float* center_sum; float center_scale;
  int32_t B, T, C;
  float* s1; float* s2; float* s3;                /* [B][C] */
  float* partial; size_t partial_bytes;           /* >= zs_row_moments_workspace(B, T, C) */
} ZsRowMoments;
size_t zs_row_moments_workspace(int32_t B, int32_t T, int32_t C);
int zs_row_moments(const ZsRowMoments* p, void* stream);

/* zs_in2d_*: nn.InstanceNorm2d (no affine, biased variance, eps) + nn.Dropout2d over [B, T = H*W, C] rows.
 * dm[b][c] = keep / (1 - p) (1 when dropout is off); xhat = a * inv_dm (inv_dm = 1/dm, 0 for a dropped map).
 *  finalize : mean = s1/n, rstd = 1/sqrt(q/n + eps)         (s1 = sum y, q = sum (y - mean)^2 from zs_row_moments)
 *  fwd      : a = (y - mean) * rstd * dm
 *  bwd      : gz = [rstd*dm*(ga - S1/n) - rstd*xhat*(S2 + S2x)/n] * lrelu'(y)          (S1 = sum ga, S2 = sum ga*a)
 *  adj      : double backward of `bwd` for the gradient penalty: with gbar_y = gbar_z*lrelu'(y), A1 = sum gbar_y, A2 = sum gbar_y*a:
 *               gbar_a = dm*rstd*(gbar_y - A1/n - xhat*inv_dm*A2/n)                       (adjoint of ga)
 *               xbar_a = -inv_dm*rstd*(gbar_y*S2/n + ga*dm*inv_dm*A2/n)                   (adjoint of xhat, as a gradient w.r.t. a)
 *             the adjoint of rstd, A3 = sum gbar_z*gz, is added to S2 (S2x) in the following `bwd` through the forward graph. */
int zs_in2d_finalize(const float* s1, const float* q, float* mean, float* rstd, int64_t n_bc, int32_t T, float eps, void* stream);
/* zs_in2d_stats: mean and rstd of the forward pass in ONE pass over y (instead of zs_row_moments twice + finalize: the rows
 * of a 512-row slab are held in registers for a local mean and a local centred second moment; slabs are merged pairwise in a
 * fixed order with Chan's update  M2 = M2a + M2b + d^2 na nb / n, so the result is as accurate as the two-pass form).
 * y: [B][T] rows of ldy elements (T dtype), C % 8 == 0; partial: >= zs_row_moments_workspace(B, T, C) bytes. */
int zs_in2d_stats(int32_t dtype, const void* y, int64_t ldy, int32_t B, int32_t T, int32_t C, float eps, float* mean, float* rstd,
                  float* partial, size_t partial_bytes, void* stream);
typedef struct {
  int32_t dtype;
  const void* y; int64_t ldy; void* a; int64_t lda;
  const float* mean; const float* rstd; const float* dm;   /* dm may be NULL (1) */
  int32_t B, T, C;
} ZsIn2dFwd;
int zs_in2d_fwd(const ZsIn2dFwd* p, void* stream);
typedef struct {
  int32_t dtype;
  const void* ga; int64_t ldga; const void* ga2; int64_t ldga2;   /* ga2: optional second addend of the incoming gradient */
  const void* a; int64_t lda; const void* y; int64_t ldy;
  const float* S1; const float* S2; const float* S2x; const float* rstd; const float* dm;
  float slope;
  void* gz; int64_t ldgz;
  int32_t B, T, C;
} ZsIn2dBwd;
int zs_in2d_bwd(const ZsIn2dBwd* p, void* stream);
typedef struct {
  int32_t dtype;
  const void* gbz; int64_t ldgbz; const void* y; int64_t ldy; const void* a; int64_t lda; const void* ga; int64_t ldga;
  const float* A1; const float* A2; const float* S2; const float* rstd; const float* dm;
  float slope;
  void* gba; int64_t ldgba; void* xba; int64_t ldxba;
  int32_t B, T, C;
} ZsIn2dAdj;
int zs_in2d_adj(const ZsIn2dAdj* p, void* stream);

/* utils.calculate_gradients_penalty (utils.py:58-77) around the double backward:
 *  zs_lerp_rows : out[b] = alpha[b]*x[b] + (1 - alpha[b])*y[b]   (fp32 rows of n elements)
 *  zs_gp_penalty: s_b = sqrt(1e-12 + sum g_b^2);  *gp = mean_b (1 - s_b)^2;  gbar[b] = scale * (2/B) * (s_b - 1)/s_b * g[b] */
int zs_lerp_rows(const float* x, const float* y, const float* alpha, float* out, int32_t B, int64_t n, void* stream);
int zs_gp_penalty(const float* g, int32_t B, int64_t n, float scale, float* s_out, float* gp_out, float* gbar, void* stream);

/* Trainer.gen_step (trainer.py:266-278) and its gradient.  mode 0: x_gen = xd + m; 1 ('targeted_residual'): x_gen = xd + xd*m.
 * bwd: dpre = dx_gen * (mode ? xd : 1) * (tanh_out ? 1 - m^2 : m*(1 - m))   -- gradient w.r.t. the generator's pre-activation.
 * zs_l1_plain: loss = mean|a - b| (two-stage, fixed order), d = sign(a - b) * scale / n   (trainer.py:539 target-guided loss). */
/* xd, m: fp32 [rows][ld_in] (the decoders' output rows), x_gen / dx_gen: fp32 [rows][F] contiguous (the discriminator's input) */
int zs_gen_combine_fwd(const float* xd, const float* m, int64_t ld_in, float* x_gen, int64_t rows, int32_t F, int32_t mode, void* stream);
typedef struct {
  int32_t dtype;
  const float* dx_gen; int64_t ld_dx; const float* xd; const float* m; int64_t ld_in;
  void* dpre; int64_t ldo; int32_t fill_cols;                            /* T dtype rows */
  int64_t rows; int32_t F; int32_t mode, tanh_out;
} ZsGenCombineBwd;
int zs_gen_combine_bwd(const ZsGenCombineBwd* p, void* stream);
int zs_l1_plain(const float* a, const float* b, int64_t n, float scale, float* partial, float* loss_out, float* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The autolocker step (trainer.py:563-611): re-encode x_gen, BCE against the first encode's units, back to the encoder input.
 * zs_bce_mbv_bwd: torch.nn.BCELoss (mean over N = rows*E) of x = bits (the re-encode's enc_act) against y = target (the first
 * encode's enc_act, both fp32 [rows][E]), logs clamped at -100: loss_out = sum l / N (double partials per block, fixed grid,
 * summed in order by one thread: deterministic).  Fused with the MBV straight-through backward (zs_mbv_bwd):
 *   dx = (x - y) / max(x (1 - x), 1e-12) * grad_scale / N;   dlogits[2e] = dx * y0 (1 - y0) / tau,  dlogits[2e + 1] = -that,
 * with y0 the re-encode's soft unit-0 probability (ZsMbvFwd.y0).  On hard units (x, y in {0, 1}) loss = 100 * mismatches / N and
 * dx = +-1e12 / N at the mismatches.  dlogits: compute dtype [rows][ld], columns [2E, fill_cols) zeroed.
 * partial: >= 1024 doubles.  grad_scale 0 = 1. */
typedef struct {
  int32_t dtype;
  const float* bits; const float* y0; const float* target;
  int64_t rows; int32_t E; float tau; float grad_scale;
  void* dlogits; int64_t ld; int32_t fill_cols;
  double* partial; float* loss_out;
} ZsBceMbvBwd;
int zs_bce_mbv_bwd(const ZsBceMbvBwd* p, void* stream);

/* zs_enc_dx_fold: the encoder's input gradient from its two parts.  g: fp32 [B][T + 2 pad][ldg], the data gradient of the
 * conv bank over its input padded by `pad` rows on both sides; pass_through (optional, compute dtype [B][T][ld_pass]): the gradient of
 * the concatenation's pass-through columns.  dx fp32 [B][T][ldx] = g[b, t + pad] + (REFLECT: the padding rows that mirror row t)
 * + pass_through[b, t].  ZERO padding drops the padding rows.  REFLECT needs T > pad. */
typedef struct {
  int32_t dtype;
  const float* g; int64_t ldg;
  const void* pass_through; int64_t ld_pass;
  int32_t B, T, C, pad, pad_mode;
  float* dx; int64_t ldx;
} ZsEncDxFold;
int zs_enc_dx_fold(const ZsEncDxFold* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * zs_eval_accum: one held-out validation batch added into device-resident tables (zs_amd.validation).  No host
 * synchronisation, no gradient, no allocation; the host reads the tables once, after the last batch.
 * Reconstruction error per speaker.  x_dec fp32 [B*T][ld_dec], x fp32 [B*T][ldx] (F valid columns each; the padding columns
 * are never read), c int64 [B]:
 *   s_b = sum_{t, f} |x_dec - x|       the difference in fp32, the sum in double: ZS_EVAL_PARTS workgroups per sample, each
 *                                      over a fixed share of the rows in a fixed order, their partials summed in order
 *   for b = 0 .. B-1 in this order:    spk_sum[c[b]] += s_b (double),  spk_cnt[c[b]] += 1
 * There is no floating-point atomic: the same launch on the same tables gives the same bits.  A c[b] outside [0, n_speakers) is
 * never used as an index: the sample is skipped and *bad += 1.  work: scratch of >= B * ZS_EVAL_PARTS doubles.
 * 16-byte loads of four columns need 4-byte alignment only; columns F - F % 4 .. F - 1 are read one by one.
 * Unit statistics (bits_f32 == null skips them and leaves ones / flips / rows / pairs alone).  bits_f32 fp32 [B*T4][E], dense, the
 * 0 / 1 units the encoder writes (a unit is set when its value != 0):
 *   ones[j]  += #{rows with unit j set}
 *   flips[j] += #{(b, t), t + 1 < T4 : unit j of rows (b, t) and (b, t + 1) differs}      (never across two samples)
 *   *rows += B * T4,  *pairs += B * (T4 - 1)
 * added with integer atomics (integer sums do not depend on the order).
 * ZS_EINVAL (nothing launched): a null struct or required pointer (x_dec, x, c, work, spk_sum, spk_cnt, bad; with bits_f32 also
 * ones, flips, rows, pairs), B, T or F <= 0, T * F >= 2^31, ld_dec < F, ldx < F, n_speakers <= 0 or > 2^24, with bits_f32 T4 <= 0 or
 * E <= 0. */
#define ZS_EVAL_PARTS 8
typedef struct {
  const float* x_dec; int64_t ld_dec;
  const float* x; int64_t ldx;
  const int64_t* c;
  int32_t B, T, F, n_speakers;
  double* work;
  double* spk_sum; int64_t* spk_cnt; uint64_t* bad;
  const float* bits_f32; int32_t T4, E;
  uint64_t* ones; uint64_t* flips; uint64_t* rows; uint64_t* pairs;
} ZsEvalAccum;
int zs_eval_accum(const ZsEvalAccum* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Unit codebook (zs_amd.codebook): K codewords of E bits, fitted by k-modes over bit-packed units; a unit is snapped to its nearest
 * codeword in Hamming distance.  Rows and bit order are zs_units_pack's (convert.pack_units): `units` uint8 [n][row_bytes], `code`
 * uint8 [K][code_bytes], bit j of byte b is column 8b + j.  Only the (E + 7) / 8 bytes of a row that carry columns are read or
 * written: bits at columns >= E of the last of them are ignored on input (units and codewords) and zero on output, and the bytes
 * of a pitch behind them are never touched.  Everything is integer, so every result is bitwise reproducible.
 * Limits: 1 <= E <= ZS_CODE_MAX_E, 1 <= K <= ZS_CODE_MAX_K, row_bytes and code_bytes >= (E + 7) / 8, 0 <= n < 2^40.  n == 0 succeeds
 * and launches nothing.  A null struct, K < 1, K > ZS_CODE_MAX_K, E < 1, E > ZS_CODE_MAX_E, n < 0, a pitch too small or a null
 * operand with work to do return ZS_EINVAL and launch nothing.  No allocation, no synchronisation; launches are stream-ordered.
 *
 * zs_code_assign: for every unit the codeword of least Hamming distance over the columns < E; ties go to the lowest index.
 *   idx[i]     = that codeword                                   (int32 [n], optional)
 *   dist[i]    = its distance                                    (int32 [n], optional)
 *   snapped[i] = code[idx[i]], bits >= E zero                    (uint8 [n][row_bytes], optional; may be `units` itself: in place)
 *   *total    += sum_i dist[i]                                   (int64, optional)
 * One unit row per lane in registers (two above ZS_CODE_BIG_N rows); the codewords go through LDS ZS_CODE_TILE_WORDS dwords at a
 * time, a codeword padded to the next power of two of its dwords, i.e. ZS_CODE_TILE_WORDS / pow2(ceil(E / 32)) codewords per pass.
 * Below ZS_CODE_SPLIT_N rows the 16 waves of a workgroup share 64 units and a sixteenth of every pass each. */
#define ZS_CODE_MAX_E 1024
#define ZS_CODE_MAX_K 65536
#define ZS_CODE_TILE_WORDS 4096
#define ZS_CODE_BIG_N 262144
#define ZS_CODE_SPLIT_N 65536
typedef struct {
  const uint8_t* units; int64_t n; int32_t row_bytes;
  const uint8_t* code; int32_t K, code_bytes, E;
  int32_t* idx; int32_t* dist; uint8_t* snapped; int64_t* total;
} ZsCodeAssign;
int zs_code_assign(const ZsCodeAssign* p, void* stream);
/* zs_code_accum: the votes of one k-modes iteration.  For every unit i with 0 <= idx[i] < K:
 *   cnt[idx[i]] += 1,   ones[idx[i]][j] += bit j of unit i  (j < E)          cnt int32 [K], ones int32 [K][E], dense
 * An idx[i] outside [0, K) is never used as an index: the unit is skipped and *bad += 1 (int32).  Integer atomics, privatised: a
 * workgroup keeps the counters of a tile of codewords in LDS over its slice of the units and adds the non-zero ones at the end. */
typedef struct {
  const uint8_t* units; const int32_t* idx; int64_t n; int32_t row_bytes, K, E;
  int32_t* cnt; int32_t* ones; int32_t* bad;
} ZsCodeAccum;
int zs_code_accum(const ZsCodeAccum* p, void* stream);
/* zs_code_update: majority vote.  For every k with cnt[k] > 0, bit j < E of code[k] becomes 1 if 2 ones[k][j] > cnt[k], 0 if
 * 2 ones[k][j] < cnt[k], and stays if they are equal; cnt[k] <= 0 leaves every byte of code[k] as it is.
 * *changed += #{k : code[k] differs from before in a column < E}  (int32). */
typedef struct {
  uint8_t* code; int32_t K, code_bytes, E;
  const int32_t* cnt; const int32_t* ones; int32_t* changed;
} ZsCodeUpdate;
int zs_code_update(const ZsCodeUpdate* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Vector codebook (zs_amd.vq): K real-valued codewords of E columns for enc_mode 'continues', fitted by k-means over encoder rows; an
 * encoded frame is snapped to its nearest codeword in Euclidean distance and a unit file is the sequence of indices.  `code` is fp32
 * [K][ld_code], `cnorm` fp32 [K] (the squared norms, kept by the caller / zs_vq_update).  Limits: 1 <= K <= ZS_CODE_MAX_K,
 * 1 <= E <= ZS_CODE_MAX_E, 0 <= n < 2^31, every leading dimension >= E.  A null struct, a K, E or n outside its range, a leading
 * dimension below E, a null operand with work to do or an operand not aligned to its element return ZS_EINVAL and launch nothing;
 * n == 0 (n_frag == 0) succeeds and launches nothing.  Caller-owned buffers, no allocation, no synchronisation, stream-ordered.
 *
 * zs_vq_assign: x [n][ld_x] of `dtype` (fp32 when src_f32), read in place (the encoder's own output rows of a chunk are such an
 * operand, as for zs_units_pack).  The score of row i against codeword k is
 *   s(i, k) = cnorm[k] - 2 sum_j x[i][j] code[k][j]
 * with exact fp32 operands (bf16 widened), the products and the sum in fp32 on v_mfma_f32_32x32x2_f32, one rounding for the
 * subtraction.  idx[i] is the k of least computed score, ties to the lowest k.  Every output is optional:
 *   idx[i]   = that k                                            (int32 [n])
 *   dist[i]  = max(0, |x_i|^2 + s(i, idx[i])), |x_i|^2 in fp32   (fp32 [n])
 *   *moved  += #{i : idx[i] differs from the value found in idx[i] on entry}     (int32; when count_moved, which needs idx and moved)
 * Two decompositions with bitwise equal results (one pair's score does not depend on where the codeword sits):
 *   rows   a workgroup owns 128 rows and walks the codewords ZS_VQ_TILE_K at a time with a running best per row;
 *   split  below ZS_VQ_SPLIT_N rows, when `work` is given and K > ZS_VQ_TILE_K: the codeword tiles are dealt to about
 *          ZS_VQ_SPLIT_WGS workgroups in all, whose (orderable score, k) words meet by a 64-bit minimum in `work` (order-independent),
 *          and a second launch writes the outputs.  `work` is 8-byte aligned and holds ZS_VQ_WORK_BYTES (12 bytes per row is what is
 *          asked for); work == NULL selects `rows` at any n.
 * Results are bitwise equal from run to run. */
#define ZS_VQ_TILE_K 128
#define ZS_VQ_SPLIT_N 32768
#define ZS_VQ_SPLIT_WGS 512
#define ZS_VQ_WORK_BYTES 393216
typedef struct {
  int32_t dtype, src_f32;
  const void* x; int64_t n, ld_x;
  const float* code; int64_t ld_code; const float* cnorm; int32_t K, E;
  int32_t* idx; float* dist; int32_t* moved; int32_t count_moved;
  void* work; int64_t work_bytes;
} ZsVqAssign;
int zs_vq_assign(const ZsVqAssign* p, void* stream);
/* zs_vq_accum: the sums of one k-means iteration, in fixed point.  x fp32 [n][ld_x].  For every row i with 0 <= idx[i] < K:
 *   cnt[idx[i]] += 1,   sum[idx[i]][j] += q(x[i][j])  (j < E)                  cnt int32 [K], sum int64 [K][E], dense
 *   q(v) = (int64) rint(v 2^shift), the product exact in double, half to even; -64 <= shift <= 62
 * Integer sums do not depend on the order of the adds.  An idx[i] outside [0, K) is never used as an index: the row is skipped and
 * *bad += 1 (int32).  Privatised as zs_code_accum: a workgroup keeps the sums of a tile of codewords in LDS over its slice of the rows. */
typedef struct {
  const float* x; const int32_t* idx; int64_t n, ld_x; int32_t K, E, shift;
  int32_t* cnt; int64_t* sum; int32_t* bad;
} ZsVqAccum;
int zs_vq_accum(const ZsVqAccum* p, void* stream);
/* zs_vq_update: the means.  For every k with cnt[k] > 0 and j < E
 *   code[k][j] = (float)((double)sum[k][j] / (double)cnt[k] * 2^-shift)
 * (int64 -> double to nearest even, an IEEE division, an exact scaling, one rounding to fp32); cnt[k] <= 0 leaves the row as it is.
 * cnorm[k] is rewritten for EVERY k as the fp32 rounding of sum_j code[k][j]^2 accumulated in double.
 * *changed += #{k : code[k] differs bitwise from before}  (int32). */
typedef struct {
  float* code; int64_t ld_code; float* cnorm; int32_t K, E, shift;
  const int32_t* cnt; const int64_t* sum; int32_t* changed;
} ZsVqUpdate;
int zs_vq_update(const ZsVqUpdate* p, void* stream);
/* zs_vq_gather: indices straight into the Decoder's input operand of one inference chunk (zs_units_unpack for codewords).  idx int32
 * [n_idx] holds every utterance of a batch; start (int64 [n_frag], an entry of idx) and len (int32 [n_frag]) are device tables.
 * dst [n_frag][T][ld_dst] of `dtype`, 16-byte aligned, ld_dst a multiple of 8, written with 16-byte stores:
 *   dst[f][t][c] = cast(code[idx[start[f] + t]][c])             t < len[f], c < E      (round to nearest even)
 *   dst[f][t][c] = 0                                             len[f] <= t < T, or E <= c < ld_dst
 * An entry with len < 0, len > T, start < 0 or start + len > n_idx writes a zero fragment and reads nothing; an idx outside [0, K)
 * writes a zero row and *bad += 1 (int32).  n_frag in [0, ZS_UNITS_MAX_FRAG]. */
typedef struct {
  int32_t dtype;
  const int32_t* idx; int64_t n_idx;
  const float* code; int64_t ld_code; int32_t K, E;
  const int64_t* start; const int32_t* len; int32_t n_frag, T;
  void* dst; int64_t ld_dst; int32_t* bad;
} ZsVqGather;
int zs_vq_gather(const ZsVqGather* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training through the vector codebook (zs_amd.vq_train): the straight-through quantiser between the 'continues' Encoder and
 * the Decoder, its commitment term and the exponential moving average that moves the codebook after the encoder.  One training
 * iteration is zs_vq_assign (above, unchanged) -> zs_vq_commit -> zs_vq_accum (above, unchanged) -> zs_vq_ema (-> zs_vq_restart when
 * dead codewords are restarted) in the forward and zs_vq_st_bwd in the backward.  `code` fp32 [K][ld_code] and the limits on K, E, n and the leading dimensions are the vector
 * codebook's (above).  A null struct, a K, E or n outside its range, a leading dimension below E, a null operand with work to do or a
 * misaligned operand return ZS_EINVAL and launch nothing; n == 0 succeeds and launches nothing.  Caller-owned buffers, no allocation,
 * no synchronisation, stream-ordered; no launch argument depends on the iteration, so a captured graph replays them.  No float
 * atomics: every result is bitwise equal from run to run.
 *
 * zs_vq_commit: the Decoder's operand and the commitment loss.  z [n][ld_z] of `dtype` (the encoder's rows, read in place, any
 * alignment of its element), idx int32 [n].  q [n][ld_q] of `dtype`, 16-byte aligned, ld_q a multiple of 8, written with 16-byte stores:
 *   q[i][j]      = cast(code[idx[i]][j])   j < E (round to nearest even);   0 for E <= j < ld_q
 *   z_f32[i][j]  = (float) z[i][j]         j < E      (fp32 [n][ld_zf], optional: the operand zs_vq_accum wants when z is bf16)
 *   idx_acc[i]   = idx[i], or -1 when row i has an element that is not of magnitude < ZS_VQ_MAX_ABS (NaN included): zs_vq_accum
 *                  then leaves the row out, so its int64 sums cannot overflow under vq_shift(n, ZS_VQ_MAX_ABS); *over += 1 for
 *                  such a row.  (int32 [n], optional, must not overlap idx; over int32, optional)
 *   *loss        = (float)(scale * sum_ij ((double) z[i][j] - (double) code[idx[i]][j])^2)   (optional; needs partial)
 * The sum: every lane adds its terms in double in a fixed order, a workgroup's lanes are summed in a fixed tree into
 * partial[workgroup] (double [ZS_VQ_COMMIT_PARTS]) and a second launch of one workgroup adds the partials in a fixed order.
 * An idx[i] outside [0, K) is never used as an index: q[i] is a zero row, the row is left out of the loss, idx_acc[i] = -1 and
 * *bad += 1 (int32, required).  A row is owned by a team of 2^t <= 64 lanes of one wave, one 16-byte piece of q per lane and round. */
#define ZS_VQ_COMMIT_PARTS 1024
#define ZS_VQ_MAX_ABS 65536
typedef struct {
  int32_t dtype;
  const void* z; int64_t n, ld_z;
  const int32_t* idx;
  const float* code; int64_t ld_code; int32_t K, E;
  void* q; int64_t ld_q;
  float* z_f32; int64_t ld_zf;
  int32_t* idx_acc;
  double scale; double* partial; float* loss;
  int32_t* bad; int32_t* over;
} ZsVqCommit;
int zs_vq_commit(const ZsVqCommit* p, void* stream);
/* zs_vq_st_bwd: the straight-through gradient plus the commitment term's.  dq, dz [n][ld] of `dtype`, 16-byte aligned, both leading
 * dimensions multiples of 8; z [n][ld_z] of `dtype`; g fp32 (2 beta / (n E), rounded once by the caller):
 *   dz[i][j] = cast(dq[i][j] + g * (z[i][j] - code[idx[i]][j]))   j < E;    0 for E <= j < ld_dz
 * The subtraction, the product and the sum are three fp32 operations, each rounded once (no fused multiply-add), then one cast.
 * dz == dq (with ld_dz == ld_dq) updates in place; any other overlap is undefined.  The codeword row is read again, so the forward
 * keeps no residual.  An idx[i] outside [0, K) is never used as an index: dz[i] = dq[i] and *bad += 1 (int32, required). */
typedef struct {
  int32_t dtype;
  const void* dq; int64_t n, ld_dq;
  const void* z; int64_t ld_z;
  const int32_t* idx;
  const float* code; int64_t ld_code; int32_t K, E;
  float g;
  void* dz; int64_t ld_dz;
  int32_t* bad;
} ZsVqStBwd;
int zs_vq_st_bwd(const ZsVqStBwd* p, void* stream);
/* zs_vq_ema: the codebook follows the encoder.  cnt int32 [K] and sum int64 [K][E] as zs_vq_accum left them (shift: its shift);
 * N fp32 [K], m fp32 [K][E] dense; decay a double in [0, 1).  For every k, in IEEE double with one rounding per stored fp32:
 *   N[k]       = (float)(decay N[k]    + (1 - decay) cnt[k])
 *   m[k][j]    = (float)(decay m[k][j] + (1 - decay) (double) sum[k][j] 2^-shift)
 *   code[k][j] = (float)((double) m[k][j] / (double) N[k])      when the new N[k] >= 1e-3; else the row stays as it is
 * (no fused multiply-add; int64 -> double to nearest even; 1 - decay in double).  cnorm[k] is rewritten for EVERY k exactly as
 * zs_vq_update writes it: lane t of 256 adds code[k][j]^2, j = t, t + 256, .., in double, the 64 lanes of a wave are added
 * pairwise at distances 32, 16, .., 1, and the four waves' sums left to right.  *used += #{k : cnt[k] > 0} (int32, optional).
 * Nothing is summed across k.  One workgroup per codeword. */
typedef struct {
  const int32_t* cnt; const int64_t* sum; int32_t K, E, shift;
  double decay;
  float* N; float* m;
  float* code; int64_t ld_code; float* cnorm;
  int32_t* used;
} ZsVqEma;
int zs_vq_ema(const ZsVqEma* p, void* stream);
/* zs_vq_restart: dead codewords go back onto this step's encoder rows, directly behind zs_vq_ema on the same stream.
 * x fp32 [n][ld_x] (the rows zs_vq_accum read), idx_acc int32 [n] (optional: zs_vq_commit's), cnt int32 [K] (zs_vq_accum's), and
 * N, m [K][E] dense, code [K][ld_code], cnorm as zs_vq_ema just left them.  thresh fp32 in (0, 1); 1 <= stride <= n.
 *   dead(k)  = cnt[k] == 0 && N[k] < thresh            (fp32 comparison: NaN and equality are not dead)
 *   j(k)     = #{k' < k : dead(k')}
 *   start    = mix64(seed + *seed_ptr + 0x5651524553544152) mod n      (unsigned 64-bit, wrapping; seed_ptr optional)
 *   mix64(z) : z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   r(k)     = (start + (j(k) mod n) * stride) mod n
 * For every dead k: when idx_acc is given and idx_acc[r(k)] < 0 the codeword stays and *skipped += 1; else code[k][j] = m[k][j] =
 * x[r(k)][j] for j < E, N[k] = 1, cnorm[k] = the double sum of squares in zs_vq_ema's order rounded once, and *restarted += 1
 * (both int32, required).  Columns E <= j < ld_code are not touched.  work int32 [K + 2], required, undefined afterwards.  Two
 * launches: one workgroup ranks the K flags into work, then one workgroup per dead codeword (at most 1024, striding) copies its row;
 * with nothing dead the second reads one word per workgroup and writes nothing.  n == 0 succeeds and launches nothing; a thresh
 * outside (0, 1) or a stride outside [1, n] is ZS_EINVAL as the cases above are.  No float atomics. */
typedef struct {
  float thresh;
  const float* x; int64_t n, ld_x;
  const int32_t* idx_acc;
  const int32_t* cnt; int32_t K, E;
  float* N; float* m;
  float* code; int64_t ld_code; float* cnorm;
  uint64_t seed;
  const uint64_t* seed_ptr;
  int32_t stride;
  int32_t* work;
  int32_t* restarted; int32_t* skipped;
} ZsVqRestart;
int zs_vq_restart(const ZsVqRestart* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Residual vector codebook (zs_amd.rvq): S codebooks of K codewords each, stage s quantising what stage s - 1 left over,
 * 2 <= S <= ZS_RVQ_MAX_S in a file (the kernels take S = 1 too).  The search of every stage is zs_vq_assign (above, unchanged); the two
 * entry points here are the glue around it.  The limits on K, E, n and the leading dimensions are the vector codebook's.  A null struct,
 * a K, E, n, S or s_use outside its range, a leading dimension below E, a null operand with work to do or a misaligned operand return
 * ZS_EINVAL and launch nothing; n == 0 (n_frag == 0) succeeds and launches nothing.  Caller-owned buffers, no allocation, no
 * synchronisation, stream-ordered; no float atomics and no fused multiply-add: every result is bitwise equal from run to run.
 *
 * zs_rvq_residual: what a stage leaves over.  x [n][ld_x] of `dtype` (fp32 when src_f32; aligned to its element), idx int32 [n],
 * code fp32 [K][ld_code]; r fp32 [n][ld_r], ld_r >= E:
 *   r[i][j] = (float) x[i][j] - code[idx[i]][j]        j < E       (one IEEE fp32 subtraction; bf16 widened exactly)
 * Columns E <= j < ld_r are not touched.  An idx[i] outside [0, K) is never used as an index: r[i] = (float) x[i] and *bad += 1
 * (int32, required).  r == x is allowed when x is fp32 and ld_r == ld_x (every lane reads the piece it writes); any other overlap is
 * undefined.  A row is owned by a team of 2^t <= 64 lanes of one wave, four columns per lane and round, with 16-byte loads and
 * stores where the operand is 16-byte aligned (x bf16: 8) and its leading dimension a multiple of 4, element by element otherwise. */
#define ZS_RVQ_MAX_S 8
typedef struct {
  int32_t dtype, src_f32;
  const void* x; int64_t n, ld_x;
  const int32_t* idx;
  const float* code; int64_t ld_code; int32_t K, E;
  float* r; int64_t ld_r;
  int32_t* bad;
} ZsRvqResidual;
int zs_rvq_residual(const ZsRvqResidual* p, void* stream);
/* zs_rvq_gather: S planes of indices straight into the Decoder's input operand of one inference chunk (zs_vq_gather for a sum of
 * codewords).  idx int32 [S][ld_idx]: plane s holds stage s of every frame of the batch, n_idx <= ld_idx entries of it; code fp32
 * [S][K][ld_code], the codebooks plane_code elements apart (>= (K - 1) ld_code + E); the first s_use stages are used, 1 <= s_use <= S
 * <= ZS_RVQ_MAX_S.  start, len, n_frag, T, dst, ld_dst and bad exactly as in ZsVqGather:
 *   dst[f][t][c] = cast(((code[0][k_0][c] + code[1][k_1][c]) + ..) + code[s_use - 1][k_{s_use - 1}][c])     t < len[f], c < E
 *                  with k_s = idx[s][start[f] + t]; fp32 adds in increasing s, each rounded once, then one cast (to nearest even)
 *   dst[f][t][c] = 0                                             len[f] <= t < T, or E <= c < ld_dst
 * A frame with any of its s_use indices outside [0, K) writes a zero row and *bad += 1 (once per frame); no index of such a frame is
 * used as an index, and the planes s >= s_use are not read.  With S = s_use = 1 the operand is zs_vq_gather's, bit for bit. */
typedef struct {
  int32_t dtype;
  const int32_t* idx; int64_t n_idx, ld_idx; int32_t S, s_use;
  const float* code; int64_t ld_code, plane_code; int32_t K, E;
  const int64_t* start; const int32_t* len; int32_t n_frag, T;
  void* dst; int64_t ld_dst; int32_t* bad;
} ZsRvqGather;
int zs_rvq_gather(const ZsRvqGather* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training through the residual codebook (zs_amd.rvq_train): the per-stage glue of the S-stage straight-through quantiser.
 * One training iteration is, for every stage s in increasing order, zs_vq_assign -> zs_rvq_commit -> zs_vq_accum -> zs_vq_ema
 * (-> zs_vq_restart), all but the second unchanged, then zs_rvq_loss and zs_rvq_gather (above, unchanged: the Decoder's operand) in
 * the forward and zs_rvq_st_bwd in the backward.  The limits on K, E, n and the leading dimensions are the vector codebook's.  A null
 * struct, a K, E, n or S outside its range, a leading dimension below E, a null operand with work to do, a misaligned operand or a
 * forbidden overlap return ZS_EINVAL and launch nothing; n == 0 succeeds and launches nothing.  Caller-owned buffers, no allocation, no
 * synchronisation, stream-ordered; no launch argument depends on the iteration, so a captured graph replays them.  No float atomics
 * and no fused multiply-add: every result is bitwise equal from run to run.
 *
 * zs_rvq_commit: what stage s leaves over, and everything the step wants of it, in one pass over the row.  x [n][ld_x] of `dtype`
 * (fp32 when src_f32; aligned to its element) is r_s, the stage's input: the encoder's rows at stage 0, the fp32 residual behind it.
 * idx int32 [n] (zs_vq_assign's of this stage), code fp32 [K][ld_code].  With ok(i) = 0 <= idx[i] < K:
 *   r[i][j]      = (float) x[i][j] - code[idx[i]][j]      j < E   (fp32 [n][ld_r]; one IEEE fp32 subtraction, bf16 widened exactly)
 *   x_f32[i][j]  = (float) x[i][j]                        j < E   (fp32 [n][ld_xf], optional: the operand zs_vq_accum wants of bf16 rows)
 *   idx_acc[i]   = idx[i], or -1 when !ok(i) or row i of x has an element that is not of magnitude < ZS_VQ_MAX_ABS (NaN included);
 *                  *over += 1 for such a row of x                                      (int32 [n], required; over int32, required)
 *   a[i][j]      = r[i][j]            when `first`;   a[i][j] + r[i][j] otherwise (read, one fp32 add, written)   (fp32 [n][ld_a])
 *   partial[w]   = the sum over the rows of workgroup w of (double) r[i][j] * (double) r[i][j], the STORED fp32 residual: every lane
 *                  adds its terms in double in a fixed order, the 64 lanes of a wave are added pairwise at distances 32, .., 1 and the
 *                  four waves left to right; partial[w] = 0 for the launch's workgroup count <= w < ZS_VQ_COMMIT_PARTS
 *                  (double [ZS_VQ_COMMIT_PARTS], required: zs_rvq_loss reads all of them)
 * Columns E <= j of r, x_f32 and a are not touched.  A row with !ok(i) is never used as an index: r[i] = (float) x[i], it adds nothing
 * to partial, a[i] = 0 when `first` and is left as it is otherwise, idx_acc[i] = -1 and *bad += 1 (int32, required).  r, x_f32 and a
 * must not be x or each other.  A row is owned by a team of 2^t <= 64 lanes of one wave, four columns per lane and round, with 16-byte
 * loads and stores where the operand is 16-byte aligned (x bf16: 8) and its leading dimension a multiple of 4, element by element
 * otherwise; the magnitude check is an OR over the team. */
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
} ZsRvqCommit;
int zs_rvq_commit(const ZsRvqCommit* p, void* stream);
/* zs_rvq_loss: the commitment loss of the S stages from zs_rvq_commit's partials.  partial double [S][ZS_VQ_COMMIT_PARTS] dense,
 * 1 <= S <= ZS_RVQ_MAX_S; loss fp32 [1 + S].  d_s = the sum of partial[s][.]: lane t of 256 adds partial[s][t], [t + 256], .. in
 * double, a wave's lanes are added pairwise at distances 32, .., 1 and the four waves left to right.
 *   loss[1 + s] = (float)(scale * d_s)
 *   loss[0]     = (float)(scale * (((d_0 + d_1) + ..) + d_{S-1}))         (doubles, in increasing s; scale = beta / (n E), a double)
 * One workgroup.  It has no n: it always launches. */
typedef struct {
  const double* partial; int32_t S;
  double scale;
  float* loss;
} ZsRvqLoss;
int zs_rvq_loss(const ZsRvqLoss* p, void* stream);
/* zs_rvq_st_bwd: the straight-through gradient plus the commitment terms' of every stage.  dq, dz [n][ld] of `dtype`, 16-byte
 * aligned, both leading dimensions multiples of 8; a fp32 [n][ld_a] as the last zs_rvq_commit left it (r_1 + .. + r_S added in
 * increasing stage); g fp32 (2 beta / (n E), rounded once by the caller):
 *   dz[i][j] = cast(dq[i][j] + g * a[i][j])      j < E;    0 for E <= j < ld_dz
 * The product and the sum are two fp32 operations, each rounded once (no fused multiply-add), then one cast (to nearest even).  With
 * S = 1 this is zs_vq_st_bwd's value bit for bit.  dz == dq (with ld_dz == ld_dq) updates in place; any other overlap is undefined.
 * One lane per 16-byte piece of dz, grid-stride; a is read with 16-byte loads when it is 16-byte aligned and ld_a a multiple of 4. */
typedef struct {
  int32_t dtype;
  const void* dq; int64_t n, ld_dq;
  const float* a; int64_t ld_a;
  int32_t E;
  float g;
  void* dz; int64_t ld_dz;
} ZsRvqStBwd;
int zs_rvq_st_bwd(const ZsRvqStBwd* p, void* stream);
/* zs_xfade_gather: the vocoder's padded input out of decode windows that overlap (convert.unit_windows): every output row is one
 * source row, or the cross-fade of two.  src fp32 [src_rows][ld_src]; out fp32 [rows][out_ld]; i0, i1 int32 [rows] and w0, w1 fp32
 * [rows], device tables planned on the host (convert._xfade_tables); cols <= min(ld_src, out_ld):
 *   out[r][f] = D( i0[r] < 0 ? 0
 *                : i1[r] < 0 ? src[i0[r]][f]
 *                : fl32(fl32(w0[r] * src[i0[r]][f]) + fl32(w1[r] * src[i1[r]][f])) )        f < cols
 * Two products and one sum, each rounded once to fp32 (no fused multiply-add); a row with one source is copied, not multiplied, and
 * w0, w1 are read for blended rows only.  D: the expression of zs_gl_denormalize / zs_gen_scatter (one shared device function: the
 * same bits for the same input) when denorm is set, else the identity.  A row with i0 outside [-1, src_rows) or i1 outside
 * [-1, src_rows) reads nothing and holds D(0), as zs_frag_gather treats a bad table entry.  out must not alias src; the columns
 * cols <= f < out_ld are not written.  Rows need only 4-byte alignment (513 floats): one wave per row, the grid strides over rows,
 * 16-byte stores over the 16-byte aligned middle of an output row (the source rows read in 16-byte pieces at their own 4-byte
 * alignment, both rows of a blended frame in the same pass) and single elements at its two ends.
 * No allocation, no synchronisation, no atomics; stream-ordered and bitwise reproducible.  Errors (ZS_EINVAL, nothing is launched):
 * a null operand with rows > 0; a negative size; cols > ld_src or cols > out_ld; rows >= 2^31.  rows == 0 succeeds and launches
 * nothing. */
typedef struct {
  const float* src; int64_t src_rows, ld_src;
  const int32_t* i0; const int32_t* i1;
  const float* w0; const float* w1;
  float* out; int64_t rows, out_ld;
  int32_t cols, denorm;
} ZsXfadeGather;
int zs_xfade_gather(const ZsXfadeGather* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif

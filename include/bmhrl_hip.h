/*
 * bmhrl_hip.h -- C ABI of the MI355X (gfx950) hot path of Berghojo/bmhrl.
 *
 * The reference has no native code: its hot path is a chain of stock torch ops
 * (model/multihead_attention.py, model/blocks.py, model/bm_hrl_agent.py, loss/,
 * epoch_loops/captioning_bmrl_loops.py).  Each entry point below replaces one such chain
 * and cites it.  All pointers are DEVICE pointers owned by the caller; nothing is
 * allocated or freed inside; every call enqueues work on `stream` and returns
 * immediately (0 = ok, negative = -errno style argument error, positive = hipError_t).
 * No global mutable state: calls are re-entrant across processes (one process per GPU).
 *
 * bf16 tensors are passed as `void*` to 16-bit storage.  Every 2-D bf16 buffer has an
 * explicit leading dimension (elements) that must be a multiple of 8; padding columns
 * must hold finite values (the library never writes them; allocate zeroed).
 */
#ifndef BMHRL_HIP_H
#define BMHRL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* bmhrl_stream_t; /* hipStream_t */

/* ---------------------------------------------------------------------------------------------
 * Batched MFMA GEMM with fused epilogue:  C[b](M,N) = epilogue( sum_k A[b](m,k) * B[b](k,n) )
 * Replaces nn.Linear forward/backward (model/multihead_attention.py:70-72,89; model/blocks.py:178-184;
 * model/bm_hrl_agent.py:439,464) and the Q.K^T / P.V products of attention() backward
 * (model/multihead_attention.py:13,25).  bf16 operands, fp32 accumulate.
 *   a_trans = 0: A stored [M][K] (k contiguous, leading dim lda)   1: stored [K][M]
 *   b_trans = 0: B stored [N][K] (k contiguous; nn.Linear weight)  1: stored [K][N]
 *   batch index = b1 * batch2 + b2; element offset of operand X = b1 * x_sb1 + b2 * x_sb2.
 * ------------------------------------------------------------------------------------------- */
enum {
  BMHRL_EPI_LINEAR = 0, /* v = alpha*acc (+bias[n]) ; mask==0 -> -1e9 ; relu ; dropout ; (+residual[m][n]) */
  BMHRL_EPI_PROB = 1,   /* p = exp(masked(alpha*acc) - rowvec[m]) / rowvec2[m]        (recompute softmax P) */
  BMHRL_EPI_DSCORE = 2, /* ds = aux[m][n] * (acc - rowvec[m]) * alpha, 0 where mask == 0 (softmax backward) */
  BMHRL_EPI_RELU_BWD = 3 /* dz = aux[m][n] > 0 ? alpha*acc : 0     (ReLU + inverted-dropout backward of the FFN) */
};

typedef struct bmhrl_gemm_desc {
  int32_t M, N, K;
  int32_t batch1, batch2;
  const void* A; int64_t lda, a_sb1, a_sb2; int32_t a_trans;
  const void* B; int64_t ldb, b_sb1, b_sb2; int32_t b_trans;
  float* C;  int64_t ldc, c_sb1, c_sb2;          /* fp32 output, may be NULL */
  void* Cb;  int64_t ldcb, cb_sb1, cb_sb2;       /* bf16 output, may be NULL */
  int32_t epilogue;
  float alpha;
  int32_t relu;
  int32_t accumulate;                             /* C += v instead of C = v (fp32 output only: refused (-22) together with
                                                     Cb or colsum) */
  int32_t allow_split_k;                          /* C is zero-initialised: long reductions may be split (fp32 atomics) */
  const float* bias;                              /* [N] or NULL */
  const float* residual; int64_t ldr, r_sb1, r_sb2; /* fp32 [M][N] or NULL */
  const uint8_t* mask; int64_t mask_sb1, mask_sm; /* byte mask[b1][m*mask_sm + n], mask_sm may be 0 */
  const float* rowvec; const float* rowvec2; int64_t rv_sb1, rv_sb2; /* per-row fp32 vectors: (row max, row sum) or delta */
  const void* aux; int64_t ldaux, aux_sb1, aux_sb2; /* bf16 [M][N] (P for DSCORE) */
  float dropout_p; uint64_t seed;                 /* inverted dropout on v; element id = b1*drop_sb1 + b2*drop_sb2 + m*drop_sm + n */
  int64_t drop_sb1, drop_sb2, drop_sm;            /* (all 0 -> id = (batch*M + m)*N + n) */
  const uint64_t* seed_dev;                       /* optional device word added to seed (changes under graph replay) */
  float* colsum; int64_t colsum_sb2;              /* optional: colsum[b2*colsum_sb2 + n] += sum_m v (fp32 atomics; the bias
                                                     gradient of the layer whose dY this GEMM writes); not with split-K */
  int64_t bias_sb2;                               /* bias of batch entry (b1, b2) starts at bias + b1*bias_sb1 + b2*bias_sb2 (per-head bias slices) */
  int64_t colsum_sb1, bias_sb1;                   /* batch1 strides of colsum / bias (two weight sets in one launch: ABI 8) */
  float* split_ws; int64_t split_ws_elems;        /* optional workspace of >= bmhrl_gemm_splits() * batch1 * batch2 * M * N floats
                                                     (ABI 14): a K split then stores its partial tiles there and a second launch
                                                     adds them in split order -- C needs no zeroing, `accumulate` is allowed, and
                                                     the result is the same from run to run (fp32 atomics are not) */
} bmhrl_gemm_desc;

int bmhrl_gemm(const bmhrl_gemm_desc* d, bmhrl_stream_t stream);
/* n independent problems; up to four at a time run as ONE launch when they are 64 x 64-tile problems of the same operand
 * layout on the register-staged main loop (reductions that are no multiple of 64), any other mix one by one.  Same results
 * as n calls of bmhrl_gemm.  Meant for leaf products (the caption-side weight gradients of a fusion layer's backward). */
int bmhrl_gemm_group(const bmhrl_gemm_desc* descs, int32_t n, bmhrl_stream_t stream);
/* K splits bmhrl_gemm uses for a plain fp32 output of (M, N) over a reduction of K with allow_split_k set and `batch` =
 * batch1 * batch2 (the weight-gradient products): 1 = every element of C is stored exactly once, so C may be uninitialised
 * memory; > 1 = fp32 atomics into a C the caller must have zeroed.  Same decision function as the launcher's.  < 0: bad
 * arguments. */
int bmhrl_gemm_splits(int32_t M, int32_t N, int32_t K, int32_t batch);
/* What bmhrl_gemm would launch for *d (ABI 18): the launcher's own decision, a pure host function that dereferences no
 * pointer (only their alignment is read).  0 and plan[] filled, or < 0 where bmhrl_gemm would refuse the descriptor.
 *   plan[0] main loop     0 register-staged (gemm_kernel: K % 64 != 0, M < 8 or N < 8), 1 direct-to-LDS, 2 direct-to-LDS 8-wave
 *   plan[1] tile          0 64 x 64, 1 128 x 128, 2 128 x 64
 *   plan[2] LDS stages    2 (register-staged: its two buffers), 2 or 4 (direct-to-LDS), 3 (8-wave)
 *   plan[3] K splits      1 = none
 *   plan[4] split form    0 none, 1 fp32 atomics into C, 2 ordered (partial tiles in split_ws + a reduction pass)
 *   plan[5] epilogue path 0 fast bf16, 1 fast softmax (PROB / DSCORE), 2 generic (also every K split's partial tiles; its
 *                         interior tiles may take the specialised fp32 loop: bmhrl_gemm_f32_fast_path)
 *   plan[6] vec_ok        1: the generic path uses 16-byte accesses away from the right edge, 0: scalar accesses throughout
 *   plan[7] colsum pass   1: the column sums are a second, ordered pass (BMHRL_DETERMINISTIC=1), 0: atomics or none
 * Padding of the operands (columns K .. lda, or M / N .. lda when transposed) and gaps between batch entries may hold any
 * value, NaN included: no element outside the operands' logical extent reaches a stored output. */
int bmhrl_gemm_plan(const bmhrl_gemm_desc* d, int32_t plan[8]);
/* 1 when the interior tiles of *d's output leave through the specialised fp32 epilogue (plan[5] reports such a launch as
 * generic: tiles on the M / N edge do take the generic loop, and the two agree bit for bit), 0 when every tile takes the path
 * plan[5] names, < 0 for a refused descriptor.  It serves LINEAR products with an fp32 output, no K split, no mask / aux /
 * row vectors / relu / column sums, every base and leading dimension aligned for vector accesses (plan[6]), in one of these
 * forms: plain (+ bias), accumulate, (bias +) residual, (bias +) dropout + residual, the last also with a bf16 twin.
 * BMHRL_GEMM_FAST_F32=0 in the environment (read once) turns it off.  Pure host function, as bmhrl_gemm_plan. */
int bmhrl_gemm_f32_fast_path(const bmhrl_gemm_desc* d);
/* bmhrl_gemm_group's decision for descs[0 .. n): the number of gemm_group_kernel launches it makes (per four problems: 1 when
 * they share one launch, 0 when they run one by one), < 0 for a refused descriptor. */
int bmhrl_gemm_group_plan(const bmhrl_gemm_desc* descs, int32_t n);

/* ---------------------------------------------------------------------------------------------
 * Fused scaled-dot-product attention forward (flash style, S x S never materialised).
 * Replaces attention() + the head split/merge views, model/multihead_attention.py:7-31,75-86:
 *   O[b,q,h,:] = softmax_k( Q[b,q,h,:].K[b,k,h,:] * scale ; mask==0 -> -1e9 ) . V[b,k,h,:]
 * Q,K,V,O are bf16 (B, S, H*DK) row-major with leading dims ldq/ldk/ldv/ldo (heads are column
 * slices, exactly the .view(B,-1,H,d_k) of the reference; base pointers 16-byte aligned, leading
 * dims multiples of 8 elements).  DK must be 256 (the reference's d_model 1024 / H 4).  mask: bytes, mask[b*mask_sb + q*mask_sq + k], mask_sq = 0 for key-padding
 * masks (B,1,Sk).  row_max / row_sum (B,H,Sq) fp32 = softmax statistics of the masked scaled scores, kept
 * separately (not as one log-sum-exp) so that fully masked rows (all scores -1e9) stay exact in backward.
 * dropout_p > 0 applies the reference's dropout on the attention OUTPUT (:27-28).
 * ------------------------------------------------------------------------------------------- */
int bmhrl_attention_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                        void* O, int64_t ldo, float* row_max, float* row_sum, const uint8_t* mask, int64_t mask_sb,
                        int64_t mask_sq,
                        int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t DK, float scale,
                        float dropout_p, uint64_t seed, const uint64_t* seed_dev, bmhrl_stream_t stream);

/* The same attention in the absorbed-projection form for keys / values that are 128 wide before their projection (the
 * audio stream): scores_h = scale * Qp_h X^T with Qp_h = Q_h Wk_h (B,Sq,H,128), context_h = softmax(scores_h) X --
 * X (B,Sk,128) serves every head as keys and values; Q_h K_h^T differs from Qp_h X^T only by a per-row constant, and
 * P_h V_h = context_h Wv_h^T + bv_h (model/multihead_attention.py:7-31 with K = X Wk^T + bk, V = X Wv^T + bv).
 * ctx (B,Sq,H,128) bf16, normalised, no dropout (it applies after the Wv projection).  mask: (B,Sk) bytes or NULL.
 * row_max / row_sum as bmhrl_attention_fwd.  (Both attention entry points accept Sk up to 10 112.) */
int bmhrl_attention_shared128_fwd(const void* Qp, int64_t ldq, const void* X, int64_t ldx, void* ctx, int64_t ldo,
                                  float* row_max, float* row_sum, const uint8_t* mask, int64_t mask_sb,
                                  int32_t B, int32_t H, int32_t Sq, int32_t Sk, float scale, bmhrl_stream_t stream);

/* IEEE-half (fp16) operand variants of the two forward entry points: Q / K / V / X / Qp in, O / ctx out are _Float16 instead
 * of bfloat16 (v_mfma_f32_32x32x16_f16; scores, softmax statistics and accumulation stay fp32); every other argument as
 * above.  BASELINE configs[4] names "fp16/bf16 MFMA cross-attention"; the training path of this package uses bf16. */
int bmhrl_attention_fwd_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                            void* O, int64_t ldo, float* row_max, float* row_sum, const uint8_t* mask, int64_t mask_sb,
                            int64_t mask_sq, int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t DK, float scale,
                            float dropout_p, uint64_t seed, const uint64_t* seed_dev, bmhrl_stream_t stream);
int bmhrl_attention_shared128_fwd_f16(const void* Qp, int64_t ldq, const void* X, int64_t ldx, void* ctx, int64_t ldo,
                                      float* row_max, float* row_sum, const uint8_t* mask, int64_t mask_sb,
                                      int32_t B, int32_t H, int32_t Sq, int32_t Sk, float scale, bmhrl_stream_t stream);

/* Fused backward of bmhrl_attention_shared128_fwd (autograd of attention(), model/multihead_attention.py:7-31, in the
 * absorbed-projection form): given dCx (B,Sq,H,128) bf16, the forward's statistics and delta[b,h,q] = sum_d dCx*Cx
 * (bmhrl_attn_delta), writes dQp (B,Sq,H,128) bf16 and -- when dX != NULL -- dX (B,Sk,128) fp32 (leading dim lddx; += when
 * accumulate_dx) = sum over heads of P_h^T dCx_h + dS_h^T Qp_h.  P and dS are recomputed per tile from the statistics and
 * never written to memory; masked keys get no score gradient (masked_fill); deterministic (no atomics).  workspace:
 * bmhrl_attention_shared128_bwd_workspace(B,H,Sk) fp32 elements (the per-head partials of dX), uninitialised is fine. */
int64_t bmhrl_attention_shared128_bwd_workspace(int32_t B, int32_t H, int32_t Sk);
int bmhrl_attention_shared128_bwd(const void* Qp, int64_t ldq, const void* X, int64_t ldx, const void* dCx, int64_t lddo,
                                  const float* row_max, const float* row_sum, const float* delta, const uint8_t* mask,
                                  int64_t mask_sb, void* dQp, int64_t lddq, float* dX, int64_t lddx, int32_t accumulate_dx,
                                  float* workspace, int32_t B, int32_t H, int32_t Sq, int32_t Sk, float scale,
                                  bmhrl_stream_t stream);

/* Largest Sk the fused attention kernels accept (their key-mask ballots live in LDS); longer memories take the materialised
 * GEMM path of the host code. */
int bmhrl_attention_max_keys(void);

/* Tuning aid: pin the (query blocks x key splits) shape of the attention workgroups -- head_dim 256 or 128; code = 10 * QW + KW
 * (41: 4 x 1, 22: 2 x 2; head_dim 256 also 256: the two-phase exact-softmax kernel for at most 256 keys, which the automatic
 * choice takes when the grid fills the chip; head_dim 128 also 24: 2 x 4 and 14: the r04 form in which one wave carries two heads over four key
 * splits; a shape it does not serve -- an odd head count -- is refused while it is pinned), 0 = automatic (the default).  Process-wide, not
 * thread-safe; results do not depend on it beyond bf16 rounding of P. */
int bmhrl_attention_config(int32_t head_dim, int32_t code);

/* Which kernel an attention entry would launch for a shape under the current bmhrl_attention_config pin (pure host query, no
 * launch; the entries take their automatic choices through the same functions).  kind 0: bmhrl_attention_fwd (256, 41 or
 * 22); kind 1: bmhrl_attention_shared128_fwd (14, 41, 22 or 24); kind 2: bmhrl_attention_shared128_bwd (41: the wide dQp
 * kernel, 22: the narrow one; it has no pin).  mask_sq as passed to the entry (0: key mask or none).  < 0 for a shape the
 * entry refuses (Sk above bmhrl_attention_max_keys, a pinned 14 with an odd head count, ...).  The fp16 entries have no pin:
 * they take what this reports with the pin at 0, except that they have no two-phase kernel (41 or 22 in place of 256). */
int bmhrl_attention_plan(int32_t kind, int32_t B, int32_t H, int32_t Sq, int32_t Sk, int64_t mask_sq);

/* Attention core of SHORT sequences (Sq, Sk <= 32; d_k in {64, 128, 256, 512}) as one launch per direction: the caption
 * self attention of the fusion layers and the worker's goal attention (model/multihead_attention.py:7-31 on the 30 caption
 * positions).  Q / K / V / O / dO / dQ / dK / dV are bf16 row-major matrices whose row b * S + i holds the heads side by side
 * (head h at columns [h * d_k, (h + 1) * d_k) of the given pointer), P is bf16 (B, H, Sq, ldp) with ldp = Sk rounded up to 8
 * (padding columns written as zero) -- the probabilities the backward needs.  mask: bytes, mask[b * mask_sb + q * mask_sq +
 * key] == 0 -> the score is the reference's -1e9 fill (mask_sq = 0: one key mask per batch row); dropout on the OUTPUT with
 * element id (b * Sq + q) * H * d_k + h * d_k + d, like the context GEMM's epilogue it replaces.  Backward: dO is the gradient
 * of the pre-dropout output; the row term of the softmax is sum_k P dP from the same rounded P; masked keys get no score
 * gradient; dbq / dbk / dbv (optional, fp32 (H * d_k)) receive the column sums of dQ / dK / dV by atomic adds.
 * bmhrl_small_attention_ok: 1 when the shape is served. */
int bmhrl_small_attention_ok(int32_t Sq, int32_t Sk, int32_t dk);
int bmhrl_small_attention_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                              int64_t ldo, void* P, int32_t ldp, const uint8_t* mask, int64_t mask_sb, int64_t mask_sq,
                              int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t dk, float scale, float dropout_p,
                              uint64_t seed, const uint64_t* seed_dev, bmhrl_stream_t stream);
int bmhrl_small_attention_bwd(const void* dO, int64_t lddo, const void* P, int32_t ldp, const void* Q, int64_t ldq,
                              const void* K, int64_t ldk, const void* V, int64_t ldv, void* dQ, int64_t lddq, void* dK,
                              int64_t lddk, void* dV, int64_t lddv, float* dbq, float* dbk, float* dbv, const uint8_t* mask,
                              int64_t mask_sb, int64_t mask_sq, int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t dk,
                              float scale, bmhrl_stream_t stream);

/* Row softmax of materialised scores (small-Sq path: caption self/cross attention, goal attention).
 * S fp32 (rows, lds) -> P bf16 (rows, ldp), cols valid columns; also writes nothing else. */
/* Few-query attention over a long memory in the absorbed-projection form (functional.PairMemAttnFn; model/bm_hrl_agent.py:
 * 87-101): L <= 32 queries of a (sample, head) against Sk <= 896 memory rows of width dm (multiple of 32, <= 1024), keys =
 * values = the memory rows.  One launch per direction instead of GEMM + row kernel + GEMM:
 *   forward  (backward = 0): P = softmax(scale X mem^T, -1e9 at masked keys) -> PD slot 0; Y = P mem          (X = Q', Y = context)
 *   backward (backward = 1): dS = scale P (X mem^T - rowsum(P X mem^T)), 0 at masked keys -> PD slot 1; Y = dS mem (X = d context, Y = dQ')
 * X / Y: bf16, row (b2 * L + q) * ld + h * dm; mem: bf16 (n_mem, Sk, dm) row-major, sample b2 reads memory b2 % n_mem; mem_t:
 * the same memory transposed per sample, (n_mem, dm, ldt) with the columns [Sk, ldt) zero and ldt >= Sk rounded up to 16
 * (bmhrl_cast_memory writes both from the fp32 memory in one pass); PD: bf16, element (b2 * L + q) * pd_row + slot * pd_slot +
 * h * pad8(Sk) + key; mask: bytes, b2 * mask_sb + key.  bmhrl_memory_attention_ok: 1 when the shape is served. */
int bmhrl_memory_attention_ok(int32_t L, int32_t Sk, int32_t dm);
int bmhrl_cast_memory(const float* x, void* y, void* y_t, int32_t B, int32_t Sk, int32_t dm, int32_t ldt, bmhrl_stream_t stream);
int bmhrl_memory_attention(int32_t backward, const void* X, int64_t ldx, const void* mem, int64_t mem_sb, const void* mem_t,
                           int64_t mem_t_sb, int32_t ldt, void* PD, int64_t pd_row, int64_t pd_slot, void* Y, int64_t ldy,
                           const uint8_t* mask, int64_t mask_sb, int32_t n_mem, int32_t B2, int32_t H, int32_t L, int32_t Sk,
                           int32_t dm, float scale, bmhrl_stream_t stream);

/* rows_per_group > 0: the bf16 rows (P here; P and dS in the backward) are laid out in groups of rows_per_group consecutive
 * rows, group g starting g * group_stride elements into the buffer (0: plain rows with the leading dimension) */
int bmhrl_softmax_rows(const float* S, int64_t lds, void* P, int64_t ldp, int64_t rows, int32_t cols, int32_t rows_per_group,
                       int64_t group_stride, bmhrl_stream_t stream);

/* Backward of the same row softmax (autograd of F.softmax + masked_fill in attention(), model/multihead_attention.py:22-25):
 * dS[r][c] = scale * P[r][c] * (dP[r][c] - sum_k P[r][k] dP[r][k]), 0 where the key is masked; P bf16 (rows, ldp), dP fp32
 * (rows, lddp) -> dS bf16.  Rows are ordered (sample, query, rows_per_query) with `queries` queries per sample; mask (optional)
 * is addressed mask[sample * mask_sb + query * mask_sq + c] (0 = masked). */
int bmhrl_softmax_bwd_rows(const void* P, int64_t ldp, const float* dP, int64_t lddp, void* dS, int64_t ldds,
                           int64_t rows, int32_t cols, float scale, const uint8_t* mask, int64_t mask_sb, int64_t mask_sq,
                           int32_t rows_per_query, int32_t queries, int32_t rows_per_group, int64_t group_stride,
                           bmhrl_stream_t stream);

/* Softmax part of the backward of the head-dimension-256 attentions with at most 256 keys (video self attention, A<-V cross
 * attention: autograd of attention(), model/multihead_attention.py:7-31, called at model/bm_hrl_agent.py:358-377) in ONE
 * launch: P = exp(masked scaled scores - row_max) / row_sum from the forward's statistics, dP = dO V^T,
 * delta = sum_k P dP, dS = P (dP - delta) scale (0 at masked keys: no gradient through masked_fill).  Q, K, V, dO are bf16
 * rows with head h at columns [h*256, h*256+256) (leading dims in elements); mask: key mask (B, Sk) bytes or NULL;
 * P and dS: bf16 (B, H, Sq, ldp), ldp = pad8(Sk), padding columns written as 0.  Replaces bmhrl_attn_delta + the PROB and
 * DSCORE GEMM epilogues of bmhrl_gemm for these shapes.  _ok: 1 when the shape is served (dk == 256, Sk <= 256, key mask). */
int bmhrl_attention_bwd_scores256_ok(int32_t Sq, int32_t Sk, int32_t dk, int64_t mask_sq);
int bmhrl_attention_bwd_scores256(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                  const void* dO, int64_t lddo, const float* row_max, const float* row_sum,
                                  const uint8_t* mask, int64_t mask_sb, void* P, void* dS, int64_t ldp, int32_t B, int32_t H,
                                  int32_t Sq, int32_t Sk, float scale, bmhrl_stream_t stream);

/* delta[b,h,q] = scale * sum_d dO[b,q,h,d] * O[b,q,h,d]   (softmax backward row term) */
int bmhrl_attn_delta(const void* dO, int64_t lddo, const void* O, int64_t ldo, float* delta, float scale,
                     int32_t B, int32_t H, int32_t Sq, int32_t DK, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm (eps 1e-5, affine) -- nn.LayerNorm inside ResidualConnection, model/blocks.py:132,138,
 * and normCA/normCV, model/bm_hrl_agent.py:68-69,107-108.
 *   fwd: x fp32 (rows, D) -> y bf16 (rows, ldy) and/or y32 fp32 (rows, D); saves mean, rstd.
 *   bwd: dx = [dx_add +] LN'(dy) ; dgamma/dbeta accumulated with fp32 atomics into zeroed buffers.
 * ------------------------------------------------------------------------------------------- */
int bmhrl_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16, int64_t ldy,
                        float* y_f32, float* mean, float* rstd, int64_t rows, int32_t D, bmhrl_stream_t stream);
int bmhrl_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                        float* dx, const float* dx_add /* optional: dx = dx_add + LN'(dy) */, float* dgamma,
                        float* dbeta, int64_t rows, int32_t D, bmhrl_stream_t stream);
/* Same result; the column sums go block partials -> `workspace` -> dgamma/dbeta instead of every block adding into
 * the same 2*D addresses.  workspace: bmhrl_layernorm_bwd_workspace(rows, D) floats, need not be initialised; with a
 * NULL / too small workspace the call is bmhrl_layernorm_bwd. */
int64_t bmhrl_layernorm_bwd_workspace(int64_t rows, int32_t D);
int bmhrl_layernorm_bwd_ws(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                           float* dx, const float* dx_add, float* dgamma, float* dbeta, int64_t rows, int32_t D,
                           float* workspace, int64_t workspace_floats, bmhrl_stream_t stream);

/* `groups` independent LayerNorms of rows_per_group rows each in one launch (the worker and the manager half of a paired
 * fusion block, model/bm_hrl_agent.py:523,528): x, y, mean, rstd, dy, dx are group-major ((groups * rows_per_group, .)),
 * gamma / beta / dgamma / dbeta are (groups, D).  Same arithmetic per row as bmhrl_layernorm_fwd / _bwd. */
int bmhrl_layernorm_fwd_groups(const float* x, const float* gamma, const float* beta, void* y_bf16, int64_t ldy, float* y_f32,
                               float* mean, float* rstd, int64_t rows_per_group, int32_t D, int32_t groups,
                               bmhrl_stream_t stream);
int bmhrl_layernorm_bwd_groups(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                               float* dx, const float* dx_add, float* dgamma, float* dbeta, int64_t rows_per_group, int32_t D,
                               int32_t groups, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Feature add + positional encoding (K1): out = a (+ b) + PE[s]  (epoch_loops/captioning_bmrl_loops.py:498,
 * model/blocks.py:105-112).  pe is the precomputed fp32 table (S_max, D).  Optional bf16 copy and dropout.
 * ------------------------------------------------------------------------------------------- */
int bmhrl_add_posenc(const float* a, const float* b, const float* pe, float* out, void* out_bf16, int64_t ldob,
                     int32_t B, int32_t S, int32_t D, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                     bmhrl_stream_t stream);

/* Embedding * sqrt(D) (+ second embedding mix) + PE : model/blocks.py:44-48, model/bm_hrl_agent.py:611-625,642.
 * emb_out (B,L,D) fp32 = un-positional-encoded embeddings (critic input); out = emb_out + PE. */
int bmhrl_embed_posenc(const int64_t* tok, const int64_t* tok2, float mix, const float* table, const float* pe,
                       float* emb_out, float* out, int32_t B, int32_t L, int32_t D, float scale,
                       float dropout_p, uint64_t seed, const uint64_t* seed_dev, bmhrl_stream_t stream);
/* dTable[tok] += scale * (1-mix) * dC ; dTable[tok2] += scale * mix * dC  (fp32 atomics) */
int bmhrl_embed_bwd(const int64_t* tok, const int64_t* tok2, float mix, const float* dC, float* dtable,
                    int32_t B, int32_t L, int32_t D, float scale, bmhrl_stream_t stream);

/* fp32 -> bf16 cast of a (rows, cols) matrix into a padded-leading-dimension buffer, with optional scale
 * and inverted dropout (regenerates the forward mask from seed: element id = row*cols + col). */
int bmhrl_cast_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int32_t cols, float scale,
                    float dropout_p, uint64_t seed, const uint64_t* seed_dev, bmhrl_stream_t stream);

/* Split operand of a GEMM that needs more than bf16's 8 mantissa bits (the vocabulary projection feeding log_softmax,
 * model/bm_hrl_agent.py:463-466,483-484): hi = bf16(x), lo = bf16(x - hi); y gets three column blocks of width `part`:
 * block 0 = hi, block lo_slot (1 or 2) = lo, the other block = hi.  Activations use lo_slot 2, weights lo_slot 1, so that one
 * GEMM with K = 3 * part yields x_hi W_hi + x_hi W_lo + x_lo W_hi.  Padding columns (cols .. part) are not written. */
/* x2 (optional): a second source whose cols2 columns follow x's cols in every block (the concatenated operand of the
 * vocabulary head, cat[x, goal completion], in one launch) */
int bmhrl_cast_split3_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t part, int32_t lo_slot, int64_t rows,
                           int32_t cols, const float* x2, int64_t ldx2, int32_t cols2, bmhrl_stream_t stream);

/* bmhrl_cast_bf16 + column sums of the rounded result in one pass: colsum[n] += sum_m y[m][n] (fp32 atomics; colsum is
 * accumulated into, the caller zeroes it).  dY cast and bias gradient of one layer -- nn.Linear's db of
 * model/multihead_attention.py:53-56 / model/blocks.py:181-182 under autograd. */
int bmhrl_cast_colsum_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int32_t cols, float scale,
                           float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* colsum, bmhrl_stream_t stream);
/* the same over `rows / group_rows` row groups, group g adding into colsum + g * colsum_stride (the dY of two layers in one
 * buffer); rows % group_rows == 0.  Dropout element ids run over all rows, as in the one-group call. */
int bmhrl_cast_colsum_bf16_groups(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int32_t cols, float scale,
                                  float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* colsum,
                                  int64_t group_rows, int64_t colsum_stride, bmhrl_stream_t stream);

/* One launch for many casts: the per-step refresh of every bf16 weight shadow / concatenated bias (what the reference
 * gets for free by computing in fp32: model/multihead_attention.py:53-56, model/blocks.py:181-182 hold fp32 weights).
 * `segments` (device memory) holds 6 int64 per segment: source address (fp32), destination address, rows, cols,
 * destination leading dimension in elements (bf16 destination) or <= 0 (fp32 destination, packed), and the index of the
 * segment's first block; a block covers 4096 consecutive elements, n_blocks = sum over segments of
 * ceil(rows*cols / 4096). */
int bmhrl_cast_segments(const int64_t* segments, int32_t n_segments, int32_t n_blocks, bmhrl_stream_t stream);

/* db[n] (+)= sum_m dY[m][n]  (bias gradient of nn.Linear), dY bf16 */
int bmhrl_colsum_bf16(const void* dY, int64_t ld, float* db, int32_t accumulate, int64_t rows, int32_t cols,
                      bmhrl_stream_t stream);
/* the same for `groups` row groups laid out back to back ((groups * rows_per_group, ld)); the sums of group g are ADDED at
 * db + g * db_stride (zero them first).  One launch. */
int bmhrl_colsum_bf16_groups(const void* dY, int64_t ld, float* db, int64_t rows_per_group, int32_t cols, int32_t groups,
                             int64_t db_stride, bmhrl_stream_t stream);
/* y[c] = bf16(x) for c in [0, copies): copy c starts copy_stride elements after copy c - 1 (no scale, no dropout) */
int bmhrl_cast_bf16_copies(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int32_t cols, int32_t copies,
                           int64_t copy_stride, bmhrl_stream_t stream);

/* Fusion gate (K7): out = g*Cv + (1-g)*Ca, g = sigmoid(clamp(a,-2,2)), model/bm_hrl_agent.py:111-114 */
int bmhrl_gate_fwd(const float* cv, const float* ca, const float* a_v, float* out, void* out_bf16, int64_t ldob,
                   int64_t rows, int32_t D, bmhrl_stream_t stream);
int bmhrl_gate_bwd(const float* dout, const float* cv, const float* ca, const float* a_v, float* dcv, float* dca,
                   float* da_v /* atomic += */, int64_t rows, int32_t D, bmhrl_stream_t stream);

/* The tail of a BMFusionLayer in one launch (model/bm_hrl_agent.py:107-114): out = g * normCV(cv) + (1 - g) * normCA(ca),
 * g = sigmoid(clamp(a_v, -2, 2)); rows are n_groups (1 or 2) groups of rows_per_group rows, group i with its own parameters
 * (the worker and the manager stack advance together).  stats: (4, rows) fp32 out = mean / rstd of ca, mean / rstd of cv.
 * bwd: dca / dcv (rows, D); the parameter gradients are ADDED (fp32 atomics) into the group's d* pointers (NULL: skipped),
 * which the caller zeroes.  D <= 512. */
typedef struct bmhrl_fusion_tail_params {
  const float* gamma_ca; const float* beta_ca; const float* gamma_cv; const float* beta_cv; const float* a_v;
  float* dgamma_ca; float* dbeta_ca; float* dgamma_cv; float* dbeta_cv; float* da_v;          /* backward only */
} bmhrl_fusion_tail_params;
/* out_bf16 (optional, row stride ldob >= D): the result in bf16 as well -- the operand of the blocks that consume it */
int bmhrl_fusion_tail_fwd(const float* ca, const float* cv, const bmhrl_fusion_tail_params* groups, int32_t n_groups,
                          int64_t rows_per_group, int32_t D, float* out, float* stats, void* out_bf16, int64_t ldob,
                          bmhrl_stream_t stream);
/* dout: the incoming gradient of group 0 (row stride ldd0, <= 0: D); dout1: of group 1 (row stride ldd1; NULL: the rows
 * behind group 0's in the same tensor) -- the two stacks' outputs are consumed by different heads */
int bmhrl_fusion_tail_bwd(const float* dout, const float* dout1, int64_t ldd0, int64_t ldd1, const float* ca, const float* cv,
                          const float* stats, const bmhrl_fusion_tail_params* groups, int32_t n_groups, int64_t rows_per_group,
                          int32_t D, float* dca, float* dcv, bmhrl_stream_t stream);

/* Manager.expand_goals (K8), model/bm_hrl_agent.py:415-429: src[row] = row of goals_in copied to (b,l), or -1 = zero.
 * bmhrl_expand_goals_index builds the (B*L) int32 source map from the segment labels with the reference's
 * row-transition quirks; fwd is a gather, bwd a scatter-add. */
int bmhrl_expand_goals_index(const int32_t* seg, int32_t* src, int32_t B, int32_t L, bmhrl_stream_t stream);
/* bmhrl_expand_goals_index + bmhrl_gather_rows as one launch (Manager.expand_goals, model/bm_hrl_agent.py:415-429): out[b, l] =
 * x[src[b, l]] (0 where src = -1), `src` is written for the backward's scatter; out_bf16: optional bf16 copy.  L <= 1024. */
int bmhrl_expand_goals(const int32_t* seg, const float* x, int32_t* src, float* out, void* out_bf16, int64_t ldob, int32_t B,
                       int32_t L, int32_t D, bmhrl_stream_t stream);
/* The same with the manager's exploration noise (Manager.forward, model/bm_hrl_agent.py:444-452; on after the constructor and
 * left on by teach_warmstart / teach_manager, :572-589): ONE (D,) vector noise[c] = z_c * std' + 0.5 * mean', z ~ N(0, 1),
 * mean' = nanmean(x) / mean_factor, std' = sqrt(nanmean(|x - nanmean(x)|^2)) / std_factor over all B*L*D entries of x, added
 * to every goal before the segment copy (rows the copy zeroes stay zero).  z comes from the library's counter RNG over
 * (seed + seed_dev[0], column): reproducible, and it changes between replays of a captured step.  noise_out: optional (D,)
 * copy of the vector.  The noise is detached in the reference, so the backward is the plain scatter along `src`.
 * B*L*D < 2^24, D <= 1024. */
int bmhrl_expand_goals_explore(const int32_t* seg, const float* x, int32_t* src, float* out, void* out_bf16, int64_t ldob,
                               int32_t B, int32_t L, int32_t D, float mean_factor, float std_factor, uint64_t seed,
                               const uint64_t* seed_dev, float* noise_out, bmhrl_stream_t stream);
int bmhrl_gather_rows(const float* x, const int32_t* src, float* out, void* out_bf16, int64_t ldob, int64_t rows,
                      int32_t D, bmhrl_stream_t stream);
/* backward of the gather along a row map of bmhrl_expand_goals[_index]: dx[s] = sum of dout[r] over src[r] == s, every row of dx
 * written.  The map's structure is used (a run of consecutive rows points at its LAST row, other rows at themselves or at -1):
 * the sum runs in row order, no atomics -- the manager's goal gradient is the same from run to run.
 * dx, the contract: callers pass a ZEROED (rows, D) buffer and a map whose entries are -1 or in [0, rows).  The two modes differ
 * in what they do with dx, and a zeroed buffer is the one input on which they agree:
 *   default:               every element of dx is OVERWRITTEN (rows that nothing points at get 0); only the row maps of
 *                          bmhrl_expand_goals[_index] are summed correctly -- a general map is not supported;
 *   BMHRL_DETERMINISTIC=1: one thread per column walks the rows in order and ACCUMULATES into dx (dx[src[r]] += dout[r]); any
 *                          map is handled, and whatever dx held before stays in the sum. */
int bmhrl_scatter_add_rows(const float* dout, const int32_t* src, float* dx, int64_t rows, int32_t D,
                           bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-token loss step (K9-K11): log-softmax over the vocabulary fused with the loss.
 *  bmhrl_log_softmax:   logits fp32 (rows, V) -> log-probs in place (WorkerCore, model/bm_hrl_agent.py:463-466)
 *  bmhrl_smooth_kl_fwd: per-row sum of LabelSmoothing (biased_trg == NULL; loss/label_smoothing.py:12-32) or
 *                       BiasedKL (loss/biased_kl.py:22-53) over the unreduced (rows, V) divergence, never
 *                       materialising the target distribution; amp = clamp(score*p(a)*n_row, 0, 1) is computed
 *                       here (epoch_loops/captioning_bmrl_loops.py:285,321-322,409-416).
 *  bmhrl_smooth_kl_bwd: d(loss_scale * sum)/d logits (wrt_logits = 1, log-softmax folded in) or /d log-probs
 *                       (wrt_logits = 0) -> bf16 (rows, ldg) and/or fp32 (rows, V), incl. the path through amp.
 *  bmhrl_log_softmax_bwd: dlogits = dlogp - exp(logp) * rowsum(dlogp) -> bf16 (rows, ldg)
 *  zero_pad_rows: the reference's `idx.sum() > 0` guard: 1/0 forces it, -1 lets the kernel evaluate it on the device.
 *  n_row == NULL with biased_trg given: `score` IS the amplitude, an argument of BiasedKL.forward and not a function of the
 *                       log-probs (clamped to [0, 1] all the same): bmhrl_smooth_kl_bwd then has no path through it.
 * ------------------------------------------------------------------------------------------- */
int bmhrl_log_softmax(float* logits, int64_t ld, int64_t rows, int32_t V, bmhrl_stream_t stream);
int bmhrl_smooth_kl_fwd(const float* logp, int64_t ld, const int64_t* trg, const int64_t* biased_trg,
                        const float* score, const float* n_row, float smoothing, int32_t pad_idx,
                        int32_t zero_pad_rows, float* row_loss, float* amp_out, int64_t rows, int32_t V,
                        bmhrl_stream_t stream);
/* the unreduced divergence itself, (rows, V) fp32 -- the reference criteria's return value (callers that inspect entries) */
int bmhrl_smooth_kl_full(const float* logp, int64_t ld, const int64_t* trg, const int64_t* biased_trg, const float* score,
                         const float* n_row, float smoothing, int32_t pad_idx, int32_t zero_pad_rows, float* out,
                         int64_t rows, int32_t V, bmhrl_stream_t stream);
int bmhrl_smooth_kl_bwd(const float* logp, int64_t ld, const int64_t* trg, const int64_t* biased_trg,
                        const float* score, const float* n_row, float smoothing, int32_t pad_idx,
                        int32_t zero_pad_rows, const float* loss_scale /* device scalar */,
                        const float* loss_scale2 /* second device scalar multiplied in (the incoming d loss), or NULL */,
                        int32_t wrt_logits, void* grad_bf16, int64_t ldg, float* grad_f32, int64_t rows, int32_t V,
                        bmhrl_stream_t stream);
/* The loops' reduction of the row sums: loss = weight * sum(row_loss) / (n_tokens * factor), n_tokens = #(trg != pad_idx)
 * (epoch_loops/captioning_bmrl_loops.py:1156-1158: factor 1; :829-833,846-862: factor 4/20); scale = weight / (n_tokens *
 * factor) is what bmhrl_smooth_kl_bwd takes as loss_scale.  weight: optional device scalar (data-parallel token weight). */
int bmhrl_token_loss_reduce(const float* row_loss, const int64_t* trg, int64_t rows, int64_t pad_idx, const float* weight,
                            float factor, float* loss, float* scale, bmhrl_stream_t stream);
/* The warmstart loss tail as one launch (r03): log_softmax in place over `logits` (model/bm_hrl_agent.py:463-466), the
 * LabelSmoothing row sums (loss/label_smoothing.py:12-32), loss_scale[0] = weight * sum(rows) / (n_tokens * factor) and
 * loss_scale[1] = weight / (n_tokens * factor) (epoch_loops/captioning_bmrl_loops.py:1156-1158), and d loss / d logits as
 * bf16 (loss.backward() of the loops, through the log-softmax) for the gradient `dloss` (device scalar or NULL = 1) the
 * caller will pass to backward.  V % 4 == 0, V <= 12288.  `counter`: four zero-initialised 32-bit words (8-byte aligned)
 * the kernel re-arms: the rows are summed as 2^-32 fixed point with integer atomics (order independent: deterministic), the
 * block that arrives last writes loss_scale.  Same values as bmhrl_log_softmax + bmhrl_smooth_kl_fwd +
 * bmhrl_token_loss_reduce + bmhrl_smooth_kl_bwd(wrt_logits) up to the rounding of the loss's sums. */
int bmhrl_head_loss(float* logits, int64_t ld, const int64_t* trg, float smoothing, int32_t pad_idx, const float* weight,
                    float factor, const float* dloss, float* row_loss, float* loss_scale, void* dlogits_bf16, int64_t ldg,
                    uint32_t* counter, int64_t rows, int32_t V, bmhrl_stream_t stream);
int bmhrl_log_softmax_bwd(const float* dlogp, const float* logp, int64_t ld, void* dlogits_bf16, int64_t ldg,
                          int64_t rows, int32_t V, bmhrl_stream_t stream);
/* out[row] = d rowloss / d log(raw amplitude) (0 where clamp(., 0, 1) is active): the share of the gradient that reaches the
 * row through its amplitude.  Manager branch of biased_kl(), epoch_loops/captioning_bmrl_loops.py:299-317: the amplitude holds
 * the product of p(a) over a segment, so this also flows to the segment's other tokens (bmhrl_amd/functional.py ManagerKLFn).
 * With a given amplitude (n_row == NULL): out[row] = d rowloss / d amplitude, on the closed interval [0, 1] (GivenAmpKLFn). */
int bmhrl_smooth_kl_amp_grad(const float* logp, int64_t ld, const int64_t* trg, const int64_t* biased_trg, const float* score,
                             const float* n_row, float smoothing, int32_t pad_idx, int32_t zero_pad_rows, float* out,
                             int64_t rows, int32_t V, bmhrl_stream_t stream);
/* a ~ Categorical(exp(logp)) by inverse CDF with one uniform per row (counter RNG: seed (+ *seed_dev when given: a device
 * word advanced per step, so that a captured step draws fresh samples at every replay), row_offset + row -- row_offset = the
 * first row of this rank's share of the global batch, so that data-parallel ranks draw independent samples);
 * greedy != 0 -> argmax.  epoch_loops/captioning_bmrl_loops.py:283-284 */
int bmhrl_sample_tokens(const float* logp, int64_t ld, int64_t* out, float* p_out, int64_t rows, int32_t V,
                        int32_t greedy, uint64_t seed, const uint64_t* seed_dev, int64_t row_offset, bmhrl_stream_t stream);
/* Reinforce (loss/biased_kl.py:69-81): per-row terms of -adv*log(clamp(p(a), 1e-5, 1-1e-5)) and adv^2, adv = value -
 * critic_value; `pred` holds log-probs (is_logp = 1) or probabilities (0, the reference's input).  The backward
 * writes d(gscale * (mean(policy) + mean(value terms))) w.r.t. the (rows, V) probabilities, value and critic_value. */
int bmhrl_reinforce_fwd(const float* pred, int64_t ld, int32_t is_logp, const int64_t* action, const float* value,
                        const float* critic_value, float* row_policy, float* row_value, int64_t rows, int32_t V,
                        bmhrl_stream_t stream);
int bmhrl_reinforce_bwd(const float* probs, int64_t ld, const int64_t* action, const float* value,
                        const float* critic_value, const float* gscale /* device scalar */, float* dprobs, float* dvalue,
                        float* dcritic, int64_t rows, int32_t V, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Frozen segment critic (K15; SegmentCritic.forward, model/bm_hrl_agent.py:204-215), fp32 throughout because its
 * output is thresholded into integer segment labels (:638-640).
 *  bmhrl_gemm_f32   : C[M,N] = A[M,K] W[N,K]^T + bias1 + bias2 on the f32-input MFMA (input projections W_ih x + b)
 *  bmhrl_rnn_step   : one time step of one LSTM (gates = 4, order i,f,g,o) or GRU (gates = 3, order r,z,n) layer:
 *                     xproj (B*L, gates*H) row b*L + t, W_hh (gates*H, H), b_hh (GRU only), state ping-pong buffers
 *                     (B, H); writes h_t (optionally through AReLU, :13-23) to seq_out (B*L, H)
 *  bmhrl_critic_head: score = lin(x), labels = sigmoid(score) > threshold
 * ------------------------------------------------------------------------------------------- */
int bmhrl_gemm_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias1, const float* bias2,
                   float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, bmhrl_stream_t stream);
int bmhrl_rnn_step(int32_t gates, const float* xproj, const float* whh, const float* bhh, const float* h_prev,
                   const float* c_prev, float* h_out, float* c_out, float* seq_out, const float* arelu_alpha,
                   const float* arelu_beta, int32_t B, int32_t L, int32_t H, int32_t t, bmhrl_stream_t stream);
/* The whole recurrent stack as a wavefront over (layer, time): cell (l, t) runs in launch l + t (chunk = 1), so the stack takes
 * L + n_layers - 1 launches (all cells of a diagonal in one grid) instead of n_layers * (1 + L).  Layer l reads
 * in_seq (B, L, in_ld) -- the embeddings for l = 0, seq_out of layer l - 1 otherwise -- and writes seq_out (B, L, H)
 * (through AReLU when arelu_alpha / arelu_beta are given: the last layer of the LSTM and of the GRU stack,
 * model/bm_hrl_agent.py:209-213); h / c are two (B, H) state buffers each (c unused for the GRU).  fp32 throughout.
 * With chunk = T > 1 cell (l, t) runs in launch t + T*l (L + T*(n_layers-1) launches). */
typedef struct bmhrl_rnn_layer {
  const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh;   /* nn.LSTM / nn.GRU parameter layout */
  const float* in_seq; int64_t in_ld; int32_t in_dim; int32_t gates;            /* gates: 4 = LSTM (i,f,g,o), 3 = GRU (r,z,n) */
  float* seq_out; float* h[2]; float* c[2];
  const float* arelu_alpha; const float* arelu_beta;
  float* xproj;                                           /* (B, L, gates*H) scratch, needed when chunk > 1 */
} bmhrl_rnn_layer;
int bmhrl_rnn_wavefront(const bmhrl_rnn_layer* layers, int32_t n_layers, int32_t B, int32_t L, int32_t H,
                        int32_t chunk /* time steps a layer trails the one below: W_ih is read once per chunk; 1 = the
                                         plain diagonal, which runs the matrix-pipe cell (v_mfma_f32_16x16x4_f32) */,
                        bmhrl_stream_t stream);
int bmhrl_critic_head(const float* x, const float* w, const float* b, float threshold, float* score, int32_t* labels,
                      int64_t rows, int32_t H, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training the segment critic (csrc/critic_train.hip), fp32, zero initial state, every sum in a fixed order (no float
 * atomics: two runs agree bit for bit).  Sequence buffers have row b*L + t.
 *  bmhrl_rnn_step_train  : bmhrl_rnn_step's cell with the recurrent product on the f32 matrix pipe (k split over the waves);
 *                          keeps the raw h_t in h_seq (B*L, H), h_{t-1} in hprev_seq (B*L, H) (zero at t = 0; step t reads its
 *                          row t and writes row t + 1), c_t in c_seq (LSTM), the gate activations i,f,g,o / r,z,n in gate_seq
 *                          (B*L, gates*H), W_hn h_{t-1} + b_hn in hn_seq (GRU) and AReLU(h_t) in y_seq when arelu_alpha /
 *                          arelu_beta are given
 *  bmhrl_rnn_bwd_step    : backward of one cell, called with t descending from L - 1.  dy (B*L, H) is the gradient of the
 *                          layer's output sequence (of y_seq when the AReLU parameters are given).  The launch of step t forms
 *                          the carried dh = dA_h[t + 1] . W_hh (f32 matrix pipe, k split over the waves), runs the cell
 *                          equations and writes row t of dax / dah (B*L, gates*H; the LSTM has one buffer: dah is ignored) and
 *                          the element-wise carry (B, H) (LSTM dc . f, GRU dh . z; not read at t = L - 1)
 *  bmhrl_gemm_f32_nn     : C[M,N] = op(A) . B, B (K, N) row-major, A (M, K) row-major (K % 4 == 0) or, a_kmajor, (K, M)
 *                          row-major (any K): dX = dA_x . W_ih, dW_ih = dA_x^T . X, dW_hh = dA_h^T . H_prev (hprev_seq)
 *  bmhrl_rnn_bias_grad   : db_x = column sums of dax (rows, N); db_h of dah when given
 *  bmhrl_arelu_grad      : dbeta = sum dy relu(h) s(beta)(1 - s(beta)); dalpha = -sum dy relu(-h) for 0.01 <= alpha <= 0.99, else
 *                          0; partial: 128 floats of scratch
 *  bmhrl_critic_head_loss: one launch.  labels given: score = lin_w . y2 + lin_b, loss = sum mask l / sum mask with the
 *                          BCE-with-logits l of positive weight pos_weight, ds = d loss / d score; labels null: ds = ds_in.
 *                          Then dy2 = ds lin_w, dlin_w = sum ds y2, dlin_b = sum ds.  mask: one byte per row.
 * ------------------------------------------------------------------------------------------- */
int bmhrl_rnn_step_train(int32_t gates, const float* xproj, const float* whh, const float* bhh, float* h_seq, float* hprev_seq,
                         float* c_seq, float* gate_seq, float* hn_seq, float* y_seq, const float* arelu_alpha,
                         const float* arelu_beta, int32_t B, int32_t L, int32_t H, int32_t t, bmhrl_stream_t stream);
int bmhrl_rnn_bwd_step(int32_t gates, const float* whh, const float* dy, const float* h_seq, const float* c_seq,
                       const float* gate_seq, const float* hn_seq, float* carry, float* dax, float* dah,
                       const float* arelu_alpha, const float* arelu_beta, int32_t B, int32_t L, int32_t H, int32_t t,
                       bmhrl_stream_t stream);
int bmhrl_gemm_f32_nn(const float* A, int64_t lda, int32_t a_kmajor, const float* Bm, int64_t ldb, float* C, int64_t ldc,
                      int32_t M, int32_t N, int32_t K, bmhrl_stream_t stream);
int bmhrl_rnn_bias_grad(const float* dax, const float* dah, float* db_x, float* db_h, int64_t rows, int32_t N,
                        bmhrl_stream_t stream);
int bmhrl_arelu_grad(const float* dy, const float* h, const float* alpha, const float* beta, float* partial, float* dalpha,
                     float* dbeta, int64_t n, bmhrl_stream_t stream);
int bmhrl_critic_head_loss(const float* y2, const float* lin_w, const float* lin_b, const float* labels, const uint8_t* mask,
                           float pos_weight, const float* ds_in, float* score, float* loss, float* ds, float* dy2,
                           float* dlin_w, float* dlin_b, int64_t rows, int32_t H, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser (K14): torch.optim.Adam semantics (scripts/train_rl_captioning_module.py:81-83, default
 * betas/eps, L2 weight decay added to the gradient) over one flat fp32 bucket; grad_scale multiplies
 * the gradient first (1/world for data parallel averaging).
 * ------------------------------------------------------------------------------------------- */
int bmhrl_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int32_t step,
                    const int32_t* step_dev /* optional: step count read on the device (graph replay) */,
                    float grad_scale, bmhrl_stream_t stream);

/* The same update driven by a per-parameter table, writing each updated weight's bf16 shadow (or fp32 copy) in the same
 * pass.  segments: int64 (n_segments, 7) on the device = {offset of the parameter in the flat bucket (elements), shadow
 * address (0: none), rows, cols, shadow leading dimension in elements (<= 0: fp32 copy, tightly packed), first block,
 * address of the parameter's fp32 gradient (0: grad + offset, the flat bucket)};
 * a block owns 4096 consecutive elements of one parameter, n_blocks = sum over parameters of ceil(rows * cols / 4096). */
int bmhrl_adam_segments(const int64_t* segments, int32_t n_segments, int32_t n_blocks, float* param, const float* grad,
                        float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int32_t step, const int32_t* step_dev, float grad_scale, bmhrl_stream_t stream);

/* Hyper-parameter block of an optimizer (train.FlatAdam.hyper): 8 fp32 words in device memory, so that a captured step
 * follows a change of the learning rate or of the clip threshold without being captured again.
 *   [0] lr        [1] max_norm (clip threshold)        [2] coef (written by bmhrl_grad_norm; 1.0 when nothing clips)
 *   [3] norm (written by bmhrl_grad_norm)              [4..7] reserved, zero
 *
 * bmhrl_grad_norm: global L2 norm of the gradient that `segments` describes -- the table of bmhrl_adam_segments: word 6 is
 * the gradient's address, 0 = grad + offset; the shadow words are not read -- scaled by grad_scale, and the clip coefficient
 * of torch.nn.utils.clip_grad_norm_(norm_type = 2):
 *   hyper[3] = norm = sqrt(sum over every element of (g * grad_scale)^2)
 *   hyper[2] = coef = min(1, max_norm / (norm + 1e-6)) with max_norm = hyper[1], read on the device (the quotient formed as
 *              torch forms it, reciprocal(norm + 1e-6) * max_norm, in fp32); NaN when the norm is not finite.
 * Two launches in a fixed summation order (csrc/grad_norm.hip), no floating-point atomics: the two words are the same
 * bits in every run.  partials: fp32 workspace of partials_elems >= n_blocks elements, one per block. */
int bmhrl_grad_norm(const int64_t* segments, int32_t n_segments, int32_t n_blocks, const float* grad, float grad_scale,
                    float* partials, int64_t partials_elems, float* hyper, bmhrl_stream_t stream);

/* Gradient accumulation over a window of micro-batches (train.FlatAdam.accumulate), one launch per micro-batch over the
 * gradient that `segments` describes -- the table of bmhrl_adam_segments: word 0 the offset, words 2 x 3 the element count,
 * word 5 the first block, word 6 the gradient's address, 0 = grad + offset; words 1 and 4 are not read.
 * ctl: two fp32 words in device memory, read by the kernel (a captured micro-step serves every micro-batch of a window):
 *   ctl[0] = w, the weight of this micro-batch        ctl[1] != 0: the first micro-batch of a window
 *   first:      accum[offset + i] = w * g[i]          (a store: accum is not read, a NaN or Inf left there does not survive)
 *   otherwise:  accum[offset + i] = fma(w, g[i], accum[offset + i])
 * Elementwise, no sum across threads: the same bits in every run.  The padding between one parameter's end and the next
 * offset is never written.  loss_in / loss_out (optional, both or neither): loss_out[0] = (first ? 0 : loss_out[0]) +
 * w * loss_in[0], formed by the same launch. */
int bmhrl_accum_segments(const int64_t* segments, int32_t n_segments, int32_t n_blocks, const float* grad, float* accum,
                         const float* ctl, const float* loss_in, float* loss_out, bmhrl_stream_t stream);

/* bmhrl_adam_step / bmhrl_adam_segments with the learning rate and the clip coefficient read from the block: lr = hyper[0]
 * (the lr argument is not used) and the gradient is multiplied by the ONE fp32 factor grad_scale * hyper[2].  Bit-equal to
 * the entry point above called with that lr and that product as grad_scale. */
int bmhrl_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int32_t step, const int32_t* step_dev,
                        float grad_scale, const float* hyper, bmhrl_stream_t stream);
int bmhrl_adam_segments_dev(const int64_t* segments, int32_t n_segments, int32_t n_blocks, float* param, const float* grad,
                            float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int32_t step, const int32_t* step_dev, float grad_scale, const float* hyper,
                            bmhrl_stream_t stream);

/* The masks of a bimodal step in one launch (model/masking.py:18-55): v_mask[b][t] = rgb[b][t][0] != 0 (row stride ld_rgb
 * elements), a_mask likewise from audio, c_mask[b][i][j] = trg[b][j] != pad_idx && j <= i; bytes 0 / 1, each mask written
 * `copies` times back to back ((copies, B, .) layout). */
int bmhrl_make_masks(const float* rgb, int64_t ld_rgb, const float* audio, int64_t ld_aud, const int64_t* trg, int32_t B,
                     int32_t Tv, int32_t Ta, int32_t L, int64_t pad_idx, int32_t copies, uint8_t* v_mask, uint8_t* a_mask,
                     uint8_t* c_mask, bmhrl_stream_t stream);

/* Head of a training step in one launch (epoch_loops/captioning_bmrl_loops.py:487-508 feature_getter: the input / target
 * shift of the captions; model/masking.py:28-55: the masks built from the SHIFTED input): captions (B, L + 1) int64 with row
 * stride ld_cap -> trg_in = captions[:, :-1], trg_y = captions[:, 1:] (contiguous (B, L)), the three masks of
 * bmhrl_make_masks from trg_in, and the step's device counters advanced by one: bump64 (the dropout / sampling seed word)
 * and bump32[0..1] (Adam step counters); each may be NULL. */
int bmhrl_batch_head(const float* rgb, int64_t ld_rgb, const float* audio, int64_t ld_aud, const int64_t* captions,
                     int64_t ld_cap, int32_t B, int32_t Tv, int32_t Ta, int32_t L, int64_t pad_idx, int32_t copies,
                     uint8_t* v_mask, uint8_t* a_mask, uint8_t* c_mask, int64_t* trg_in, int64_t* trg_y, int64_t* bump64,
                     int32_t* bump32_a, int32_t* bump32_b, bmhrl_stream_t stream);

/* Library self-description: returns the gfx target the kernels were built for ("gfx950"). */
const char* bmhrl_hip_arch(void);
/* ---------------------------------------------------------------------------------------------
 * Conv1d(padding='same') + GroupNorm input projection of the DETR-mode agent (model/det_bmhrl_agent.py:79-86,169-174),
 * activations (B, T, C) row major.  The convolution itself is bmhrl_gemm over the unfolded operand:
 *   bmhrl_unfold1d_bf16: out[(b, t)][j*C + c] = x[b][t + j - left][c] (0 outside the clip), bf16; 'same' padding: left = (k-1)/2
 *   bmhrl_fold1d:        dx[b][t][c] = sum_j dU[(b, t - j + left)][j*C + c]      (the data gradient; ordered, no atomics)
 *   bmhrl_groupnorm_fwd / _bwd: nn.GroupNorm(G, C) over (T, C/G) per sample and group; mean / rstd (B*G) saved for the
 *   backward; dgamma / dbeta are ADDED to (zero them first).
 * ------------------------------------------------------------------------------------------- */
int bmhrl_unfold1d_bf16(const float* x, void* out, int64_t ldo, int32_t B, int32_t T, int32_t C, int32_t k, int32_t left,
                        bmhrl_stream_t stream);
int bmhrl_fold1d(const float* du, int64_t ldu, float* dx, int32_t B, int32_t T, int32_t C, int32_t k, int32_t left,
                 bmhrl_stream_t stream);
int bmhrl_groupnorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int32_t B,
                        int32_t T, int32_t C, int32_t G, float eps, bmhrl_stream_t stream);
int bmhrl_groupnorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                        float* dgamma, float* dbeta, int32_t B, int32_t T, int32_t C, int32_t G, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Beam-search caption decoding (bmhrl_amd/decode.py BeamDecoder: B samples x K beams, rows sample-major).  Both read the
 * step position t from a device word (a captured token step replays them unchanged).
 *  bmhrl_beam_select: per sample, the K best of the candidates (k, v) with score_k + logp[k][v] (live beam k) or (k, pad)
 *    with score_k (finished beam k), best first, ties to the smaller k*V + v.  Writes the new scores and finished flags
 *    (finished = parent finished or v == end_idx; the outputs may alias the inputs), the parent beam (0..K-1 within the
 *    sample), the next input token, hist[row][t + 1] (when t + 1 < hist_cols), and last_live[0] = t + 1 when any new
 *    beam is live.  1 <= K <= 16, K <= V.
 *  bmhrl_beam_reorder: for every table entry and every row j whose parent is not itself, exactly the first
 *    min(beam_bytes, (t + 1) * pos_bytes) bytes of row j (pos_bytes = 0: the whole row) take the parent row's: phase 0
 *    copies state[parent row] -> scratch[j], phase 1 scratch[j] -> state[j]; the rest of the row is not touched.
 *    n_blocks = sum over entries of rows * ceil(beam_bytes / 16384).
 * ------------------------------------------------------------------------------------------- */
typedef struct bmhrl_beam_buffer {
  void* state;          /* (rows, beam_bytes) per-beam buffer */
  void* scratch;        /* the same size: the gathered rows between the two phases */
  int64_t beam_bytes;   /* bytes per beam row */
  int64_t pos_bytes;    /* bytes per position of the row; 0: no position axis */
} bmhrl_beam_buffer;
int bmhrl_beam_select(const float* logp, int64_t ld, const float* scores_in, const uint8_t* finished_in, float* scores_out,
                      uint8_t* finished_out, int32_t* parent, int64_t* tok, int64_t* hist, int64_t ldh, int32_t hist_cols,
                      const int64_t* t, int32_t* last_live, int32_t B, int32_t K, int32_t V, int32_t end_idx,
                      int32_t pad_idx, bmhrl_stream_t stream);
int bmhrl_beam_reorder(const bmhrl_beam_buffer* table, int32_t n_buffers, int64_t n_blocks, const int32_t* parent,
                       int32_t rows, int32_t K, const int64_t* t, int32_t phase, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Diverse (group) beam search (bmhrl_amd/decode.py GroupBeamDecoder, rules G1-G4 of its group beam search section).
 *  bmhrl_group_beam_select: bmhrl_beam_select with the K beams of a sample split into G groups of K' = K / G consecutive
 *    beams that choose one after another, g = 0 .. G-1.  A live beam k of group g offers (k, v) with s = score_k + logp[k][v]
 *    and the selection value a = s - diversity_penalty * c (c as fp32, one fp32 multiply, one fp32 subtract, no FMA; c = 0:
 *    a = s bit for bit), c = how many beams of groups 0 .. g-1 of the sample chose, at this step, token v as a candidate of
 *    a live beam; a finished beam offers (k, pad) with a = s = score_k, neither penalised nor counted.  The K' best of the
 *    group's candidates by a, ties to the smaller k*V + v, become beams g*K' .. g*K' + K' - 1 best first: a parent always
 *    lies in its own group.  The new score is s, never a.  Outputs exactly as bmhrl_beam_select writes them (scores and
 *    flags may alias the inputs; parent = the beam index 0..K-1 within the sample; the next token; hist[row][t + 1] when
 *    t + 1 < hist_cols; last_live[0] = t + 1 when any new beam is live); t is read from the device word.  One launch for
 *    all groups; G = 1 selects what bmhrl_beam_select selects, bit for bit.
 *    Refused with -22, outputs untouched: a null pointer, B < 1, K < 1, K > 16, G < 1, K % G != 0, K / G > V, a
 *    diversity_penalty that is negative or not finite (and the ld / ldh / hist_cols / pad_idx conditions of
 *    bmhrl_beam_select).
 * ------------------------------------------------------------------------------------------- */
int bmhrl_group_beam_select(const float* logp, int64_t ld, const float* scores_in, const uint8_t* finished_in,
                            float* scores_out, uint8_t* finished_out, int32_t* parent, int64_t* tok, int64_t* hist,
                            int64_t ldh, int32_t hist_cols, const int64_t* t, int32_t* last_live, int32_t B, int32_t K,
                            int32_t V, int32_t end_idx, int32_t pad_idx, int32_t G, float diversity_penalty,
                            bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-prefix caption rewards (bmhrl_amd/rewards.py CiderScorer / BleuScorer): the score of every prefix of every sampled
 * caption against its reference caption, as the reference's metrics/cider.py and metrics/bleu.py compute it on the host.
 *  hyp (B, L) int64 vocab ids, row stride ldh; vmap[V]: vocab id -> word id (-1: the token yields no word; ids outside
 *  [0, V) yield none either); eos: the vocab id of "</s>" (CIDEr stops there; -1: none); ref (B, R) int32 word ids, row
 *  stride ldr, of which ref_len[b] (device, clamped to [0, R]) are used.  CIDEr reads the document-frequency table:
 *  df_cap (a power of two) keys of 4 int32 word ids (-1 behind the gram; key[0] = -1: empty slot) and log(df) per key.
 *  Writes scores (B, L) fp64 (the reference's per-prefix `rewards` row, padded as it pads) and delta (B, L) fp32
 *  (column 0: the score, then first differences).  n: gram lengths 1..n (1 <= n <= 4); sigma: CIDEr's length penalty.
 *  L <= BMHRL_REWARDS_MAX_L, R <= BMHRL_REWARDS_MAX_R; other shapes are refused with -22.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_REWARDS_MAX_L 256
#define BMHRL_REWARDS_MAX_R 512
#define BMHRL_REWARD_CIDER 0
#define BMHRL_REWARD_BLEU 1
int bmhrl_rewards(const int64_t* hyp, int64_t ldh, const int32_t* vmap, int32_t V, int64_t eos, const int32_t* ref,
                  int64_t ldr, const int32_t* ref_len, const int32_t* df_keys, const double* df_logs, int32_t df_cap,
                  int32_t metric, int32_t n, double sigma, int32_t B, int32_t L, int32_t R, double* scores, int64_t lds,
                  float* delta, int64_t ldd, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-prefix METEOR rewards (bmhrl_amd/rewards.py MeteorScorer; the rules are in DESIGN.md section 19): nltk's
 * single_meteor_score of every prefix of every sampled caption against its reference caption, as the reference's
 * metrics/batched_meteor.py computes it on the host.  No cut at an end token.
 *  hyp (B, L) int64 vocab ids, row stride ldh; vmap[V]: vocab id -> word id (-1: the token yields no word and its position
 *  repeats the score before it; ids outside [0, V) yield none either); vstem[V]: vocab id -> stem id of the entries that
 *  yield a word (null: no stem stage); syn_off[V + 1], syn_ids[n_syn]: the synonym sets of the entries' words as CSR rows
 *  of word ids (both null: no synonym stage; exactly one null is refused; offsets are clamped to [0, n_syn]; the word
 *  itself always belongs to its set, listed or not).  ref / ref_stem (B, R) int32 word ids / stem ids of the reference
 *  words, one row stride ldr, of which ref_len[b] (device, clamped to [0, R]) are used; ref_stem is read only with vstem.
 *  Every prefix is aligned from scratch: exact, then stem, then synonym matches, each over what the stage before left
 *  unmatched, hypothesis words from last to first, each taking the highest unmatched reference position that passes.
 *  score = (1 - gamma * pow(chunks / m, beta)) * P R / (alpha P + (1 - alpha) R) in fp64; 0 without a match.
 *  Writes scores (B, L) fp64 and delta (B, L) fp32 (column 0: the score as fp32, then differences of the fp32 scores).
 *  L <= BMHRL_REWARDS_MAX_L, R <= BMHRL_REWARDS_MAX_R; other shapes and null required pointers are refused with -22.
 *  Deterministic: no atomics, no reduction across samples.
 * ------------------------------------------------------------------------------------------- */
int bmhrl_meteor(const int64_t* hyp, int64_t ldh, const int32_t* vmap, const int32_t* vstem, int32_t V,
                 const int32_t* syn_off, const int32_t* syn_ids, int32_t n_syn, const int32_t* ref, const int32_t* ref_stem,
                 int64_t ldr, const int32_t* ref_len, double alpha, double beta, double gamma, int32_t B, int32_t L,
                 int32_t R, double* scores, int64_t lds, float* delta, int64_t ldd, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation forms of the caption metrics (bmhrl_amd/evaluate.py DenseCaptionEvaluator): what the
 * reference's evaluation/evaluate.py asks of pycocoevalcap's Bleu, Rouge and Cider for each video, over the video's
 * (prediction, reference) pairs.
 *  hyp (P, L) / ref (P, R) int32 word ids >= 0 out of one string table, row strides ldh / ldr, of which hyp_len[p] /
 *  ref_len[p] (device, clamped to [0, L] / [0, R]) are used.  group_off (G + 1) int32, device: the pairs
 *  [group_off[g], group_off[g + 1]) are group g; group_off[0] = 0, group_off[G] = P, never descending (an empty group
 *  scores 0 everywhere).  The offsets are copied back and checked before the launches, so the call synchronises the
 *  stream once and cannot be captured in a graph; nothing is read back between the two launches.
 *  Per pair: pair_ints (P, 10) int32 = BLEU's guess[4], clipped correct[4], the hypothesis length, the reference length;
 *  pair_lcs (P) int32 the LCS length; pair_cider (P) fp64 = 10 * the mean over the gram lengths 1..4 of the tf-idf cosine
 *  with the Gaussian length penalty (sigma 6, bigram counts), document frequency of a gram = the number of pairs of the
 *  group whose reference holds it, log reference length = log(pairs of the group).
 *  Per group: group_scores (G, 6) fp64 = Bleu_1..4 (counts and lengths summed over the group, tiny 1e-15, small 1e-9,
 *  brevity penalty of the summed lengths), the mean ROUGE-L (beta 1.2; 0 for a pair without a common word), the mean of
 *  pair_cider.  The floating-point sums run in pair order: two runs give equal bits.
 *  L <= BMHRL_REWARDS_MAX_L, R <= BMHRL_REWARDS_MAX_R; null pointers, P <= 0, G <= 0, other shapes and offsets that
 *  descend or do not span [0, P] are refused with -22.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_CAPTION_EVAL_PAIR_INTS 10
#define BMHRL_CAPTION_EVAL_GROUP_SCORES 6
int bmhrl_caption_eval(const int32_t* hyp, int64_t ldh, const int32_t* hyp_len, const int32_t* ref, int64_t ldr,
                       const int32_t* ref_len, const int32_t* group_off, int32_t P, int32_t G, int32_t L, int32_t R,
                       int32_t* pair_ints, int32_t* pair_lcs, double* pair_cider, double* group_scores,
                       bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SODA_c dense-captioning evaluation (bmhrl_amd/evaluate.py soda_scores; the rules are in DESIGN.md section 25).  A group
 * is one (video, ground-truth file): P_g predictions in time order and R_g references in story order.  Both calls read
 *  hyp_off / ref_off (G + 1) int32 and cell_off (G + 1) int64, device: group g owns the entries [hyp_off[g], hyp_off[g+1])
 *  of the prediction-side arrays (n_pred entries in all), [ref_off[g], ref_off[g+1]) of the reference-side arrays (n_ref)
 *  and the cells [cell_off[g], cell_off[g+1]) of S (n_cells), cell (i, j) at cell_off[g] + i * R_g + j.  Every offset
 *  array starts at 0, never descends and ends at n_pred / n_ref / n_cells, and cell_off[g+1] - cell_off[g] = P_g * R_g;
 *  a group with P_g = 0 or R_g = 0 owns no cell.  The offsets (and the indices below) are copied back and checked before
 *  the launch, so each call synchronises the stream once and cannot be captured in a graph; nothing else is read back, and
 *  S stays on the device between the two calls.  No atomics; equal inputs give equal bits.
 *
 * bmhrl_meteor_matrix: S[cell (i, j) of g] = the METEOR score of the whole hypothesis hyp_idx[hyp_off[g] + i] against the
 *  reference ref_idx[ref_off[g] + j], fp64, with the bits of bmhrl_meteor's scores column L - 1 for that pair.
 *  hyp (Nh, L) int64 vocab ids of the distinct hypotheses, row stride ldh (-1 and ids outside [0, V) yield no word; a
 *  hypothesis without a word scores 0); vmap / vstem / V / syn_off / syn_ids / n_syn / alpha / beta / gamma as in
 *  bmhrl_meteor; ref / ref_stem (Nr, R) int32 with one row stride ldr and ref_len (Nr) (device, clamped to [0, R]): the
 *  distinct references; hyp_idx (n_pred) / ref_idx (n_ref) int32, device, inside [0, Nh) / [0, Nr).  One alignment per
 *  cell; only the n_cells cells are written.  L <= BMHRL_REWARDS_MAX_L, R <= BMHRL_REWARDS_MAX_R, any P_g and R_g.
 * bmhrl_soda_dp: out (G, T, 4) fp64 = max_score, precision, recall, F of every group at every threshold tious[t] (T,
 *  fp64, device).  pred_seg (n_pred, 2) / ref_seg (n_ref, 2) fp64 start, end, in matching order.  With
 *  iou = evaluate.tiou(prediction i, reference j) (intersection over the capped union plus 1e-8, in that function's order
 *  of operations) and c[i][j] = (iou < tious[t] ? 0 : iou) * S[i][j]:
 *  D[i][j] = max(D[i-1][j], D[i][j-1], D[i-1][j-1] + c[i][j]) with zero borders; max_score = D[P_g][R_g], precision =
 *  max_score / P_g, recall = max_score / R_g, F = ((2 precision) recall) / (precision + recall), 0 when the sum is 0.  fp64
 *  without contraction: the bits of the plain double loop.  A group with P_g = 0 or R_g = 0 writes four zeros.
 *  R_g <= BMHRL_SODA_MAX_REFS, any P_g, 1 <= T <= BMHRL_SODA_MAX_T.
 * Refused with -22 before any launch: a null required pointer, G <= 0, shapes past the limits or the row strides (Nh, Nr,
 *  L, R, V < 1; ldh < L; ldr < R), vstem without ref_stem, exactly one of syn_off / syn_ids, negative counts, offsets that
 *  break the rules above, indices outside their range.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_SODA_MAX_REFS 256
#define BMHRL_SODA_MAX_T 16
int bmhrl_meteor_matrix(const int64_t* hyp, int64_t ldh, int32_t Nh, int32_t L, const int32_t* vmap, const int32_t* vstem,
                        int32_t V, const int32_t* syn_off, const int32_t* syn_ids, int32_t n_syn, const int32_t* ref,
                        const int32_t* ref_stem, int64_t ldr, const int32_t* ref_len, int32_t Nr, int32_t R,
                        const int32_t* hyp_idx, int32_t n_pred, const int32_t* ref_idx, int32_t n_ref, const int32_t* hyp_off,
                        const int32_t* ref_off, const int64_t* cell_off, int32_t G, double alpha, double beta, double gamma,
                        double* S, int64_t n_cells, bmhrl_stream_t stream);
int bmhrl_soda_dp(const double* pred_seg, int32_t n_pred, const double* ref_seg, int32_t n_ref, const int32_t* hyp_off,
                  const int32_t* ref_off, const int64_t* cell_off, int32_t G, const double* S, int64_t n_cells,
                  const double* tious, int32_t T, double* out, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sampled caption decoding (bmhrl_amd/decode.py SampleDecoder; the rules are at the top of its sampling section).  One step
 * for every row r of logp (rows, ld) fp32 log-probs, t read from the device word t[0]:
 *  finished[r] != 0: tok[r] = pad_idx, out[r][t + 1] = pad_idx, step_logp / step_logq [r][t] = 0, sum_logp unchanged;
 *  otherwise q_v = exp((lp_v - max lp) / temperature) over the order (lp descending, ties to the smaller id); top_k (0 or
 *  >= V: all) and top_p (1: all) keep the shorter prefix of that order (count k; mass >= top_p * sum q), at least one token;
 *  u = uniform01(seed + seed_dev[0], ((row_offset + r) << 16) + t) (common.h; seed_dev may be null: 0); the pick is the
 *  first kept token of positive q, in token-id order, whose inclusive q sum exceeds u * kept mass (none: the last such
 *  token).  temperature = 0, top_k = 1 and rows without a finite entry take the arg-max (first maximum; step_logq 0).
 *  Writes tok[r], out[r][t + 1], sum_logp[r] += lp_pick, finished[r] = 1 when the pick is end_idx, step_logp[r][t] =
 *  lp_pick and step_logq[r][t] = log(q_pick / kept mass) (both optional, row stride ld_out like out); the history
 *  entries only when t + 1 < ld_out.  1 <= V <= BMHRL_SAMPLE_MAX_V, temperature finite >= 0, top_k >= 0,
 *  0 < top_p <= 1, 0 <= pad_idx < V; other arguments are refused with -22.  Deterministic: no atomics.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_SAMPLE_MAX_V 16384
int bmhrl_sample_step(const float* logp, int64_t ld, int32_t rows, int32_t V, float temperature, int32_t top_k, float top_p,
                      uint64_t seed, const uint64_t* seed_dev, const int64_t* t, int64_t row_offset, int32_t end_idx,
                      int32_t pad_idx, uint8_t* finished, int64_t* tok, int64_t* out, int64_t ld_out, float* sum_logp,
                      float* step_logp, float* step_logq, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Constrained caption decoding (bmhrl_amd/decode.py; the rules are at the top of its constraints section).  For every row r
 * of logp (rows, ld) fp32 log-probs, edited in place, with t read from the device word t[0] and the row's sequence
 * s = hist[r][0 .. t] (int64 token ids, row stride ld_hist; ids outside [0, V) take part in the comparisons but select no
 * entry):
 *  1. penalty != 1: for every distinct id v of s with v != pad_idx, lp[v] = lp[v] * penalty (one fp32 multiply per id);
 *  2. ngram = n >= 1 and t + 1 >= n: for every j in [0, t + 1 - n] with s[j .. j+n-2] == s[t-n+2 .. t],
 *     lp[s[j+n-1]] = -inf (n = 1: every token of s);
 *  3. t < min_len: lp[end_idx] = -inf;
 *  in this order, so a banned entry is -inf whatever rule 1 did to it.  At most t + 2 entries of a row are written and
 *  columns V .. ld-1 are never touched; ngram = 0, min_len = 0, penalty = 1 writes nothing.  The history holds ld_hist
 *  positions per row, 1 <= ld_hist <= BMHRL_LOGIT_RULES_MAX_HIST (the kernel's LDS copy of s); a launch whose t lies
 *  outside [0, ld_hist - 1] writes nothing.  rows >= 1, 1 <= V <= ld, ngram >= 0, min_len >= 0, penalty finite > 0,
 *  0 <= end_idx < V, 0 <= pad_idx < V; other arguments are refused with -22.  Deterministic: no atomics.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_LOGIT_RULES_MAX_HIST 256
int bmhrl_logit_rules(float* logp, int64_t ld, int32_t rows, int32_t V, const int64_t* hist, int64_t ld_hist,
                      const int64_t* t, int32_t ngram, int32_t min_len, float penalty, int32_t end_idx, int32_t pad_idx,
                      bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Paragraph-aware constrained decoding (bmhrl_amd/decode.py; rules C1-C5 of its constraints section): the three rules of
 * the entry above and the context rules in one launch, which a token step issues IN PLACE of the plain one.  ctx holds
 * rows / rows_per_ctx contexts of ld_ctx int64 entries each (row stride ld_ctx): the tokens of a clip's earlier captions.
 * An entry is a word when 0 <= id < V and id != pad_idx, anything else a gap.  Row r reads context row r / rows_per_ctx.
 *  1.  as above;
 *  C1. ctx_penalty != 1: for every distinct word id v of the context, lp[v] = lp[v] * ctx_penalty (one fp32 multiply per
 *      id, after rule 1's where an id is in both);
 *  2.  as above;
 *  C2. ctx_ngram = n_c >= 1 and t >= n_c - 1: for every j in [0, ld_ctx - n_c] whose window ctx[j .. j+n_c-1] is all words
 *      and whose first n_c - 1 entries equal s[t-n_c+2 .. t] (the last n_c - 1 generated tokens, never the start token;
 *      empty for n_c = 1), lp[ctx[j+n_c-1]] = -inf.  A window that holds a gap matches nothing;
 *  3.  as above;
 *  in this order.  Columns V .. ld-1 and other rows are never touched, and a t outside [0, ld_hist - 1] writes nothing.
 *  Everything the entry above refuses is refused here, and so are a null ctx, ld_ctx outside
 *  [1, BMHRL_LOGIT_RULES_MAX_CTX], rows_per_ctx < 1 or rows % rows_per_ctx != 0, ctx_ngram < 0, a ctx_penalty that is not
 *  finite or <= 0, and V > BMHRL_LOGIT_RULES_CTX_MAX_V (C1's map of one bit per token id in LDS), all with -22.
 *  Deterministic: the only atomic is an LDS or-and-return that picks which context position does an id's one multiply;
 *  global memory sees plain stores, and equal inputs give equal bits.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_LOGIT_RULES_MAX_CTX 1024
#define BMHRL_LOGIT_RULES_CTX_MAX_V 65536
int bmhrl_logit_rules_ctx(float* logp, int64_t ld, int32_t rows, int32_t V, const int64_t* hist, int64_t ld_hist,
                          const int64_t* t, int32_t ngram, int32_t min_len, float penalty, int32_t end_idx, int32_t pad_idx,
                          const int64_t* ctx, int64_t ld_ctx, int32_t rows_per_ctx, int32_t ctx_ngram, float ctx_penalty,
                          bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Consensus (minimum-Bayes-risk) utilities of a clip's hypotheses (bmhrl_amd/decode.py; rules R1-R6 are at the top of its
 * consensus section).  hist is a decoder's token history: row r = b * K + k holds hypothesis k of clip b, row stride ld,
 * column 0 the start token and columns 1 .. steps the generated tokens; columns beyond `steps` are never read.  The words
 * of a hypothesis are its tokens before the first end_idx (all `steps` tokens without one; an end_idx that is no token id
 * never matches).  Writes util[b * K + i] = U_i, the mean over j != i of u(i, j) (0 with K = 1), and -- when pair is not
 * null -- pair[(b * K + i) * K + j] = u(i, j), with u(i, i) written as 0.  u(i, j) is the mean over g = 1 .. N of the
 * clipped g-gram match of i in j divided by the larger of the two gram masses, a gram weighing the mean of its tokens'
 * token_weight[V] entries (null: every gram weighs 1; an id outside [0, V) weighs 0 and still compares by its id).  All
 * arithmetic is fp64 in the order the rules prescribe, without FMA contraction and without atomics: equal inputs give
 * equal bits.  B >= 1, 1 <= K <= BMHRL_CONSENSUS_MAX_K, 0 <= steps <= BMHRL_CONSENSUS_MAX_STEPS (0: every utility is 0),
 * 1 <= N <= BMHRL_CONSENSUS_MAX_N, V >= 0 (>= 1 with token_weight), ld >= steps + 1; other arguments are refused with -22.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_CONSENSUS_MAX_K 16
#define BMHRL_CONSENSUS_MAX_STEPS 256
#define BMHRL_CONSENSUS_MAX_N 4
int bmhrl_consensus(const int64_t* hist, int64_t ld, int32_t B, int32_t K, int32_t steps, int64_t end_idx, int32_t N,
                    const float* token_weight, int32_t V, double* util, double* pair, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The DETR word loss (bmhrl_amd/loss/hungarian_matcher.py): the caption's words are matched one to
 * one to the detector's Q queries by minimum total cost -cost_scale * p(word | query), and the class logits are scored by
 * the cross entropy with weight eos_coef on the rows of unmatched queries, whose class is "no word" (the last, C - 1).
 * Four ordinary launches, ordered by the stream alone; none synchronises across blocks or uses atomics, and equal inputs
 * give equal bits.  B, Q, L >= 1, Q <= BMHRL_WORD_LOSS_MAX_Q, L <= BMHRL_WORD_LOSS_MAX_L, L <= Q, C >= 2, leading
 * dimensions >= C, B * Q <= INT32_MAX; other shapes and null required pointers are refused with -22 and launch nothing.
 *
 * bmhrl_word_cost: logits (B * Q, C) fp32 with leading dimension ld (any ld >= C: rows need only 4-byte alignment; columns
 *  C .. ld-1 are never read); captions (B, L) int64, row stride ldc.  The words of sample b are its entries != pad_idx, in
 *  order, wherever the pads sit; an id outside [0, C - 2] is dropped like a pad, so no row is ever indexed outside
 *  [0, C).  Writes words (B, L) int32 (-1 behind the n_b words), n_words (B) int32, and per row r = b * Q + q:
 *  lse[r] = log sum exp of the row (maximum subtracted) with lse_lo[r] the rounding residue of its last addition (the
 *  pair lse + lse_lo is what the other launches subtract: DESIGN.md section 20), x_none[r] = x[C - 1],
 *  gathered[r][j] = x[words[b][j]] and cost[r][j] = cost_scale * -exp(gathered - lse - lse_lo) for j < n_b, both 0 for
 *  j >= n_b (gathered, cost: (B, Q, L) fp32).
 * bmhrl_lsa_match: rectangular minimum-cost assignment, nothing word-specific.  cost (B, Q, L) fp32 with element strides
 *  sb, sq, sl; n (B) int32, clamped to [0, L].  Writes query_of_target (B, L) int32: targets 0 .. n_b-1 get distinct
 *  queries of minimum total cost, the rest -1.  One wavefront per sample, shortest augmenting paths with fp64 duals,
 *  every tie to the lowest query index.  Entries of targets >= n_b are never read.  A non-finite cost cannot hang or
 *  misindex the kernel; the matching is then unspecified (a target may stay at -1).
 * bmhrl_word_loss: tgt_class (B, Q) int32 = the word matched to the query or C - 1; row_w (B, Q) fp32 = 1 or eos_coef;
 *  loss_scale[0] = sum row_w (lse + lse_lo - x_t) / sum row_w, loss_scale[1] = 1 / sum row_w, summed in fp64 in a fixed order; x_t
 *  comes from gathered / x_none.  query_of_target entries outside [0, Q) match nothing; a query named twice takes the
 *  later target.
 * bmhrl_word_loss_bwd: dlogits[r][c] = g * row_w[r] * loss_scale[1] * (exp(x[r][c] - lse[r] - lse_lo[r]) - [c == tgt_class[r]]) for
 *  c < C, into fp32 rows of leading dimension ldd (columns C .. ldd-1 are not written).  g: device scalar, null = 1.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_WORD_LOSS_MAX_Q 128
#define BMHRL_WORD_LOSS_MAX_L 64
int bmhrl_word_cost(const float* logits, int64_t ld, const int64_t* captions, int64_t ldc, int64_t pad_idx, float cost_scale,
                    int32_t B, int32_t Q, int32_t L, int32_t C, int32_t* words, int32_t* n_words, float* lse, float* lse_lo,
                    float* x_none, float* gathered, float* cost, bmhrl_stream_t stream);
int bmhrl_lsa_match(const float* cost, int64_t sb, int64_t sq, int64_t sl, const int32_t* n, int32_t B, int32_t Q, int32_t L,
                    int32_t* query_of_target, bmhrl_stream_t stream);
int bmhrl_word_loss(const int32_t* words, const int32_t* n_words, const int32_t* query_of_target, const float* lse,
                    const float* lse_lo, const float* x_none, const float* gathered, float eos_coef, int32_t B, int32_t Q,
                    int32_t L, int32_t C, int32_t* tgt_class, float* row_w, float* loss_scale, bmhrl_stream_t stream);
int bmhrl_word_loss_bwd(const float* logits, int64_t ld, const float* lse, const float* lse_lo, const int32_t* tgt_class,
                        const float* row_w, const float* loss_scale, const float* g, float* dlogits, int64_t ldd, int32_t B,
                        int32_t Q, int32_t C, bmhrl_stream_t stream);

/* ---- temporal proposal generation (csrc/proposal.hip) -------------------------------------------
 * Anchor heads in the YOLO style: head h of a modality sees S feature positions of cell_sec seconds each and predicts, for
 * each of the modality's A anchor lengths (seconds), a centre offset, a log length factor and an objectness logit.  All
 * launches are ordinary launches on the caller's stream, none reads back to the host, and equal inputs give equal bits.
 * Bad shapes and null required pointers are refused with -22 and launch nothing.
 *
 * bmhrl_proposal_assign: targets (n_targets, 4) fp32 rows [video index in batch, centre s, length s, unused]; anchors (A).
 *  For row r: g = centre / cell_sec, w = length / cell_sec, cell = floor(g); the best anchor is the argmax over a of the
 *  tIoU of the lengths anchors[a] / cell_sec and w laid on a common centre (fp32, the reference's tiou_vectorized arithmetic
 *  with without_center_coords), ties to the smaller a.  Writes tx[r] = g - floor(g), tw[r] = log(w / (anchors[best] /
 *  cell_sec) + 1e-16) for every row, and owner (B, A, S) int32: the LARGEST r whose (video, best anchor, cell) it is, -1
 *  where none is; rows whose video index or cell is outside [0, B) x [0, S) own nothing.  counts[0] = number of owned
 *  cells, counts[1] = B * A * S - counts[0].  B * A * S <= INT32_MAX.
 * bmhrl_proposal_head: x (B, S, 3 A) fp32 contiguous, channel 3 a + {0, 1, 2} = (c, l, o) of anchor a.  Writes the rows
 *  row_off + a * S + s of pred (B, n_total, 3): [(sigmoid(c) + s) * cell_sec, anchors[a] * exp(l), sigmoid(o)].
 *  With owner (training): sums[0..4] = loss_x, loss_w, loss_obj, loss_noobj, total, where
 *   loss_x = mean over owned cells of (sigmoid(c) - tx[r])^2      loss_w = mean over owned cells of (l - tw[r])^2
 *   loss_obj = mean over owned cells of softplus(-o)               loss_noobj = mean over the other cells of softplus(o)
 *   total = loss_x + loss_w + obj_coeff * loss_obj + noobj_coeff * loss_noobj,
 *  a mean over no cell being 0 (softplus(-o) and softplus(o) are torch's BCELoss of sigmoid(o) against 1 and 0 wherever
 *  that does not clamp its logarithm at -100); and, when dx is given, dx (B, S, 3 A) = dscale[0] * d total / d x (dscale null = 1), every
 *  element stored.  partials: 4 * BMHRL_PROPOSAL_HEAD_BLOCKS fp32 scratch; counter: 16 bytes of scratch, 16-byte aligned,
 *  zeroed by the call itself (on the stream).  The block sums are fp32 in a fixed order, their sum over the blocks fp64 in index
 *  order.  Without owner (inference): predictions only; dx must be null, sums / partials / counter are not touched.
 * bmhrl_proposal_select: pred (B, N, 3) fp32 rows [centre s, length s, confidence], durations (B) fp32.  Per video: the
 *  min(k, N) rows of highest confidence, ties to the smaller row; start = centre - length / 2, end = centre + length / 2;
 *  start = min(max(start, 0), duration), end = min(end, duration); then, when nms_tiou >= 0, greedy suppression in that
 *  order: a kept segment removes every later one whose tIoU with it is not < nms_tiou (tIoU = intersection / (min(hull,
 *  sum of lengths - intersection) + 1e-8), fp32, IEEE division).  props (B, k, 3) = [start, end, confidence] of the
 *  survivors in order, zeros behind them; count (B) int32.  1 <= k <= BMHRL_PROPOSAL_MAX_K, 1 <= N <= BMHRL_PROPOSAL_MAX_N.
 *  workspace: 64-bit words, needed when N > 4096: with c(m) = ceil(m / 4096) * k, B * (c(N) + c(c(N))) words are enough. */
#define BMHRL_PROPOSAL_MAX_K 128
#define BMHRL_PROPOSAL_HEAD_BLOCKS 1024
#define BMHRL_PROPOSAL_MAX_N (1 << 24)
int bmhrl_proposal_assign(const float* targets, int32_t n_targets, const float* anchors, int32_t A, float cell_sec, int32_t B,
                          int32_t S, int32_t* owner, float* tx, float* tw, int32_t* counts, bmhrl_stream_t stream);
int bmhrl_proposal_head(const float* x, const float* anchors, float cell_sec, int32_t B, int32_t S, int32_t A, float* pred,
                        int64_t n_total, int64_t row_off, const int32_t* owner, const float* tx, const float* tw,
                        const int32_t* counts, float obj_coeff, float noobj_coeff, const float* dscale, float* dx, float* sums,
                        float* partials, uint32_t* counter, bmhrl_stream_t stream);
int bmhrl_proposal_select(const float* pred, int32_t B, int64_t N, const float* durations, int32_t k, float nms_tiou,
                          float* props, int32_t* count, uint64_t* workspace, int64_t workspace_elems, bmhrl_stream_t stream);
/* bmhrl_proposal_select_soft: Soft-NMS over a pool.  pred, durations as for bmhrl_proposal_select.
 *  Per video the pool is the min(m, N) rows of highest confidence in that call's order (ties to the smaller row); rank = a
 *  row's position in it; corners and trimming as above.  Then at most k picks: the alive row of largest CURRENT score is
 *  picked, ties to the smaller rank (the 64-bit key (image(score) << 32) | (0xFFFFFFFF - rank)); a score < min_score ends
 *  the loop (min_score = -INFINITY: no floor); otherwise (start, end, current score, row) is emitted and the row retired,
 *  and every other alive row q with t = tIoU(picked, q) not < tiou_thresh (the fp32 tIoU above) is
 *   BMHRL_NMS_HARD      retired
 *   BMHRL_NMS_LINEAR    rescored: score_q = score_q * (1.f - t), fp32
 *   BMHRL_NMS_GAUSSIAN  rescored: score_q = score_q * (float)exp(-((double)t * (double)t) / (double)sigma), the product fp32.
 *  props (B, k, 3) = [start, end, rescored confidence] in pick order, zeros behind; rows (B, k) int32 = the picked rows'
 *  indices in pred, -1 behind (may be null); count (B) int32.  For non-negative confidences the emitted scores never
 *  increase.  Confidences are expected finite.  BMHRL_NMS_HARD with m == k <= BMHRL_PROPOSAL_MAX_K gives
 *  bmhrl_proposal_select's bits.  A fixed number of launches, nothing read back.  -22: a null pred / durations / props /
 *  count; B outside [1, 65535]; N outside [1, BMHRL_PROPOSAL_MAX_N]; m outside [1, BMHRL_PROPOSAL_SOFT_MAX_M]; k outside
 *  [1, m]; an unknown method; a NaN tiou_thresh or min_score; sigma not > 0 with BMHRL_NMS_GAUSSIAN; a workspace smaller
 *  than bmhrl_proposal_select's rule gives with k := m. */
#define BMHRL_PROPOSAL_SOFT_MAX_M 1024
#define BMHRL_NMS_HARD 0
#define BMHRL_NMS_LINEAR 1
#define BMHRL_NMS_GAUSSIAN 2
int bmhrl_proposal_select_soft(const float* pred, int32_t B, int64_t N, const float* durations, int32_t m, int32_t k,
                               int32_t method, float tiou_thresh, float sigma, float min_score, float* props,
                               int32_t* rows, int32_t* count, uint64_t* workspace, int64_t workspace_elems,
                               bmhrl_stream_t stream);
/* bmhrl_proposal_chain (csrc/event_chain.hip): event-chain selection.  props (B, P, 3) fp32 rows
 *  [start, end, score] and count (B) int32 are bmhrl_proposal_select's / bmhrl_proposal_select_soft's outputs as they
 *  stand: the first count[b] rows of video b are valid (count[b] is clamped to [0, P]; count null = all P rows).  All
 *  arithmetic fp32, uncontracted, in the order written.  Per video:
 *   eligible  row i < count with (end - start) > min_length, score == score and gain g = score - event_cost > 0
 *   order     i before j iff (start_i, end_i, i) < (start_j, end_j, j) lexicographically; position = place in it
 *   link      i -> j iff i before j, end_i <= end_j and t_ij <= max_tiou (t: bmhrl_proposal_select's fp32 tIoU)
 *   V[1][j] = g_j;  V[l][j] = the maximum over the linked i (in order) with V[l-1][i] defined of
 *             (V[l-1][i] - (overlap_weight * t_ij)) + g_j, l = 2 .. max_events.  The running maximum starts at -INFINITY
 *             and a candidate replaces it only when it is greater: the first maximum wins, and a candidate that is NaN
 *             or -INFINITY (an infinite score or weight) is no candidate.  V[l][j] without a candidate is undefined.
 *   answer    the largest defined V[l][j], ties to the smaller l, then to the earlier j; the chain is read back through
 *             the maximising i of every level.
 *  events (B, max_events, 3) = the chosen rows of props (their bits) in time order, zeros behind; chain (B, max_events)
 *  int32 = their row indices in props, -1 behind; length (B) int32; value (B) fp32 = the answer's V, 0.f for length 0
 *  (may be null).  One launch, nothing read back.  -22: a null props / events / chain / length; B outside [1, 65535]; P
 *  outside [1, BMHRL_PROPOSAL_CHAIN_MAX_P]; max_events outside [1, BMHRL_PROPOSAL_CHAIN_MAX_L]; a NaN or negative
 *  max_tiou, overlap_weight, event_cost or min_length. */
#define BMHRL_PROPOSAL_CHAIN_MAX_P 1024
#define BMHRL_PROPOSAL_CHAIN_MAX_L 32
int bmhrl_proposal_chain(const float* props, const int32_t* count, int32_t B, int32_t P, int32_t max_events, float max_tiou,
                         float overlap_weight, float event_cost, float min_length, float* events, int32_t* chain,
                         int32_t* length, float* value, bmhrl_stream_t stream);

/* ---- segment crop (csrc/segment_crop.hip) --------------------------------------------------------
 * Cuts and pads the rows of P temporal segments out of full-length feature stacks that are resident on the device: the
 * reference's crop_a_segment (captioning_datasets/load_features.py:14-35) and the padding of a batch of clips, without the
 * feature files.  One ordinary launch on the caller's stream behind a one-wave launch that zeroes status; nothing is read
 * back.
 *
 * src (V, S_pad, D) fp32 contiguous; src_len (V) int32: the true row count S of each video; durations (V) float64 seconds;
 * seg_video (P) int32; seg_times (P, 2) float64 [start s, end s].  For segment p of video v, in IEEE float64 and in this
 * order of operations (bmhrl_amd/loader.py crop_bounds):
 *   a = trunc(S * (start / duration)), b = trunc(S * (end / duration))       (toward zero; limited to the int32 range)
 *   if a == b: a -= 1 when a == S, else b += 1
 *   (lo, hi) = Python's slice(a, b).indices(S): a negative end gets + S, then both are clamped to [0, S]
 *   n = max(hi - lo, 0)
 * Rows [0, min(n, T_out)) of out[p] (P, T_out, D) are src[v, lo + r]; the rows behind them hold pad_value; n == 0 gives one
 * row of zeros and then pad_value (the loader's "missing clip").  lengths[p] = n, NOT clipped to T_out; lo[p] (optional) =
 * lo, 0 where n == 0.  status[0] = number of segments with n > T_out (their first T_out rows are copied; nothing outside out
 * is written); status[1] = number of segments without a defined crop, which are laid out as n == 0: seg_video outside [0, V),
 * duration not > 0, a non-finite quotient or product, or src_len[v] outside [0, S_pad] (no row outside src is ever read).
 * The counters are integer atomic adds of one thread per segment: exact in any order, the same with BMHRL_DETERMINISTIC.
 * Every element of out is stored exactly once; 16-byte accesses when D % 4 == 0 and src and out are 16-byte aligned, 4-byte
 * ones otherwise (any D >= 1).  -22 and nothing launched: a null pointer other than lo; V, P, D, T_out or S_pad < 1. */
int bmhrl_crop_segments(const float* src, const int32_t* src_len, const double* durations, int32_t V, int32_t S_pad, int32_t D,
                        const int32_t* seg_video, const double* seg_times, int32_t P, float pad_value, int32_t T_out,
                        float* out, int32_t* lengths, int32_t* lo, int32_t* status, bmhrl_stream_t stream);

/* ---- proposal metrics (csrc/proposal_eval.hip) ----------------------------------------------------
 * The tIoU of every prediction of a group against every reference of the group, left as integers: what detection
 * precision / recall, AR@AN and the caption pairing of bmhrl_amd/evaluate.py are built from.  iou(i, j) is
 * evaluate.tiou(prediction i, reference j): inter = max(0, min(e, e_i) - max(s, s_i)), union = min(max(e, e_i) - min(s, s_i),
 * ((e - s) + e_i) - s_i), iou = inter / (union + 1e-8), fp64 in this order without contraction (csrc/tiou.h): that
 * function's bits.  pred_seg (n_pred, 2) / ref_seg (n_ref, 2) fp64 start, end, device.
 *
 * The group table.  groups (G, 4) int32, one row per group: [p0, P, r0, R] -- the group's predictions are rows
 * [p0, p0 + P) of pred_seg and its references rows [r0, r0 + R) of ref_seg.  Any P >= 0 and R >= 0; groups may overlap
 * (the (video, file) groups of one video name the same predictions).  The outputs are laid out by the running sums of the
 * groups' own counts: out_off (2, G + 1) int64, row 0 the exclusive running sum of P (group g's predictions own the slots
 * [out_off[0][g], out_off[0][g] + P) of the prediction-side outputs, sum P slots in all), row 1 the same for R.  The table
 * is passed twice: groups_host in host memory, which is checked here before anything is launched, and groups / out_off
 * on the device, which the kernels read -- ordinary launches on the caller's stream, nothing is read back, no atomics,
 * equal inputs give equal bits.  The caller keeps the copies equal (ops.tiou_groups builds all three from one array); a
 * kernel checks its device row against the same bounds again, and a row that breaks them writes nothing.
 *
 * bmhrl_tiou_hits: a cell passes threshold t when iou > tious[t] (strict = 1) or iou >= tious[t] (strict = 0); tious (T)
 *  fp64, device, 1 <= T <= BMHRL_TIOU_MAX_T.  pred_hits (T, ld_pred) int32: [t][slot of prediction i] = the number of the
 *  group's references the prediction passes.  ref_first (T, ld_ref) int32: [t][slot of reference j] = the smallest in-group
 *  index i of a prediction that passes the reference, P when none does (so 0 in a group without predictions).  Only the
 *  first sum P / sum R words of each row are written; ld_pred >= sum P, ld_ref >= sum R.
 * bmhrl_tiou_pairs: the ordered pair list of one threshold.  pair_off (n_slots + 1) int64, device, n_slots = sum P: the
 *  exclusive running sum of max(pred_hits[slot], 1) of a strict = 0 call with the same tables and threshold.  The prediction
 *  of slot s writes the rows r0 + j of its group's references with iou >= tiou, j ascending, to pair_ref[pair_off[s] ...]
 *  (int32, n_pairs words), or a single -1 when there is none.  A word outside [pair_off[s], pair_off[s + 1]) or outside
 *  pair_ref is never written, whatever pair_off holds.
 * Refused with -22 before anything is launched: a null required pointer, T outside its range, strict other than 0 / 1,
 *  negative counts, a group with a negative entry or running past n_pred / n_ref, ld_pred < sum P, ld_ref < sum R,
 *  n_slots != sum P.  G = 0 returns 0 and launches nothing.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_TIOU_MAX_T 16
int bmhrl_tiou_hits(const double* pred_seg, int32_t n_pred, const double* ref_seg, int32_t n_ref, const int32_t* groups_host,
                    const int32_t* groups, const int64_t* out_off, int32_t G, const double* tious, int32_t T, int32_t strict,
                    int32_t* pred_hits, int64_t ld_pred, int32_t* ref_first, int64_t ld_ref, bmhrl_stream_t stream);
int bmhrl_tiou_pairs(const double* pred_seg, int32_t n_pred, const double* ref_seg, int32_t n_ref, const int32_t* groups_host,
                     const int32_t* groups, const int64_t* out_off, int32_t G, double tiou, const int64_t* pair_off,
                     int64_t n_slots, int32_t* pair_ref, int64_t n_pairs, bmhrl_stream_t stream);

/* ---- self-critical policy gradient on sampled rollouts (csrc/policy_loss.hip) ----------------------
 * bmhrl_rollout_advantage: rollouts and the reward launch's per-prefix table -> per-token weights, nothing read on the host.
 *  toks (B * n, ldt) int64, sample-major (the n rollouts of clip b are rows b * n .. b * n + n - 1), column 0 the start
 *  token, columns 1 .. m the generated tokens (a row holds the pad token after its first end_idx); scores (B * n, m) fp64
 *  with row stride lds: the per-prefix scores of toks[:, 1:]; base (B) fp64, read with BMHRL_BASELINE_GIVEN only.
 *   R1. len_i = 1 + the index of the first end_idx in toks[i, 1 : m + 1], or m without one;
 *   R2. r_i = scores[i, len_i - 1], a copy of the fp64 word (whether the end token counts as a word is the scorer's business);
 *   R3. baseline, fp64 without FMA contraction: LEAVE_ONE_OUT b_i = (sum of r_j over the clip's rollouts j != i, j
 *       ascending, from 0.0) / (n - 1); GIVEN b_i = base[clip]; NONE b_i = 0;
 *   R4. adv_i = r_i - b_i;
 *   R5. N = sum of len_i, an integer;
 *   R6. weight[i, t] = (float)(adv_i / (double)N) for t < len_i, else +0.0f;
 *   R7. stats[0..3] = mean r, mean b, mean len, N as fp64: the sums of r and of b run in row order from 0.0 and are divided
 *       once by (double)(B * n); mean len = (double)N / (double)(B * n).
 *  Writes len (B * n) int32, reward and adv (B * n) fp64, weight (B * n, m) fp32 with row stride ldw (columns m .. ldw are
 *  never written) and stats (4) fp64.  One block; every sum has one owner that adds in the order above, so equal inputs give
 *  equal bits and a host restatement of R1-R7 gives the same bits.  Refused with -22: a null required pointer, n outside
 *  [1, BMHRL_ROLLOUT_MAX_N], m outside [1, BMHRL_REWARDS_MAX_L], B < 1, LEAVE_ONE_OUT with n == 1, GIVEN without base, an
 *  unknown baseline, ldt < m + 1, lds < m, ldw < m.
 *
 * bmhrl_policy_loss_fwd / bmhrl_policy_loss_bwd: the loss on the log-probs of the training forward.  Per row i of logp
 *  (rows, V) fp32 with row stride ld: the action a_i (int64), the weight w_i (fp32, the advantage's sign), optionally
 *  logq_i (fp32, the rollout's log-prob of a_i) with the clip eps, optionally the entropy weight beta_i (fp32, already masked
 *  and normalised).
 *   policy term, clip off (eps == 0 and logq null):  l_i = -w_i logp[i, a_i],  d l_i / d logp[i, a_i] = -w_i;
 *   policy term, clip on (eps > 0 and logq given):   rho = exp(logp[i, a_i] - logq_i),
 *       l_i = -min(rho w_i, clamp(rho, 1 - eps, 1 + eps) w_i); the gradient at a_i is -rho w_i where the unclipped branch is
 *       the minimum (ties included), else 0;
 *   entropy term (ent_weight given): H_i = -sum_v p_v logp_v, p_v = exp(logp_v), a column at -inf contributing 0 to the value
 *       and to the gradient; the row loss gains -beta_i H_i and the gradient beta_i p_v (1 + logp_v) at every column.  The
 *       log-probs are independent variables here (the head's own log-softmax backward does the rest).
 *  An action outside [0, V) makes the row contribute nothing: its row loss is 0 and its gradient row is all zeros.
 *  fwd writes row_loss (rows) and row_entropy (rows) (H_i with ent_weight, action in range or not; 0 without it).
 *  bwd writes the dense gradient dlogp (rows, V) fp32 with row stride ldg, every entry times gscale[0] * drow[i] (both fp32,
 *  device), in one pass: without ent_weight zeros and one entry per row.  Columns V .. ld / ldg are never written.  No
 *  atomics: equal inputs give equal bits.
 *  Dispatch.  fwd without ent_weight: a gather, one thread per row.  fwd with ent_weight: one 256-thread block per row, the
 *  16-byte path when V % 4 == 0, ld % 4 == 0 and logp is 16-byte aligned, else the scalar path.  bwd: one 256-thread block
 *  per row, the 16-byte path when V % 4 == 0, ld % 4 == 0, ldg % 4 == 0 and logp and dlogp are 16-byte aligned, else the
 *  scalar path (any V on either).
 *  Refused with -22: a null required pointer (gscale and drow are required), rows < 1, V < 1, ld < V, ldg < V, eps < 0 or
 *  NaN, and exactly one of eps > 0 / logq given.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_ROLLOUT_MAX_N 16
#define BMHRL_BASELINE_NONE 0
#define BMHRL_BASELINE_LEAVE_ONE_OUT 1
#define BMHRL_BASELINE_GIVEN 2
int bmhrl_rollout_advantage(const int64_t* toks, int64_t ldt, int32_t B, int32_t n, int32_t m, int64_t end_idx,
                            const double* scores, int64_t lds, int32_t baseline, const double* base, int32_t* len, double* reward,
                            double* adv, float* weight, int64_t ldw, double* stats, bmhrl_stream_t stream);
int bmhrl_policy_loss_fwd(const float* logp, int64_t ld, const int64_t* action, const float* weight, const float* logq, float clip,
                          const float* ent_weight, float* row_loss, float* row_entropy, int64_t rows, int32_t V,
                          bmhrl_stream_t stream);
int bmhrl_policy_loss_bwd(const float* logp, int64_t ld, const int64_t* action, const float* weight, const float* logq, float clip,
                          const float* ent_weight, const float* gscale, const float* drow, float* dlogp, int64_t ldg, int64_t rows,
                          int32_t V, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Paragraph n-gram statistics (bmhrl_amd/evaluate.py paragraph_stats; the rules are in DESIGN.md section 33).  A paragraph
 * is a run of sentences, a sentence a run of word ids: tok (n_tok) int32 (any value: only equality is used), sent_off
 * (S + 1) int32 token offsets of the sentences (sent_off[0] = 0, sent_off[S] = n_tok), para_off (G + 1) int32 sentence
 * offsets of the paragraphs (para_off[0] = 0, para_off[G] = S); both never descend, and an empty sentence or paragraph is
 * allowed.  All three are device memory.
 *  S1. For n = 1..4 an occurrence is a start position whose n tokens lie inside one sentence; two occurrences are the same
 *      gram when their n ids are equal.  Grams span neither a sentence nor a paragraph boundary.
 *  S2. stats (G, 4, BMHRL_NGRAM_STATS_INTS) int32, per paragraph and n: total (occurrences), distinct (different grams),
 *      in_repeated (occurrences whose gram occurs at least twice in the paragraph), cross (occurrences whose gram also
 *      occurs in an earlier sentence of the paragraph), max_count (the largest multiplicity; 0 when total = 0).
 *  S3. A paragraph holds at most BMHRL_PARAGRAPH_MAX_TOKENS tokens; any number of sentences.
 *  Refused with -22 before the launch, stats untouched: a null pointer (tok may be null only with n_tok = 0), G <= 0,
 *  S < 0, n_tok < 0, offsets that descend or do not span [0, S] / [0, n_tok], a paragraph past the limit.  The offsets are
 *  copied back and checked on the host as bmhrl_caption_eval does it: one stream synchronisation, not for captured graphs.
 *  One 256-thread workgroup per paragraph, integers only, no atomics: equal inputs give equal bits.
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_PARAGRAPH_MAX_TOKENS 1024
#define BMHRL_NGRAM_STATS_INTS 5
int bmhrl_ngram_stats(const int32_t* tok, int32_t n_tok, const int32_t* sent_off, int32_t S, const int32_t* para_off,
                      int32_t G, int32_t* stats, bmhrl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Bootstrap over videos (csrc/bootstrap.hip; bmhrl_amd/evaluate.py bootstrap_ratios_host is the same definition in numpy;
 * DESIGN.md section 37).  values (M, N) fp64: column m's N per-video values are contiguous.  weights (M, N) fp64 or null.
 * stats (resamples + 1, M) fp64.  All arithmetic fp64, uncontracted, in the order written.
 *  B1. Counts.  Row 0 is the observed statistic: c_i = 1 for every i.  Row r >= 1 makes N draws j = 0 .. N - 1:
 *      h = hash_u32(seed, ((uint64)r << 32) | j) (csrc/common.h), i = (uint32)(((uint64)h * N) >> 32), and c_i is the number
 *      of draws that hit i.  Integers: no order enters, and the c_i sum to N.
 *  B2. Lane sums.  For a column m and a lane t = 0 .. 63, p_t starts at +0.0 and for i = t, t + 64, .. < N in ascending
 *      order p_t = p_t + ((double)c_i * x[m][i]): two roundings per term, every term added, those with c_i = 0 too.
 *  B3. Butterfly.  For s = 32, 16, 8, 4, 2, 1: p_t = p_t + p_(t xor s).  Every lane ends with the same bits, S_num.
 *  B4. Statistic.  With weights S_den is formed the same way from w[m][i] and stats[r][m] = S_num / S_den, or 0.0 when
 *      S_den == 0; without weights stats[r][m] = S_num / (double)N.
 *  The result depends on nothing else: not the grid, the split of the columns or the rows a workgroup carries.  Nothing is
 *  promised for non-finite inputs.  One launch, no global atomics, nothing read back.
 *  -22: a null values / stats; N outside [1, BMHRL_BOOTSTRAP_MAX_N]; M outside [1, BMHRL_BOOTSTRAP_MAX_M]; resamples
 *  outside [1, BMHRL_BOOTSTRAP_MAX_R].
 * ------------------------------------------------------------------------------------------- */
#define BMHRL_BOOTSTRAP_MAX_N 16384
#define BMHRL_BOOTSTRAP_MAX_M 4096
#define BMHRL_BOOTSTRAP_MAX_R 1048576
int bmhrl_bootstrap_ratios(const double* values, const double* weights, int32_t N, int32_t M, int32_t resamples, uint64_t seed,
                           double* stats, bmhrl_stream_t stream);
/* the rows of stats one workgroup of that launch carries (4, 2 or 1: the most whose counts fit its LDS budget); -22 for an
 * N or a number of resamples the launch refuses.  Host only; the result of the launch does not depend on it. */
int bmhrl_bootstrap_rows(int32_t N, int32_t resamples);

int bmhrl_hip_abi_version(void);
/* 1 when BMHRL_DETERMINISTIC selects the ordered sums (read once, by the library; atoi(value) != 0).  The host side asks
 * here instead of parsing the variable itself, so both sides always agree. */
int bmhrl_deterministic_enabled(void);

#ifdef __cplusplus
}
#endif
#endif /* BMHRL_HIP_H */

/*
 * taiyaki_amd_loss_varlen.h -- C ABI of the flip-flop training loss on the MI355X (gfx950) for batches whose columns have
 * different TIME lengths: the loss end of training through variable-length batches (the network half is
 * taiyaki_amd_rnn_varlen_train.h).  A library of its own (libtaiyaki_amd_loss_varlen.so: the flip-flop ABI is pinned) --
 * kernel A's sources (crf_band.hip, crf_kernels.hip) compiled a second time with -DTK_LOSS_VARLEN, and the posterior with
 * lengths of taiyaki_amd_decode_varlen.h.  It shares the conventions of taiyaki_amd_flipflop.h: device pointers plus a
 * stream, nothing allocated or synchronised inside, a nullable status word with that header's bits and counts.
 *
 *   lengths (nbatch) int32 on the device: the rows of column n, T_n, clamped to [0, nblk] where it is read.
 *
 * ONE RULE.  Column n's results are those of the fixed-length entry point of taiyaki_amd_flipflop.h on
 * scores[:T_n, n:n+1] with that read's labels:
 *   cost[n] = -score / T_n (x out_scale); the fused lossvector[n] adds logZ_n / T_n;
 *   gradient rows [0, T_n) are that call's rows; every row at or beyond T_n is WRITTEN, as exactly 0 (in the fused form
 *   too: nothing of the log-partition's gradient reaches the padding);
 *   a column with T_n == 0 or seqlen[n] == 0 has loss 0 and gradient 0, and sets no status bit;
 *   a read with seqlen[n] > T_n + 1 (no complete path) behaves as the fixed-length call on that column alone does, the
 *   status word included (a non-finite cost: TK_STATUS_NONFINITE_SCORE);
 *   scores beyond a column's length are never used: a NaN there reaches no output.
 * The workspace is the fixed-length call's at (nblk, nbatch): tk_crf_flipflop_workspace_bytes_sharp.  The checkpoint
 * layout stays sized and indexed by nblk; the launch's configuration (block length, frame slope, cells per lane) is chosen
 * once per launch from (sharpening factor, form, max_seqlen, bulk_seqlen, nblk), as there -- tk_crf_varlen_plan reports it.
 * A column whose own band is narrower than that configuration suits is what the tail launch's retry is for; the reads
 * retried and redone are counted in the status word as there (TK_STATUS_RETRIED_SHIFT, TK_STATUS_GATED_SHIFT).
 */
#ifndef TAIYAKI_AMD_LOSS_VARLEN_H
#define TAIYAKI_AMD_LOSS_VARLEN_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_*, TK_STATUS_*, tk_seq_labels */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * (a) kernel A with a length per column: tk_crf_flipflop_labels_dev's arguments, then `lengths`.  Cost only (grad NULL)
 * or cost and gradient; the plain CRF and cat-mod (modidx / modfact non-NULL, labels->mod_cats and its tables).
 * lengths == NULL: every column has nblk rows -- bit for bit what tk_crf_flipflop_labels_dev gives.
 * ------------------------------------------------------------------------- */
int tk_crf_flipflop_varlen_labels_dev(const float *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                                      const tk_seq_labels *labels, const int32_t *seqlen,
                                      int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                                      size_t max_seqlen, size_t ncan, float sharp_can, float sharp_mod,
                                      float out_scale, float *cost, float *grad, void *workspace,
                                      size_t workspace_bytes, uint32_t *status, void *stream, const int32_t *lengths);

/* ------------------------------------------------------------------------- *
 * (b) the fused train-step loss with a length per column: tk_flipflop_loss_fused_labels_dev's arguments, then `lengths`
 * (required here: the log-partition half of this library is the one with lengths).
 *   lossvector[n] = -score_A / (T_n sharp) + logZ_n / T_n,   grad = grad_scale x grad_scale_per_read[n] x d lossvector[n] / d scores
 * The posterior with lengths (tk_flipflop_posterior_varlen_dev, one wave per column) runs FIRST, on `stream`, into the
 * compact buffers of `aux` -- cat-mod: on a compact copy of the canonical columns --, and kernel A folds logZ_n / T_n into
 * its costs and (d logZ_n) / T_n into the rows [0, T_n) it writes: one launch order, eager or captured.
 *   logz (nbatch) receives the log-partition values (log nbase for a column of length 0);
 *   logz_workspace: tk_flipflop_loss_varlen_aux_bytes(.., 1) bytes;  aux: tk_flipflop_loss_varlen_aux_bytes(.., 0) bytes;
 *   crf_workspace as for (a).  scores and grad 16-byte aligned.
 * ------------------------------------------------------------------------- */
size_t tk_flipflop_loss_varlen_aux_bytes(size_t nblk, size_t nbatch, size_t nbase, size_t ntrans, int which);
int tk_flipflop_loss_fused_varlen_labels_dev(const float *scores, size_t nblk, size_t nbatch, size_t ntrans,
                                             const tk_seq_labels *labels, const int32_t *seqlen,
                                             int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                                             size_t max_seqlen, float sharpfact, float grad_scale,
                                             const float *grad_scale_per_read, float *lossvector,
                                             float *grad, float *logz, void *crf_workspace, size_t crf_workspace_bytes,
                                             void *logz_workspace, size_t logz_workspace_bytes, void *aux, size_t aux_bytes,
                                             uint32_t *status, void *stream, const int32_t *lengths);

/* ------------------------------------------------------------------------- *
 * (c) what a call of (a) or (b) launches, as numbers -- the fields of the lab build's tk_lab_crf_plan, in its order:
 * out[20] = 0 the linear path / 1 the log-domain kernel on every read; the log-domain form's R, W and checkpoint spacing
 * (behind the linear path: the tail launch's); the batch launch's R, W, block length, 2 x weight bias, frame slope, 1 with
 * a row maker, wave-count class; the retry's block length (0: none), 2 x bias, slope, R, W, 1 where its sweeps run side by
 * side; the tail's log-domain R; the slots; the tail launch's R.  form: 0 the plain CRF, 1 cat-mod (per-column factors:
 * what the labels entry points run); max_seqlen 0: nblk + 1; bulk_seqlen 0: unknown.  Returns 0 where the call is refused.
 * ------------------------------------------------------------------------- */
int tk_crf_varlen_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, int form,
                       int want_grad, float sharp, size_t workspace_bytes, size_t *out);

#ifdef __cplusplus
}
#endif
#endif /* TAIYAKI_AMD_LOSS_VARLEN_H */

/*
 * taiyaki_amd_logz_varlen.h -- C ABI of the flip-flop log-partition function on the MI355X (gfx950) for batches whose
 * columns have different TIME lengths, on the transfer-matrix kernels (kernel B): the training-shape counterpart of
 * tk_flipflop_posterior_varlen_dev (taiyaki_amd_decode_varlen.h: one wave per column, nblk serial steps, the basecaller's
 * short reads).  A library of its own (libtaiyaki_amd_logz_varlen.so: the flip-flop ABI is pinned) -- logz_kernels.hip
 * compiled a second time with -DTK_LOGZ_VARLEN (LogzWs::lengths, the kernels' VL = true instantiations) and, for the fused
 * entry, kernel A's objects of libtaiyaki_amd_loss_varlen.so as they are.  It shares the conventions of
 * taiyaki_amd_flipflop.h: device pointers plus a stream, nothing allocated or synchronised inside, a nullable status word
 * with that header's bits and counts.
 *
 *   lengths (nbatch) int32 on the device: the rows of column n, T_n, clamped to [0, nblk] where it is read.
 *
 * Three launches, as for tk_flipflop_logz_dev, with the chunk length, the transfer form and the super that call takes
 * at (nblk, nbatch); a shape it refuses (too many chunks for the middle kernel's LDS image) is TK_ERR_UNSUPPORTED here
 * too, before anything is launched.  A lane folds, chains and writes a row only where the row lies inside its own
 * column's length (a select, never a masked weight); a wave whose 64 columns all end before its chunk loads nothing.
 * Results repeat bit for bit and do not depend on which 64-column group a column sits in; they do depend on
 * (nblk, nbatch) through the chunk length, as the fixed-length operator's do.
 */
#ifndef TAIYAKI_AMD_LOGZ_VARLEN_H
#define TAIYAKI_AMD_LOGZ_VARLEN_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_*, TK_STATUS_*, tk_seq_labels */

#ifdef __cplusplus
extern "C" {
#endif

/* The workspace of (a): tk_flipflop_logz_workspace_bytes at the same shape; 0 for an nbase outside 1..4. */
size_t tk_flipflop_logz_varlen_workspace_bytes(size_t nblk, size_t nbatch, size_t nbase);

/* ------------------------------------------------------------------------- *
 * (a) log-partition and posterior transition probabilities with a length per column: the contract of
 * tk_flipflop_posterior_varlen_dev.
 *   scores (nblk, nbatch, 2 nbase (nbase + 1)) f32, 16-byte aligned
 *   trans  the same shape, 16-byte aligned, or NULL (the log-partition alone: no posterior launch): rows [0, T_n) of
 *          column n hold d logZ / d scores of scores[:T_n, n:n+1]; every row beyond is WRITTEN, as exactly 0
 *   logz   (nbatch) f32: the column's log-partition (log nbase for a column of length 0)
 * Scores beyond a column's length reach no output (a NaN there included).  TK_STATUS_NONFINITE_SCORE (logz) /
 * TK_STATUS_NONFINITE_GRAD (trans, rows inside a length only) are OR-ed into *status as tk_flipflop_logz_dev does.
 * lengths == NULL: every column has nblk rows -- bit for bit what tk_flipflop_logz_dev gives.  nbase 1..4.
 * ------------------------------------------------------------------------- */
int tk_flipflop_logz_varlen_dev(const float *scores, const int32_t *lengths, size_t nblk, size_t nbatch, size_t nbase,
                                float *trans, float *logz, void *workspace, size_t workspace_bytes, uint32_t *status,
                                void *stream);

/* ------------------------------------------------------------------------- *
 * (b) the fused train-step loss with a length per column: the arguments, the rule and the launch order of
 * tk_flipflop_loss_fused_varlen_labels_dev (taiyaki_amd_loss_varlen.h) -- the log-partition with lengths FIRST, on
 * `stream`, into the compact buffers of `aux` (cat-mod: on a compact copy of the canonical columns), then kernel A,
 * which folds logZ_n / T_n into its costs and (d logZ_n) / T_n into the rows [0, T_n) it writes; eager or captured.
 * The log-partition call is (a).
 *   logz_workspace: tk_flipflop_loss_varlen_blocks_aux_bytes(.., 1) bytes;  aux: tk_flipflop_loss_varlen_blocks_aux_bytes(.., 0)
 *   bytes (what tk_flipflop_loss_varlen_aux_bytes(.., 0) gives);  0 for any other `which`, an nbase outside 1..4 or
 *   ntrans below the canonical columns.
 * A shape (a) refuses is TK_ERR_UNSUPPORTED before anything is launched.
 * ------------------------------------------------------------------------- */
size_t tk_flipflop_loss_varlen_blocks_aux_bytes(size_t nblk, size_t nbatch, size_t nbase, size_t ntrans, int which);
int tk_flipflop_loss_fused_varlen_blocks_labels_dev(const float *scores, size_t nblk, size_t nbatch, size_t ntrans,
                                                    const tk_seq_labels *labels, const int32_t *seqlen,
                                                    int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                                                    size_t max_seqlen, float sharpfact, float grad_scale,
                                                    const float *grad_scale_per_read, float *lossvector,
                                                    float *grad, float *logz, void *crf_workspace, size_t crf_workspace_bytes,
                                                    void *logz_workspace, size_t logz_workspace_bytes, void *aux, size_t aux_bytes,
                                                    uint32_t *status, void *stream, const int32_t *lengths);

#ifdef __cplusplus
}
#endif
#endif /* TAIYAKI_AMD_LOGZ_VARLEN_H */

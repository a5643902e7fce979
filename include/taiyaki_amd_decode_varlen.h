/*
 * taiyaki_amd_decode_varlen.h -- C ABI of the basecaller's decode operators on the MI355X (gfx950) for batches whose
 * columns have different lengths: what lets reads shorter than one chunk be called as ONE batch of zero-padded columns
 * (the network half is taiyaki_amd_rnn_varlen.h).  A library of its own (libtaiyaki_amd_decode_varlen.so: the flip-flop
 * and basecall ABIs are pinned); it shares the conventions of taiyaki_amd_basecall.h: device pointers plus a stream,
 * nothing allocated or synchronised inside, a nullable status word, results that do not depend on the batch a column is
 * launched in and repeat bit for bit (one wavefront per column, no atomics on data).
 *
 *   lengths (nbatch) int32 on the device: the rows of column n, clamped to [0, nblk] where it is read.
 */
#ifndef TAIYAKI_AMD_DECODE_VARLEN_H
#define TAIYAKI_AMD_DECODE_VARLEN_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_basecall.h" /* TK_OK, TK_ERR_*, TK_STATUS_CHUNK_PLAN, TK_STATUS_NONFINITE_* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * (a) reads normalised into zero-padded columns: column j is read r = read_index[j]
 *   signal, sig_off, nread, nsignal, shift, scale   as for tk_basecall_gather_chunks_dev (the call's concatenated
 *                 signals and per-read parameters)
 *   read_index    (ncol) int32
 *   columns       (tmax, ncol, 1) f32: rows [0, len_r) of column j = (x - shift[r]) / scale[r], IEEE float32 subtract
 *                 and divide (the float32 contract of taiyaki_amd_basecall.h: bit for bit numpy's result on a float32
 *                 array); every row beyond is exactly 0.  Where shift[r] or scale[r] is NaN the column is all zeros.
 *   lengths       (ncol) int32: len_r (tmax for a longer read)
 * A read longer than tmax sets TK_STATUS_CHUNK_PLAN in *status (the basecall library's status word) and gives its
 * first tmax samples; so does a read_index entry outside [0, nread), whose column is zeros of length 0.  A tiled
 * transpose: coalesced reads along the signal, coalesced writes along the columns.
 * ------------------------------------------------------------------------- */
int tk_basecall_gather_columns_dev(const float *signal, const int64_t *sig_off, size_t nread, size_t nsignal,
                                   const float *shift, const float *scale, const int32_t *read_index, size_t ncol,
                                   size_t tmax, float *columns, int32_t *lengths, uint32_t *status, void *stream);

/* The workspace of (b) and of (c) at this shape (the larger of the two: either call takes it), 16-byte aligned; 0 for
 * an nbase outside 1..4. */
size_t tk_decode_varlen_workspace_bytes(size_t nblk, size_t nbatch, size_t nbase);

/* ------------------------------------------------------------------------- *
 * (b) path-only Viterbi with a length per column
 *   scores (nblk, nbatch, 2 nbase (nbase + 1)) f32; path (nblk + 1, nbatch) int64
 * Rows [0, lengths[n]] of column n are bit for bit what tk_flipflop_viterbi_dev gives on scores[:lengths[n], n:n+1]
 * (one fp32 add per candidate, the first index wins a tie); every row beyond repeats path[lengths[n], n], so a tail
 * that walks all nblk + 1 rows finds no move there.  A column of length 0 is all zeros.  nbase 1..4.
 * ------------------------------------------------------------------------- */
int tk_flipflop_viterbi_varlen_dev(const float *scores, const int32_t *lengths, size_t nblk, size_t nbatch,
                                   size_t nbase, int64_t *path, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* ------------------------------------------------------------------------- *
 * (c) posterior transition probabilities with a length per column
 *   trans (nblk, nbatch, 2 nbase (nbase + 1)) f32: rows [0, lengths[n]) of column n hold d logZ / d scores of
 *         scores[:lengths[n], n:n+1] -- what tk_flipflop_logz_dev writes as `grad` for that column alone (paths start
 *         in a flip state and end anywhere); every row beyond is exactly 0
 *   logz  (nbatch) f32 or NULL: the column's log-partition (log nbase for a column of length 0)
 * Forward and backward sweeps in the linear domain, each row's weights exp(s - row maximum), the state vectors
 * rescaled by exact powers of two at every step; every row of `trans` is normalised by its own sum.
 * TK_STATUS_NONFINITE_SCORE (logz) / TK_STATUS_NONFINITE_GRAD (trans) of taiyaki_amd_flipflop.h are OR-ed into *status
 * on a non-finite result (non-finite scores, or scores so far apart that a whole state vector underflows).  nbase 1..4.
 * ------------------------------------------------------------------------- */
int tk_flipflop_posterior_varlen_dev(const float *scores, const int32_t *lengths, size_t nblk, size_t nbatch,
                                     size_t nbase, float *trans, float *logz, void *workspace,
                                     size_t workspace_bytes, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TAIYAKI_AMD_DECODE_VARLEN_H */

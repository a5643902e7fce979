/*
 * taiyaki_amd_rnn_wide.h -- C ABI of the LSTM and GRU recurrences on the MI355X (gfx950) at EVERY batch width.  A
 * library of its own (libtaiyaki_amd_rnn_wide.so: the flip-flop ABI, taiyaki_amd_rnn_varlen.h and
 * taiyaki_amd_rnn_varlen_train.h are pinned); it shares their conventions, result codes and status bits.  The kernels
 * are those of taiyaki_amd_rnn_varlen_train.h and taiyaki_amd_rnn_varlen.h, built a fourth time from the same source
 * (csrc/lstm_kernels.hip, csrc/gru_kernels.hip) with the tensors' columns per time step as an argument of their own.
 *
 * Why.  The recurrences are persistent launches whose workgroups wait on each other, so a launch is admitted only
 * where its grid fits one workgroup per CU: on 256 CUs the LSTM at size 384 up to 128 columns, at 256 up to 256, at 192
 * and below up to 512; the GRU at 256 and 384 up to 256, at 192 up to 512 (at 128 and below it takes any batch).  The
 * columns of a batch are independent in the recurrence.  A wider batch is therefore run as SLABS of columns: several
 * admitted launches, each working in place on a window of columns of the whole-batch tensors.
 *
 * The slab rule.  S is the widest batch the cell's admission rule admits at (size, cu_count).  Slab k is the columns
 * [k S, min((k + 1) S, nbatch)).  Every slab is planned on its own width by the rule of the existing calls, so the
 * last, narrower slab may run another instantiation of the kernel than the full ones.  Every slab is preceded by the
 * zeroing of the granules it polls, in the one workspace that all slabs share.
 *
 * Launch order, part of the contract.  The slabs are launched in order on the caller's ONE stream, each behind the
 * one before: never on two streams, never as parallel branches of a graph.  Two persistent grids that together exceed
 * the CU count can wait on each other for ever, and the slabs share the workspace.  Captured into a hipGraph the call
 * is a linear chain of nodes.  A caller that runs two of these calls at once (two streams, two layers) breaks the same
 * rule: it must not.
 *
 * What equals what, bit for bit.  Slab k's rows of every output are what the existing call writes when it is handed
 * contiguous copies of that slab's columns at the same cu_count: tk_lstm_forward_varlen_save_dev /
 * tk_lstm_backward_varlen_dev / tk_gru_forward_varlen_save_dev / tk_gru_backward_varlen_dev, and, with NULL for the
 * saved activations, tk_lstm_forward_varlen_dev / tk_gru_forward_varlen_dev.  With lengths NULL these are in turn the
 * plain pair.  At nbatch <= S the call IS the existing call.
 *
 *   gx, w_hh, b_hh, lengths, y, gates, cell, q, dy, dgates, dq, nblk, nbatch, size, reverse: as in
 *     taiyaki_amd_rnn_varlen_train.h; the tensors are the whole batch's, (nblk, nbatch, .) contiguous.  lengths may be
 *     NULL: every column has nblk steps.
 *   The forwards take NULL for BOTH saved tensors (gates and cell; gates and q): nothing is saved, y is the only
 *     output.  One of the two NULL alone is TK_ERR_BAD_ARG.
 *
 * tk_rnn_wide_slab: S at (kind, nbatch, size, cu_count), or nbatch where one launch admits the batch; 0 where the
 *   kernels do not run.  Tests and tools read the cut from here; they do not infer it from the shape.
 * tk_rnn_wide_workspace_bytes: the workspace of both calls of `kind` (TK_RNN_KIND_LSTM / TK_RNN_KIND_GRU of
 *   taiyaki_amd_rnn_varlen.h): what tk_rnn_varlen_train_workspace_bytes returns at the widest slab, min(nbatch, S)
 *   columns.  0 where size is not one the kernels cover, where nbatch is 0 or cu_count <= 0, where a group of the size
 *   does not fit cu_count CUs, or for an unknown kind; never 0 otherwise, whatever nbatch.
 *
 * The same cu_count goes to the calls; it must not exceed the device's CU count.  TK_STATUS_RNN_TIMEOUT in *status if a
 * workgroup's wait for its group ran out of time.  Nothing is allocated or synchronised inside.  Result codes:
 * TK_ERR_BAD_ARG, TK_ERR_UNSUPPORTED, TK_ERR_WORKSPACE, TK_ERR_LAUNCH, as for tk_lstm_backward_varlen_dev.  A launch
 * error in slab k returns at once: no further slab is started, and the rows of slab k and beyond are not valid.
 */
#ifndef TAIYAKI_AMD_RNN_WIDE_H
#define TAIYAKI_AMD_RNN_WIDE_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_rnn_varlen.h" /* TK_RNN_KIND_*; TK_OK, TK_ERR_*, TK_STATUS_RNN_TIMEOUT */

#ifdef __cplusplus
extern "C" {
#endif

size_t tk_rnn_wide_workspace_bytes(int kind, size_t nbatch, size_t size, int cu_count);

size_t tk_rnn_wide_slab(int kind, size_t nbatch, size_t size, int cu_count);

int tk_lstm_forward_wide_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                             size_t size, int reverse, int cu_count, float *y, float *gates, float *cell,
                             void *workspace, size_t workspace_bytes, uint32_t *status, void *stream);

int tk_lstm_backward_wide_dev(const float *w_hh, const float *gates, const float *cell, const float *dy,
                              const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                              int cu_count, float *dgates, void *workspace, size_t workspace_bytes, uint32_t *status,
                              void *stream);

int tk_gru_forward_wide_dev(const float *gx, const float *w_hh, const float *b_hh, const int32_t *lengths, size_t nblk,
                            size_t nbatch, size_t size, int reverse, int cu_count, float *y, float *gates, float *q,
                            void *workspace, size_t workspace_bytes, uint32_t *status, void *stream);

int tk_gru_backward_wide_dev(const float *w_hh, const float *y, const float *gates, const float *q, const float *dy,
                             const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                             int cu_count, float *dgates, float *dq, void *workspace, size_t workspace_bytes,
                             uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif

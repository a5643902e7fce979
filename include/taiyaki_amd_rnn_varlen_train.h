/*
 * taiyaki_amd_rnn_varlen_train.h -- C ABI of the LSTM and GRU recurrences on the MI355X (gfx950) for TRAINING on batches
 * whose columns have different lengths: the forward that saves its activations, and the backward.  A library of its
 * own (libtaiyaki_amd_rnn_varlen_train.so: the flip-flop ABI and taiyaki_amd_rnn_varlen.h are pinned); it shares their
 * conventions, result codes and status bits.  The kernels are those of tk_lstm_forward_dev / tk_lstm_backward_dev and
 * tk_gru_forward_dev / tk_gru_backward_dev (taiyaki_amd_flipflop.h), built a third time from the same source
 * (csrc/lstm_kernels.hip, csrc/gru_kernels.hip) in their variable-length form.
 *
 *   gx, w_hh, b_hh, y, gates, cell, q, dy, dgates, dq, nblk, nbatch, size, reverse: as for the four existing calls
 *   lengths (nbatch) int32 on the device, 0 <= lengths[n] <= nblk: the steps of column n.  NULL: every column has
 *     nblk steps, and every output is what the existing training pair writes, bit for bit.
 *
 * The rule is that of taiyaki_amd_rnn_varlen.h, extended to the saved tensors and to the backward pass.
 * Forward: for time index t of column n, where t >= lengths[n] the state stays at zero and y, gates and cell (GRU: q)
 * are written as exactly 0; otherwise the step is that of the existing forward.  Every row of every output is written.
 * gx beyond the length is never used, whatever it holds.
 * Backward: where t >= lengths[n] the step writes dgates[t, n, :] = 0 (GRU: dq = 0 as well) and hands on a zero
 * recurrent gradient (dh = 0; LSTM: dc = 0 as well), publishing its granules like any other step; otherwise it is the
 * step of the existing backward.  The mask is a select: dy and the saved rows beyond the length are never used, so a
 * NaN there reaches no output.  (With reverse != 0 the backward reaches the padding after the column's real steps,
 * with a carried gradient that is not 0: masking dy alone would not do.)
 * No workgroup leaves early in either call: a launch costs nblk steps.
 *
 * Parameter and input gradients need no call of their own: dgates (dq) and y are 0 beyond the lengths, so
 * tk_lstm_weight_grad_dev, or the GEMMs dgates^T x, dgates^T (y shifted by a step), dgates W_ih and the sums over
 * dgates, run on the whole padded tensors, give the sums over every column's own steps.  The one requirement on the
 * caller: x must be FINITE in the padding (0 * NaN is NaN).
 *
 * tk_rnn_varlen_train_workspace_bytes: the workspace of both calls of `kind` (TK_RNN_KIND_LSTM / TK_RNN_KIND_GRU of
 * taiyaki_amd_rnn_varlen.h) at (nbatch, size) on a device with cu_count CUs: the backward's bound, what
 * tk_lstm_workspace_bytes / tk_gru_workspace_bytes return; 0 where the kernels do not run (an unknown kind included),
 * never 0 where they do.  The same cu_count goes to the calls.  TK_STATUS_RNN_TIMEOUT in *status if a workgroup's wait
 * for its group ran out of time.  Nothing is allocated or synchronised inside; the calls can be captured into a
 * hipGraph.  Result codes: TK_ERR_BAD_ARG (a NULL pointer other than lengths, a workspace that is not 16-byte
 * aligned), TK_ERR_UNSUPPORTED, TK_ERR_WORKSPACE, TK_ERR_LAUNCH, as for tk_lstm_backward_dev.
 */
#ifndef TAIYAKI_AMD_RNN_VARLEN_TRAIN_H
#define TAIYAKI_AMD_RNN_VARLEN_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_rnn_varlen.h" /* TK_RNN_KIND_*; TK_OK, TK_ERR_*, TK_STATUS_RNN_TIMEOUT */

#ifdef __cplusplus
extern "C" {
#endif

size_t tk_rnn_varlen_train_workspace_bytes(int kind, size_t nbatch, size_t size, int cu_count);

int tk_lstm_forward_varlen_save_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk,
                                    size_t nbatch, size_t size, int reverse, int cu_count, float *y, float *gates,
                                    float *cell, void *workspace, size_t workspace_bytes, uint32_t *status,
                                    void *stream);

int tk_lstm_backward_varlen_dev(const float *w_hh, const float *gates, const float *cell, const float *dy,
                                const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                                int cu_count, float *dgates, void *workspace, size_t workspace_bytes, uint32_t *status,
                                void *stream);

int tk_gru_forward_varlen_save_dev(const float *gx, const float *w_hh, const float *b_hh, const int32_t *lengths,
                                   size_t nblk, size_t nbatch, size_t size, int reverse, int cu_count, float *y,
                                   float *gates, float *q, void *workspace, size_t workspace_bytes, uint32_t *status,
                                   void *stream);

int tk_gru_backward_varlen_dev(const float *w_hh, const float *y, const float *gates, const float *q, const float *dy,
                               const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                               int cu_count, float *dgates, float *dq, void *workspace, size_t workspace_bytes,
                               uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif

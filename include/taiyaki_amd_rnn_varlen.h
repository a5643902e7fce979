/*
 * taiyaki_amd_rnn_varlen.h -- C ABI of the LSTM and GRU recurrences on the MI355X (gfx950) for batches whose columns
 * have different lengths, forward only and with nothing saved for a backward call.  A library of its own
 * (libtaiyaki_amd_rnn_varlen.so: the flip-flop ABI is pinned); it shares that header's conventions, result codes and
 * status bits.  The kernels are those of tk_lstm_forward_dev and tk_gru_forward_dev (taiyaki_amd_flipflop.h), built a
 * second time from the same source (csrc/lstm_kernels.hip, csrc/gru_kernels.hip) in their variable-length form.
 *
 *   gx, w_hh, b_hh, y, nblk, nbatch, size, reverse: as for tk_lstm_forward_dev / tk_gru_forward_dev
 *   lengths (nbatch) int32 on the device, 0 <= lengths[n] <= nblk: the steps of column n.  NULL: every column has
 *     nblk steps, and y is what the existing forward writes, bit for bit.
 *
 * The rule, for time index t of column n in either direction: where t >= lengths[n] the step leaves the state at
 * zero (h = 0; LSTM: c = 0), writes y[t, n, :] = 0 and hands h = 0 to its group like any other step; otherwise it is
 * the step of the existing forward.  So forward in time rows [0, lengths[n]) of column n are what the column gives
 * run alone over lengths[n] steps, and with reverse != 0 the state stays at the initial zero until t = lengths[n] - 1:
 * the rows are what the column gives run alone from its own last step.  Every row of y is written.  No workgroup
 * leaves early: a launch costs nblk steps, so nblk should be the longest length of the launch.
 *
 * Only y is written: there are no gates, cell or q arguments and nothing is allocated for them.
 *
 * tk_rnn_varlen_workspace_bytes: the workspace of a launch of `kind` at (nbatch, size) on a device with cu_count CUs,
 * 0 where the kernels do not run (an unknown kind included); never 0 where they do.  The admission rules are those of
 * tk_lstm_workspace_bytes and tk_gru_workspace_bytes, and the same cu_count goes to the call.
 * TK_STATUS_RNN_TIMEOUT in *status if a workgroup's wait for its group ran out of time.  Nothing is allocated or
 * synchronised inside; the calls can be captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_RNN_VARLEN_H
#define TAIYAKI_AMD_RNN_VARLEN_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_*, TK_STATUS_RNN_TIMEOUT */

#define TK_RNN_KIND_LSTM 0
#define TK_RNN_KIND_GRU 1

#ifdef __cplusplus
extern "C" {
#endif

size_t tk_rnn_varlen_workspace_bytes(int kind, size_t nbatch, size_t size, int cu_count);

int tk_lstm_forward_varlen_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                               size_t size, int reverse, int cu_count, float *y, void *workspace,
                               size_t workspace_bytes, uint32_t *status, void *stream);

int tk_gru_forward_varlen_dev(const float *gx, const float *w_hh, const float *b_hh, const int32_t *lengths,
                              size_t nblk, size_t nbatch, size_t size, int reverse, int cu_count, float *y,
                              void *workspace, size_t workspace_bytes, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif

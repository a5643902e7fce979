/*
 * taiyaki_amd_lstm_local.h -- C ABI of the LSTM recurrence on the MI355X (gfx950) at hidden sizes whose whole W_hh
 * fits the registers of ONE workgroup (size 96: 4 x 96 x 96 floats, 96 per lane at 384 lanes).  A library of its own
 * (libtaiyaki_amd_lstm_local.so: the flip-flop ABI and the other RNN headers are pinned, and their queries keep
 * answering 0 at this size); it shares their conventions and result codes.
 *
 * One workgroup owns every hidden unit of its batch columns, so h moves through LDS only and nothing is handed between
 * workgroups: no workspace, no status word, no bounded wait, no co-residency condition, any batch width in one launch
 * (the grid may exceed the CU count).  The cell is that of tk_lstm_forward_dev: gate order i, f, g, o; h0 = c0 = 0.
 *
 *   gx      (nblk, nbatch, 4 size)  x W_ih^T + b_ih + b_hh, the caller's GEMM
 *   w_hh    (4 size, size)
 *   lengths (nbatch) device int32, or NULL: column n has lengths[n] steps (NULL: nblk).  At and beyond a column's
 *           length y, gates, cell and dgates are written as 0 and the state handed on is 0, as in
 *           taiyaki_amd_rnn_varlen_train.h; what gx and dy hold there is read and never used.
 *   y       (nblk, nbatch, size)    h
 *   gates   (nblk, nbatch, 4 size)  the activations i, f, g, o;  cell (nblk, nbatch, size)  c.  The forward takes NULL
 *           for BOTH: nothing is saved, y is the only output.  One of the two NULL alone is TK_ERR_BAD_ARG.
 *   dy      (nblk, nbatch, size)    dL/dy;  dgates (nblk, nbatch, 4 size)  dL/d(pre-activation)
 *   reverse != 0: the recurrence runs from the last time step, on tensors in time order
 *
 * Every sum runs in an order that depends on the size alone: a column's y, gates, cell and dgates are the same bits
 * whatever nbatch is, whatever the other columns hold and however many columns a workgroup took.
 *
 * tk_lstm_local_supported: 1 where the kernels are built for the size (96), else 0.
 * tk_lstm_local_columns: the batch columns per workgroup of a launch at (nbatch, size, cu_count): 1 where every column
 *   gets a CU of its own (nbatch <= cu_count), else 2; 0 for an unsupported size, nbatch 0 or cu_count <= 0.
 *
 * Checks, in this order, before anything is launched: a NULL required pointer, gx, y, gates, cell, dy or dgates not
 * 16-byte aligned, nblk or nbatch beyond INT32_MAX: TK_ERR_BAD_ARG; an unsupported size, nbatch 0 or cu_count <= 0:
 * TK_ERR_UNSUPPORTED; nblk 0: nothing to do, TK_OK.  TK_ERR_LAUNCH if the launch fails.  Nothing is allocated or
 * synchronised inside; the calls can be captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_LSTM_LOCAL_H
#define TAIYAKI_AMD_LSTM_LOCAL_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_lstm_local_supported(size_t size);

int tk_lstm_local_columns(size_t nbatch, size_t size, int cu_count);

int tk_lstm_local_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                              size_t size, int reverse, int cu_count, float *y, float *gates, float *cell,
                              void *stream);

int tk_lstm_local_backward_dev(const float *w_hh, const float *gates, const float *cell, const float *dy,
                               const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                               int cu_count, float *dgates, void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_lstm_local_lab.so). */
/* force the batch columns per workgroup: 1 or 2 (0: the rule) */
void tk_lab_lstm_local_cols(int cols);
#endif

#ifdef __cplusplus
}
#endif

#endif

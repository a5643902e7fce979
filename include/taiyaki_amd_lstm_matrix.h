/*
 * taiyaki_amd_lstm_matrix.h -- C ABI of the LSTM forward recurrence that saves nothing, on the matrix cores of the
 * MI355X (gfx950), at hidden size 96 and for batches of thousands of columns: the basecaller's network pass.  A library
 * of its own (libtaiyaki_amd_lstm_matrix.so: the flip-flop ABI and the other RNN headers are pinned); it shares their
 * conventions and result codes.
 *
 * One workgroup owns every hidden unit of 16 batch columns and computes W_hh h as v_mfma_f32_16x16x32_bf16 on float32
 * operands split three ways into bf16, so float32 accuracy is kept.  h moves through LDS only and nothing is handed
 * between workgroups: no workspace, no status word, no bounded wait, no co-residency condition, any batch width in one
 * launch of ceil(nbatch / 16) workgroups.  The cell is that of tk_lstm_forward_dev: gate order i, f, g, o; h0 = c0 = 0.
 *
 *   gx      (nblk, nbatch, 4 size)  x W_ih^T + b_ih + b_hh, the caller's GEMM
 *   w_hh    (4 size, size)
 *   lengths (nbatch) device int32, or NULL: column n has lengths[n] steps (NULL: nblk).  At and beyond a column's
 *           length y is written as 0 and the state handed on is 0, as in taiyaki_amd_lstm_local.h; what gx holds there
 *           (a NaN too) is read and never used.
 *   y       (nblk, nbatch, size)    h, the only output
 *   reverse != 0: the recurrence runs from the last time step, on tensors in time order
 *
 * Every sum runs in one fixed order: a column's y is a function of that column's gx, its length and w_hh alone, the
 * same bits whatever nbatch is, whatever the other columns hold and whichever of a workgroup's 16 places the column
 * takes.  They are not the bits of tk_lstm_local_forward_dev, whose sums run in another order.
 *
 * tk_lstm_matrix_supported: 1 where the kernel is built for the size (96), else 0.
 * tk_lstm_matrix_columns: the batch columns per workgroup at the size (16 at 96), 0 for an unsupported size.
 *
 * Checks, in this order, before anything is launched: a NULL required pointer (gx, w_hh, y), gx or y not 16-byte
 * aligned, nblk or nbatch beyond INT32_MAX: TK_ERR_BAD_ARG; an unsupported size or nbatch 0: TK_ERR_UNSUPPORTED; nblk 0:
 * nothing to do, TK_OK.  TK_ERR_LAUNCH if the launch fails.  Nothing is allocated or synchronised inside; the call can be
 * captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_LSTM_MATRIX_H
#define TAIYAKI_AMD_LSTM_MATRIX_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_lstm_matrix_supported(size_t size);

int tk_lstm_matrix_columns(size_t size);

int tk_lstm_matrix_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                               size_t size, int reverse, float *y, void *stream);

#ifdef __cplusplus
}
#endif

#endif

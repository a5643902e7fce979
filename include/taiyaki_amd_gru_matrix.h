/*
 * taiyaki_amd_gru_matrix.h -- C ABI of the GRU forward recurrence that saves nothing, on the matrix cores of the MI355X
 * (gfx950), at hidden size 96 and for batches of thousands of columns: the basecaller's network pass through an
 * mGru_flipflop.  A library of its own (libtaiyaki_amd_gru_matrix.so: the flip-flop ABI and the other RNN headers are
 * pinned); it shares their conventions and result codes.
 *
 * One workgroup owns every hidden unit of 16 batch columns and computes W_hh h as v_mfma_f32_16x16x32_bf16 on float32
 * operands split three ways into bf16, so float32 accuracy is kept.  h moves through LDS only and nothing is handed
 * between workgroups: no workspace, no status word, no bounded wait, no co-residency condition, any batch width in one
 * launch of ceil(nbatch / 16) workgroups.  The cell is that of tk_gru_forward_dev: gate order r, z, n; h0 = 0; with
 * a = W_hh h_prev
 *   r = sigmoid(gx_r + a_r + bhh_r), z = sigmoid(gx_z + a_z + bhh_z), q = a_n + bhh_n, n = tanh(gx_n + r q),
 *   h = (1 - z) n + z h_prev.
 *
 *   gx      (nblk, nbatch, 3 size)  x W_ih^T + b_ih, the caller's GEMM
 *   w_hh    (3 size, size)
 *   b_hh    (3 size)                its third slab sits inside the reset product, so it cannot be folded into gx
 *   lengths (nbatch) device int32, or NULL: column n has lengths[n] steps (NULL: nblk).  At and beyond a column's
 *           length y is written as 0 and the state handed on is 0, as in tk_gru_forward_varlen_dev; what gx holds there
 *           (a NaN too) is read and never used.
 *   y       (nblk, nbatch, size)    h, the only output
 *   reverse != 0: the recurrence runs from the last time step, on tensors in time order
 *
 * Every sum runs in one fixed order: a column's y is a function of that column's gx, its length, w_hh and b_hh alone,
 * the same bits whatever nbatch is, whatever the other columns hold and whichever of a workgroup's 16 places the column
 * takes.  They are not the bits of tk_gru_forward_dev, whose sums run in another order.
 *
 * tk_gru_matrix_supported: 1 where the kernel is built for the size (96), else 0.
 * tk_gru_matrix_columns: the batch columns per workgroup at the size (16 at 96), 0 for an unsupported size.
 *
 * Checks, in this order, before anything is launched: a NULL required pointer (gx, w_hh, b_hh, y), gx or y not 16-byte
 * aligned, nblk or nbatch beyond INT32_MAX: TK_ERR_BAD_ARG; an unsupported size or nbatch 0: TK_ERR_UNSUPPORTED; nblk 0:
 * nothing to do, TK_OK.  TK_ERR_LAUNCH if the launch fails.  Nothing is allocated or synchronised inside; the call can be
 * captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_GRU_MATRIX_H
#define TAIYAKI_AMD_GRU_MATRIX_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_gru_matrix_supported(size_t size);

int tk_gru_matrix_columns(size_t size);

int tk_gru_matrix_forward_dev(const float *gx, const float *w_hh, const float *b_hh, const int32_t *lengths, size_t nblk,
                              size_t nbatch, size_t size, int reverse, float *y, void *stream);

#ifdef __cplusplus
}
#endif

#endif

/*
 * taiyaki_amd_lstm_matrix_sizes.h -- C ABI of the LSTM forward recurrence that saves nothing, on the matrix cores of the
 * MI355X (gfx950), at hidden sizes 384 and 192: the basecaller's network pass at the reference trainer's default --size
 * (384) and at the other size of the main library's 48-unit family.  A library of its own
 * (libtaiyaki_amd_lstm_matrix_sizes.so: the flip-flop ABI and the other RNN headers are pinned, and the size-256 library
 * of taiyaki_amd_lstm_matrix_group.h keeps its bits); it shares their conventions, result codes and status bits.
 *
 * W_hh h is v_mfma_f32_16x16x32_bf16 on float32 operands split three ways into bf16, as in taiyaki_amd_lstm_matrix.h, so
 * float32 accuracy is kept.  The split W_hh fits no single CU, so a GROUP of size / 32 workgroups (12 at 384, 6 at 192)
 * holds it, 32 hidden units each, and shares a set of batch columns (tk_lstm_matrix_sizes_columns: 16 at 384, 16 or 32
 * at 192); the members hand h to each other every step through tagged granules in the workspace.  The launch is
 * therefore persistent: every workgroup must be resident, groups x size / 32 <= cu_count, and a wider batch runs INSIDE
 * the call as slabs of tk_lstm_matrix_sizes_slab columns, one launch behind the other on the caller's one stream, each
 * in place on a window of columns of the whole-batch tensors and each preceded by the zeroing of the granules it polls
 * (the launch order of taiyaki_amd_rnn_wide.h, and its rule: never two of these calls at once).  The cell is that of
 * tk_lstm_forward_dev: gate order i, f, g, o; h0 = c0 = 0.
 *
 *   gx      (nblk, nbatch, 4 size)  x W_ih^T + b_ih + b_hh, the caller's GEMM
 *   w_hh    (4 size, size)
 *   lengths (nbatch) device int32, or NULL: column n has lengths[n] steps (NULL: nblk).  At and beyond a column's
 *           length y is written as 0 and the state handed on is 0, as in taiyaki_amd_lstm_matrix.h; what gx holds there
 *           (a NaN too) is read and never used.
 *   y       (nblk, nbatch, size)    h, the only output
 *   reverse != 0: the recurrence runs from the last time step, on tensors in time order
 *   cu_count   the CUs the launch may fill; it must not exceed the device's CU count
 *   workspace  device memory, 16-byte aligned, at least tk_lstm_matrix_sizes_workspace_bytes(nbatch, size, cu_count)
 *   status     a device word; TK_STATUS_RNN_TIMEOUT is OR-ed in if a workgroup's wait for its group ran out of time (the
 *              whole grid then leaves, and y is not valid)
 *
 * Every sum runs in one fixed order: a column's y is a function of that column's gx, its length and w_hh alone, the
 * same bits whatever nbatch and cu_count are, whatever the other columns hold, whichever place of a group the column
 * takes and however many columns a group is built for.  So slab k's rows are bit for bit those of the call on copies of
 * its columns.  They are not the bits of tk_lstm_forward_dev, whose sums run in another order.
 *
 * tk_lstm_matrix_sizes_supported: 1 where the kernel is built for the size (192, 384), else 0.
 * tk_lstm_matrix_sizes_columns: the batch columns of a group at the size as built for release, 0 for an unsupported
 *   size.
 * tk_lstm_matrix_sizes_slab: the columns of one launch, (cu_count / (size / 32)) x columns; 0 where no launch fits (fewer
 *   than size / 32 CUs) or the size is unsupported.
 * tk_lstm_matrix_sizes_workspace_bytes: the granules of the widest launch of the call, min(nbatch, slab) columns: the
 *   same from one slab on.  0 where the size is unsupported, nbatch is 0 or no launch fits.
 *
 * Checks, in this order, before anything is launched: a NULL required pointer (gx, w_hh, y), gx or y not 16-byte
 * aligned, nblk or nbatch beyond INT32_MAX, then workspace or status NULL, workspace not 16-byte aligned:
 * TK_ERR_BAD_ARG; an unsupported size, nbatch 0 or no launch that fits cu_count: TK_ERR_UNSUPPORTED; workspace_bytes too
 * small: TK_ERR_WORKSPACE; nblk 0: nothing to do, TK_OK.  TK_ERR_LAUNCH if a launch fails: no further slab is started.
 * Nothing is allocated or synchronised inside; the call can be captured into a hipGraph, where it is a linear chain of
 * nodes.
 */
#ifndef TAIYAKI_AMD_LSTM_MATRIX_SIZES_H
#define TAIYAKI_AMD_LSTM_MATRIX_SIZES_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_*, TK_STATUS_RNN_TIMEOUT */

#ifdef __cplusplus
extern "C" {
#endif

int tk_lstm_matrix_sizes_supported(size_t size);

int tk_lstm_matrix_sizes_columns(size_t size);

size_t tk_lstm_matrix_sizes_slab(size_t size, int cu_count);

size_t tk_lstm_matrix_sizes_workspace_bytes(size_t nbatch, size_t size, int cu_count);

int tk_lstm_matrix_sizes_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk,
                                     size_t nbatch, size_t size, int reverse, int cu_count, float *y, void *workspace,
                                     size_t workspace_bytes, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif

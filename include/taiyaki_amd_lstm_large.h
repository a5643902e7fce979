/*
 * taiyaki_amd_lstm_large.h -- C ABI of the LSTM recurrence on the MI355X (gfx950) at hidden size 512.  A library of its
 * own (libtaiyaki_amd_lstm_large.so: the flip-flop ABI and the other RNN headers are pinned, and their queries keep
 * answering 0 at this size); it shares their conventions and result codes.  The kernels are those of
 * tk_lstm_forward_dev / tk_lstm_backward_dev (csrc/lstm_kernels.hip, built -DTK_LSTM_LARGE) and so is the hand-off
 * between workgroups: gate order i, f, g, o; h0 = c0 = 0.  One pair of entries serves every form: with or without
 * per-column lengths, the activations saved or not, any batch width.
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
 *   status  one device word: TK_STATUS_RNN_TIMEOUT is OR-ed in if a workgroup waited past its time budget
 *
 * Geometry.  A workgroup owns 32 hidden units (4 x 32 x 512 floats of W_hh in registers, 128 per lane at 512 lanes) and
 * C batch columns; the 16 workgroups that share C columns are a group and wait on each other at every step, so a launch
 * is admitted only where groups x 16 <= cu_count.  C = 4 where ceil(nbatch / 4) x 16 <= cu_count (nbatch <= 64 on 256
 * CUs), else C = 8 where ceil(nbatch / 8) x 16 <= cu_count (nbatch <= 128 on 256 CUs).
 *
 * Slabs.  A batch wider than one launch admits runs as slabs of tk_lstm_large_slab columns inside the call, slab k being
 * columns [k S, min((k + 1) S, nbatch)): one admitted launch after the other on the caller's stream, in place, sharing
 * the workspace (as taiyaki_amd_rnn_wide.h).  The first slab is the widest.
 *
 * Every sum runs in a fixed order: two calls give the same bits; lengths NULL and lengths = nblk everywhere give the same
 * bits; y is the same bits with and without the saves; slab k's rows are the bits the call writes on a copy of slab k's
 * columns alone.
 *
 * tk_lstm_large_supported: 1 at size 512, else 0.
 * tk_lstm_large_slab: the widest batch one launch admits at (size, cu_count), or nbatch if that is smaller; 0 where
 *   nothing runs (an unsupported size, nbatch 0, cu_count < 16).
 * tk_lstm_large_workspace_bytes: the backward's granule bytes at the widest slab, 2 x groups x 16 x C x 512 x 8; this
 *   bounds the forward's.  0 where nothing runs.
 *
 * Checks, in this order, before anything is launched: a NULL required pointer, workspace not 16-byte aligned, nblk or
 * nbatch beyond INT32_MAX, one of gates / cell NULL alone: TK_ERR_BAD_ARG; no plan for (nbatch, size, cu_count):
 * TK_ERR_UNSUPPORTED; workspace_bytes below the launch's need: TK_ERR_WORKSPACE; nblk 0: nothing to do, TK_OK.
 * TK_ERR_LAUNCH if a launch fails (no further slab is started).  Nothing is allocated or synchronised inside; the calls
 * can be captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_LSTM_LARGE_H
#define TAIYAKI_AMD_LSTM_LARGE_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_*, TK_STATUS_RNN_TIMEOUT */

#ifdef __cplusplus
extern "C" {
#endif

int tk_lstm_large_supported(size_t size);

size_t tk_lstm_large_slab(size_t nbatch, size_t size, int cu_count);

size_t tk_lstm_large_workspace_bytes(size_t nbatch, size_t size, int cu_count);

int tk_lstm_large_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                              size_t size, int reverse, int cu_count, float *y, float *gates, float *cell,
                              void *workspace, size_t workspace_bytes, uint32_t *status, void *stream);

int tk_lstm_large_backward_dev(const float *w_hh, const float *gates, const float *cell, const float *dy,
                               const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                               int cu_count, float *dgates, void *workspace, size_t workspace_bytes, uint32_t *status,
                               void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_lstm_large_lab.so). */
/* force the batch columns per group: 4 or 8 (0: the rule) */
void tk_lab_lstm_large_cols(int cols);
/* the launch plan at (nbatch, size, cu_count): out[8] = admitted C and groups, U, C, groups, grid, forward and backward
 * granule bytes, as tk_lab_lstm_geometry; 0 where the kernels do not run */
int tk_lab_lstm_large_geometry(size_t nbatch, size_t size, int cu_count, size_t *out);
#endif

#ifdef __cplusplus
}
#endif

#endif

/*
 * taiyaki_amd_lstm_wgrad.h -- C ABI of the LSTM layer's parameter gradients on the MI355X (gfx950): the three
 * results that follow tk_lstm_backward_dev (taiyaki_amd_flipflop.h) in one pass over dG.  A library of its own
 * (libtaiyaki_amd_lstm_wgrad.so: the flip-flop ABI is pinned); it shares that header's conventions and result codes.
 *
 *   dgates (T, N, 4H) = dL/d(gate pre-activation), what tk_lstm_backward_dev wrote
 *   x      (T, N, I)  = the layer's input
 *   y      (T, N, H)  = the layer's forward output (h)
 *   dw_ih  (4H, I) = sum over (t, n) of dgates[t, n, :] (x) x[t, n, :]
 *   dw_hh  (4H, H) = sum over (t, n) of dgates[t, n, :] (x) y[t_prev, n, :]; t_prev = t - 1 (t = 0 adds nothing), for
 *                    reverse != 0 t_prev = t + 1 (t = T - 1 adds nothing); all zeros at T = 1
 *   db     (4H)    = sum over (t, n) of dgates[t, n, :]
 *
 * One GEMM dG^T [x | y shifted | 1] over the T N rows on the float32 matrix cores (csrc/lstm_wgrad.hip): the rows are
 * cut into runs, one workgroup per (output tile, run), whose partial results go to the workspace; a second launch
 * adds them in a fixed order.  No atomics: two calls on the same inputs give the same bits, whatever the workspace
 * held.  Every product chain is a k-ordered float32 fmaf chain of at most 8192 rows.  dgates is read from HBM once.
 *
 * tk_lstm_weight_grad_workspace_bytes: the workspace at this shape on a device with cu_count CUs (a function of its
 * five arguments only), 0 where the kernels do not run (a zero size, T N rows or an output beyond 32-bit indices): the
 * caller then uses GEMMs.  The same cu_count goes to the call.  Nothing is allocated or synchronised inside; the call
 * can be captured into a hipGraph.  Tensors are dense and row-major; 16-byte aligned tensors take the wide loads.
 */
#ifndef TAIYAKI_AMD_LSTM_WGRAD_H
#define TAIYAKI_AMD_LSTM_WGRAD_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

size_t tk_lstm_weight_grad_workspace_bytes(size_t nblk, size_t nbatch, size_t size, size_t insize, int cu_count);

int tk_lstm_weight_grad_dev(const float *dgates, const float *x, const float *y, size_t nblk, size_t nbatch,
                            size_t size, size_t insize, int reverse, int cu_count, float *dw_ih, float *dw_hh,
                            float *db, void *workspace, size_t workspace_bytes, void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_lstm_wgrad_lab.so). */
/* the number of runs the T N rows are cut into (0: the launcher's rule) */
void tk_lab_lstm_wgrad_splits(int splits);
/* the launch plan at a shape: out[8] = output tiles down and across, runs, partial results per run, rows per run, rows
 * per partial result, grid, partial results in the workspace; 0 where the kernels do not run */
int tk_lab_lstm_wgrad_plan(size_t nblk, size_t nbatch, size_t size, size_t insize, int cu_count, size_t *out);
#endif

#ifdef __cplusplus
}
#endif

#endif

/*
 * taiyaki_amd_gru_wgrad.h -- C ABI of the GRU layer's parameter gradients on the MI355X (gfx950): the four results
 * that follow tk_gru_backward_dev (taiyaki_amd_flipflop.h) in one pass over dG and dq.  A library of its own
 * (libtaiyaki_amd_gru_wgrad.so: the flip-flop ABI is pinned); it shares that header's conventions and result codes, and
 * everything but the operands with taiyaki_amd_lstm_wgrad.h.
 *
 *   dgates (T, N, 3H) = dL/dG_x, what tk_gru_backward_dev wrote (the gates r, z, n)
 *   dq     (T, N, H)  = its second result: the hidden side's pre-activation gradient is [dgates[:, :, :2H] | dq]
 *   x      (T, N, I)  = the layer's input
 *   y      (T, N, H)  = the layer's forward output (h)
 *   dw_ih  (3H, I) = sum over (t, n) of dgates[t, n, :] (x) x[t, n, :]
 *   db_ih  (3H)    = sum over (t, n) of dgates[t, n, :]
 *   dw_hh  (3H, H) = sum over (t, n) of [dgates[t, n, :2H] | dq[t, n, :]] (x) y[t_prev, n, :]; t_prev = t - 1 (t = 0
 *                    adds nothing), for reverse != 0 t_prev = t + 1 (t = T - 1 adds nothing); all zeros at T = 1
 *   db_hh  (3H)    = [db_ih[:2H] | sum over (t, n) of dq[t, n, :]]; may be NULL (a frozen bias_hh): nothing is written
 *                    for it and the other three results are the same bits
 *
 * One GEMM A^T [x | y shifted | 1] over the T N rows on the bf16 matrix cores (csrc/gru_wgrad.hip, the kernel of
 * csrc/wgrad_common.h): the output tiles under x's columns read A from dgates, those under y's columns read a 3H-wide A
 * whose columns from 2H on come from dq (chosen per float4: `size` is even, so none lies across the seam).  The rows are
 * cut into runs, one workgroup per (output tile, run), whose partial results go to the workspace; a second launch adds
 * them in a fixed order and copies db_ih[:2H] into db_hh[:2H], which therefore equal it bit for bit.  No atomics: two
 * calls on the same inputs give the same bits, whatever the workspace held.  The x tiles read dgates from HBM once; the
 * y tiles read its first 2H columns and dq.
 *
 * Arithmetic: every float32 operand a is split as it is staged, a = a1 + a2 + a3 with a1 = bf16(a), a2 = bf16(a - a1),
 * a3 = bf16(a - a1 - a2) (round to nearest even; 24 significant bits in three parts of 8), and a product is
 * a1 b1 + a1 b2 + a2 b1 + a2 b2 + a1 b3 + a3 b1: six bf16 MFMAs with float32 accumulation, each part product exact
 * in float32, the three dropped ones below 2^-26 |a b|.  The results are as close to float64 as a float32 GEMM's
 * (tests/test_gru_wgrad.py).  No accumulation chain is longer than 8192 rows.  The bias sums are float32 sums of the
 * float32 values.
 *   - A zero splits into three zeros: rows of dgates and dq that are exactly 0 add exactly 0 whatever x and y hold
 *     there (training with per-column lengths: both are 0 beyond every length).
 *   - A non-finite input gives NaN where a float32 product would give an infinity (Inf - Inf in the split); either
 *     trips the trainer's non-finite check.
 *   - Values below about 2^-108 in magnitude lose their third part, and the second below 2^-117, to bf16 underflow:
 *     their products are then only as accurate as the parts that are left.
 *
 * tk_gru_weight_grad_workspace_bytes: the workspace at this shape on a device with cu_count CUs (a function of its five
 * arguments only), 0 where the kernels do not run (a zero size, an odd `size`, T N rows or an output beyond 32-bit
 * indices): the caller then uses GEMMs.  The same cu_count goes to the call.  A workspace smaller than that gives
 * TK_ERR_WORKSPACE, a shape with no plan TK_ERR_UNSUPPORTED, a NULL (db_hh apart) or a workspace that is not 16-byte
 * aligned TK_ERR_BAD_ARG, and nothing is launched.  Nothing is allocated or synchronised inside; the call can be
 * captured into a hipGraph.  Tensors are dense and row-major; 16-byte aligned tensors take the wide loads.
 */
#ifndef TAIYAKI_AMD_GRU_WGRAD_H
#define TAIYAKI_AMD_GRU_WGRAD_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

size_t tk_gru_weight_grad_workspace_bytes(size_t nblk, size_t nbatch, size_t size, size_t insize, int cu_count);

int tk_gru_weight_grad_dev(const float *dgates, const float *dq, const float *x, const float *y, size_t nblk,
                           size_t nbatch, size_t size, size_t insize, int reverse, int cu_count, float *dw_ih,
                           float *dw_hh, float *db_ih, float *db_hh, void *workspace, size_t workspace_bytes,
                           void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_gru_wgrad_lab.so). */
/* the number of runs the T N rows are cut into (0: the launcher's rule) */
void tk_lab_gru_wgrad_splits(int splits);
/* the launch plan at a shape: out[8] = output tiles down and across, runs, partial results per run, rows per run, rows
 * per partial result, grid, partial results in the workspace (each 3H (I + H) + 4H floats, rounded up to a multiple of
 * four); 0 where the kernels do not run */
int tk_lab_gru_wgrad_plan(size_t nblk, size_t nbatch, size_t size, size_t insize, int cu_count, size_t *out);
/* the loads a call takes at these widths, `aligned`: every operand is 16-byte aligned.  0 = guarded (any shape and
 * alignment), 1 = 16-byte loads of whole tiles (both widths multiples of 128), 2 = 16-byte loads with ragged tiles
 * (both multiples of 4) */
int tk_lab_gru_wgrad_loads(size_t size, size_t insize, int aligned);
#endif

#ifdef __cplusplus
}
#endif

#endif

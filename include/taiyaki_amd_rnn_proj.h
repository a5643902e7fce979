/*
 * taiyaki_amd_rnn_proj.h -- C ABI of a recurrent layer's two projection GEMMs on the MI355X (gfx950): the input
 * projection in front of tk_lstm_forward_dev / tk_gru_forward_dev and the input gradient behind tk_lstm_backward_dev /
 * tk_gru_backward_dev (taiyaki_amd_flipflop.h).  A library of its own (libtaiyaki_amd_rnn_proj.so: the flip-flop ABI
 * is pinned); it shares that header's conventions and result codes.
 *
 *   out (rows, nout) = a (rows, k) . B^T (+ bias (nout)),  rows = T N, B (nout, k) taken from the layer's w_ih (G H, I)
 *
 *   tk_rnn_input_proj_dev   gx = x . w_ih^T + bias   k = I, nout = G H: B's rows are w_ih's rows; bias may be NULL
 *   tk_rnn_input_grad_dev   dx = dG . w_ih           k = G H, nout = I: B's rows are w_ih's columns; no bias
 *
 * One GEMM on the bf16 matrix cores (csrc/rnn_proj.hip) behind a small launch that writes the three bf16 parts of
 * w_ih into the workspace in the order the main kernel reads them (transposed for the gradient).  The images are
 * written by every call: the weights change with every optimiser step, nothing is kept between calls.  No atomics,
 * no split of k across workgroups: two calls on the same inputs give the same bits, whatever the workspace held.
 *
 * Arithmetic: that of taiyaki_amd_lstm_wgrad.h.  Every float32 operand is split a = a1 + a2 + a3 into three bf16 parts
 * (round to nearest even), a product is a1 b1 + (a1 b2 + a2 b1 + a2 b2 + a1 b3 + a3 b1): six bf16 MFMAs with float32
 * accumulation, the leading product and the five corrections in accumulators of their own, added once at the end; the
 * bias is added last, in float32.  k runs in ascending blocks of 16 inside one workgroup.
 *   - Row independence: the bits of an output row are a function of that row of `a`, of w_ih and of the bias only --
 *     not of rows, of the row's position or of the other rows.  The batched, per-column and variable-length paths of
 *     a layer therefore agree bit for bit whatever batch each of them forms.
 *   - A zero splits into three zeros: a row of `a` that is exactly 0 gives exactly 0 + bias.
 *   - A non-finite element of `a` makes its output row non-finite (NaN where a float32 product would give an
 *     infinity) and touches no other row.
 *   - bf16 underflow: as in taiyaki_amd_lstm_wgrad.h.
 *
 * tk_rnn_proj_workspace_bytes: the workspace (the pre-split weight images) for `rows` rows, a function of its four
 * arguments only; 0 where the caller should keep its GEMM: a zero size, rows x max(k, nout) beyond 32-bit indices, a
 * pair of widths outside the rule -- min(k, nout) in {16, 32, 64, 96, 128, 192, 256, 384} (the widths the recurrences
 * admit, I = H) and max(k, nout) three or four times that (the GRU's and the LSTM's gates) -- and, for the gradient
 * form alone (k > nout), fewer than 64000 rows, where the kernel was measured slower than rocBLAS.  The projection
 * form (k < nout) is admitted at every number of rows: training, inference and the variable-length paths of a layer
 * take the same forward projection.  Where it is not 0 the size does not depend on rows.  The entry points themselves
 * run at every number of rows (TK_ERR_UNSUPPORTED for the sizes and widths above only), given the workspace of the
 * same widths at an admitted number of rows.
 *
 * Tensors are dense and row-major.  Nothing is allocated or synchronised inside; the calls can be captured into a
 * hipGraph.  The workspace must be 16-byte aligned (TK_ERR_BAD_ARG otherwise).  `a` takes 16-byte loads where it is
 * 16-byte aligned and guarded 4-byte loads otherwise; w_ih, bias and out need only float alignment.
 */
#ifndef TAIYAKI_AMD_RNN_PROJ_H
#define TAIYAKI_AMD_RNN_PROJ_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

size_t tk_rnn_proj_workspace_bytes(size_t rows, size_t k, size_t nout, int cu_count);

/* gx (rows, gates_size) = x (rows, insize) . w_ih (gates_size, insize)^T + bias (gates_size; NULL: none) */
int tk_rnn_input_proj_dev(const float *x, const float *w_ih, const float *bias, size_t rows, size_t insize,
                          size_t gates_size, int cu_count, float *gx, void *workspace, size_t workspace_bytes,
                          void *stream);

/* dx (rows, insize) = dgates (rows, gates_size) . w_ih (gates_size, insize) */
int tk_rnn_input_grad_dev(const float *dgates, const float *w_ih, size_t rows, size_t insize, size_t gates_size,
                          int cu_count, float *dx, void *workspace, size_t workspace_bytes, void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_rnn_proj_lab.so). */
/* the launch plan at a shape: out[6] = rows per tile, columns per tile, row tiles, column tiles, k blocks, grid; 0
 * where tk_rnn_proj_workspace_bytes is 0 */
int tk_lab_rnn_proj_plan(size_t rows, size_t k, size_t nout, int cu_count, size_t *out);
#endif

#ifdef __cplusplus
}
#endif

#endif

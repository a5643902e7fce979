/*
 * taiyaki_amd_conv_strided.h -- C ABI of the mLstm models' third layer, Convolution(16 -> Cout, window 19, stride 5,
 * swish), forward and backward, on the MI355X (gfx950).  A library of its own (libtaiyaki_amd_conv_strided.so: the
 * flip-flop ABI is pinned); it shares that header's conventions and result codes.
 *
 *   x (T, N, 16), w (Cout, 16, 19) as nn.Conv1d keeps it, b (Cout); Tout = ceil(T / 5), rows = Tout N.
 *   Window t of column n covers input times 5 t - 9 ... 5 t + 9; times outside [0, T) read as zero.
 *   z (Tout, N, Cout) = windows . w^T + b,   y = z sigmoid(z)
 *
 * No window matrix is written, forward or backward (csrc/conv_strided.hip).  The arithmetic is that of
 * taiyaki_amd_lstm_wgrad.h and taiyaki_amd_rnn_proj.h: every float32 operand split into three bf16 parts, six bf16 MFMAs
 * per product with float32 accumulation, the leading product and the five corrections in accumulators of their own.
 *
 * tk_conv_strided_forward_dev    one small launch writes the weights' bf16 images (k re-ordered to tap-major, so that a
 *     k block of 16 is one tap: 64 contiguous bytes of x), one GEMM launch writes z (NULL: not wanted) and y.  k runs
 *     in ascending blocks inside one workgroup: the bits of an output row are a function of that row's window, of w and
 *     of b only -- not of N, of T or of the row's position.
 * tk_conv_strided_backward_dev   dz = dy (s + z s (1 - s)), s = sigmoid(z), one element-wise launch into `dz`
 *     (rows x Cout floats of the caller's);  dw, db: one split-K launch over runs of rows (partial results in the
 *     workspace, no accumulation chain longer than 8192 rows) and their sum in a fixed order, written in w's layout;
 *     dx (NULL: not wanted): a gather GEMM -- the five input times 5 u ... 5 u + 4 of column n are 80 outputs of one
 *     row (u, n), summed over the windows u - 1, u, u + 1, u + 2 in that order and over their Cout channels (k =
 *     4 Cout, the weights' image zero where a time lies outside a window) -- which writes dx itself, cropped to T.
 * No atomics: two calls on the same inputs give the same bits, whatever the workspace and `dz` held.
 *
 * tk_conv_strided_supported: 1 for cin = 16, winlen = 19, stride = 5 and cout = 192, 256 or 384 (the sizes of the
 *     recurrent kernels, each measured below the unfold + GEMM path at 102400 rows), 0 otherwise.
 * tk_conv_strided_workspace_bytes: the workspace of either call (weight images of both, the partial results) at that
 *     shape, a function of its arguments only; 0 where the shape is not supported, T or N is 0, or rows x max(304, cout)
 *     reaches 2^31 (the kernels index a window and a row of z or dz in 32 bits).
 *
 * Tensors are dense.  x, z, y, dy, dz, dx and the workspace must be 16-byte aligned (TK_ERR_BAD_ARG otherwise); w, b,
 * dw, db need float alignment.  Nothing is allocated or synchronised inside; the calls can be captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_CONV_STRIDED_H
#define TAIYAKI_AMD_CONV_STRIDED_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_conv_strided_supported(size_t cin, size_t cout, size_t winlen, size_t stride);

size_t tk_conv_strided_workspace_bytes(size_t T, size_t N, size_t cout, int cu_count);

int tk_conv_strided_forward_dev(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cout,
                                int cu_count, float *z, float *y, void *workspace, size_t workspace_bytes,
                                void *stream);

int tk_conv_strided_backward_dev(const float *dy, const float *x, const float *z, const float *w, size_t T, size_t N,
                                 size_t cout, int cu_count, float *dz, float *dx, float *dw, float *db,
                                 void *workspace, size_t workspace_bytes, void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_conv_strided_lab.so). */
/* force the number of runs of the weight-gradient launch (0: the rule) */
void tk_lab_conv_strided_set_splits(int splits);
/* the launch plan at a shape: out[12] = forward row tiles, column tiles, k blocks, grid; dx column tiles, k blocks;
 * weight gradient runs, partial results per run, rows per run, rows per partial result, grid; workspace bytes.  0
 * where tk_conv_strided_workspace_bytes is 0 */
int tk_lab_conv_strided_plan(size_t T, size_t N, size_t cout, int cu_count, size_t *out);
#endif

#ifdef __cplusplus
}
#endif

#endif

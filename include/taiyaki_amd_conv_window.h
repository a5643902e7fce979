/*
 * taiyaki_amd_conv_window.h -- C ABI of the mLstm models' third layer, Convolution(16 -> Cout, window W, stride S, swish),
 * forward and backward, at the geometries and sizes of the fast and the RNA models, on the MI355X (gfx950).  A library of
 * its own (libtaiyaki_amd_conv_window.so; taiyaki_amd_conv_strided.h and its library are pinned and stay as they are); it
 * shares that header's conventions and the result codes of taiyaki_amd_flipflop.h.
 *
 *   x (T, N, 16), w (Cout, 16, W) as nn.Conv1d keeps it, b (Cout); Tout = ceil(T / S), rows = Tout N, h = W / 2 (W is odd).
 *   Window t of column n covers input times S t - h ... S t + h; times outside [0, T) read as zero: the pad
 *   (W / 2, (W - 1) / 2) of the layer.
 *   z (Tout, N, Cout) = windows . w^T + b,   y = z sigmoid(z)
 *
 * The kernels are those of taiyaki_amd_conv_strided.h, csrc/conv_strided.hip compiled a second time with the geometry a
 * template argument: no window matrix is written, every float32 operand is split into three bf16 parts, six bf16 MFMAs
 * per product with float32 accumulation, the leading product and the five corrections in accumulators of their own.
 *
 * tk_conv_window_forward_dev    one small launch writes the weights' bf16 images (k re-ordered to tap-major, so that a k
 *     block of 16 is one tap: 64 contiguous bytes of x), one GEMM launch writes z (NULL: not wanted) and y.  k runs in
 *     ascending blocks, W of them, inside one workgroup: the bits of an output row are a function of that row's window,
 *     of w and of b only -- not of N, of T or of the row's position.
 * tk_conv_window_backward_dev   dz = dy (s + z s (1 - s)), s = sigmoid(z), one element-wise launch into `dz` (rows x Cout
 *     floats of the caller's);  dw, db: one split-K launch over runs of rows (partial results in the workspace, no
 *     accumulation chain longer than 8192 rows) and their sum in a fixed order, written in w's layout;  dx (NULL: not
 *     wanted): a gather GEMM -- the S input times S u ... S u + S - 1 of column n are 16 S outputs of one row (u, n),
 *     summed over the windows u - 1, u, u + 1, u + 2 in that order and over their Cout channels (k = 4 Cout, the
 *     weights' image zero where a time lies outside a window) -- which writes dx itself, cropped to T.
 * No atomics: two calls on the same inputs give the same bits, whatever the workspace and `dz` held.
 *
 * tk_conv_window_supported: 1 for cin = 16, (winlen, stride) = (19, 5), (31, 10) or (31, 12) -- the DNA and the two RNA
 *     geometries of the production models -- and cout = 96, 128, 192, 256 or 384, the sizes from the fast model's on for
 *     which a recurrent kernel exists; 0 otherwise.  Sizes below 96 (16, 32, 64: test models) and every other window or
 *     stride are out of scope and stay on the unfold + GEMM path.  (19, 5) at 192, 256 and 384 is also what
 *     taiyaki_amd_conv_strided.h takes; the layer asks that library first.
 * tk_conv_window_workspace_bytes: the workspace of either call (weight images of both, the partial results) at that
 *     shape, a function of its arguments only; 0 where the shape is not supported, T, N or cu_count is 0, or rows x
 *     max(16 winlen, cout) reaches 2^31 (the kernels index a window and a row of z or dz in 32 bits).
 *
 * Tensors are dense.  x, z, y, dy, dz, dx and the workspace must be 16-byte aligned (TK_ERR_BAD_ARG otherwise); w, b,
 * dw, db need float alignment.  Nothing is allocated or synchronised inside; the calls can be captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_CONV_WINDOW_H
#define TAIYAKI_AMD_CONV_WINDOW_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_conv_window_supported(size_t cin, size_t cout, size_t winlen, size_t stride);

size_t tk_conv_window_workspace_bytes(size_t T, size_t N, size_t cout, size_t winlen, size_t stride, int cu_count);

int tk_conv_window_forward_dev(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cout,
                               size_t winlen, size_t stride, int cu_count, float *z, float *y, void *workspace,
                               size_t workspace_bytes, void *stream);

int tk_conv_window_backward_dev(const float *dy, const float *x, const float *z, const float *w, size_t T, size_t N,
                                size_t cout, size_t winlen, size_t stride, int cu_count, float *dz, float *dx, float *dw,
                                float *db, void *workspace, size_t workspace_bytes, void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_conv_window_lab.so). */
/* force the number of runs of the weight-gradient launch (0: the rule) */
void tk_lab_conv_window_set_splits(int splits);
/* the launch plan at a shape: out[12] = forward row tiles, column tiles, k blocks, grid; dx column tiles, k blocks;
 * weight gradient runs, partial results per run, rows per run, rows per partial result, grid; workspace bytes.  0
 * where tk_conv_window_workspace_bytes is 0 */
int tk_lab_conv_window_plan(size_t T, size_t N, size_t cout, size_t winlen, size_t stride, int cu_count, size_t *out);
#endif

#ifdef __cplusplus
}
#endif

#endif

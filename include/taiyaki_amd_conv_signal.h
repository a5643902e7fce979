/*
 * taiyaki_amd_conv_signal.h -- C ABI of the mGru models' first layer, Convolution(1 -> Cout, window 19, stride s,
 * tanh) on the raw signal, forward and backward, on the MI355X (gfx950).  A library of its own
 * (libtaiyaki_amd_conv_signal.so: the flip-flop ABI is pinned); it shares that header's conventions and result codes.
 *
 *   x (T, N) float32: the (T, N, 1) tensor; w (Cout, 1, 19) as nn.Conv1d keeps it, b (Cout);
 *   Tout = ceil(T / s), rows = Tout N.  Window t of column n covers input times s t - 9 ... s t + 9; times outside
 *   [0, T) read as zero (the reference's padding (9, 9)).
 *   y[t, n, c] (Tout, N, Cout) = tanh(b[c] + sum over k < 19 of w[c][k] x[s t + k - 9][n])
 *
 * Plain float32 FMAs, the taps of a row walked k = 0 ... 18 from the bias on: the bits of an output row are a function
 * of that row's window, of w and of b only -- not of N, of T, of the row's position or of cu_count.  tanh saturates
 * inside the finite range: a pre-activation of +-1e4 gives exactly +-1; a NaN in x reaches the rows whose windows hold
 * it and no other.
 *
 * tk_conv_signal_forward_dev    one launch, no workspace: y.
 * tk_conv_signal_backward_dev   dz = dy (1 - y^2) is formed in registers and never written;
 *     dw[c][k] = sum over t, n of dz[t, n, c] x[s t + k - 9][n], db[c] = sum of dz[., ., c].  One launch in which every
 *     workgroup writes one partial result of Cout x 20 floats into the workspace, and a second small launch that adds
 *     the partial results in a fixed order (runs of consecutive indices in index order, the runs' sums in index order)
 *     and writes dw in w's layout and db.  No atomics: two calls on the same inputs with the same cu_count give the
 *     same bits, whatever the workspace held.  There is no dx: the layer is the network's first, its input needs no
 *     gradient.
 *
 * tk_conv_signal_supported: 1 for cin = 1, winlen = 19, stride 1 ... 8 (a run-time argument of the calls) and cout =
 *     32, 64, 96, 128, 192, 256 or 384 (every size the GRU kernels take), 0 otherwise.
 * tk_conv_signal_workspace_bytes: the workspace of the backward call at that shape (its partial results), a function
 *     of its arguments only; 0 where the shape is not supported, T or N is 0, cu_count < 1, or rows x cout reaches 2^31
 *     (the kernels index an element of y in 32 bits).
 *
 * Tensors are dense.  y, dy and the workspace must be 16-byte aligned (TK_ERR_BAD_ARG otherwise); x (N is arbitrary: its
 * rows are not 16-byte aligned anyway), w, b, dw and db need float alignment.  Nothing is allocated or synchronised
 * inside; the calls can be captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_CONV_SIGNAL_H
#define TAIYAKI_AMD_CONV_SIGNAL_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_conv_signal_supported(size_t cin, size_t cout, size_t winlen, size_t stride);

size_t tk_conv_signal_workspace_bytes(size_t T, size_t N, size_t cout, size_t stride, int cu_count);

int tk_conv_signal_forward_dev(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cout,
                               size_t stride, int cu_count, float *y, void *stream);

int tk_conv_signal_backward_dev(const float *dy, const float *x, const float *y, size_t T, size_t N, size_t cout,
                                size_t stride, int cu_count, float *dw, float *db, void *workspace,
                                size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif

/*
 * taiyaki_amd_squiggle_net.h -- C ABI of the squiggle predictor network of bin/train_squiggle.py, forward and backward,
 * as fused kernels on the MI355X (gfx950).  A library of its own (libtaiyaki_amd_squiggle_net.so: the flip-flop ABI is
 * pinned); it shares that header's conventions and result codes.
 *
 *   layer 0            a_0 = tanh(conv(x; w_0) + b_0)                        3 -> size channels
 *   layer l = 1..depth a_l = a_(l-1) + tanh(conv(a_(l-1); w_l) + b_l)        size -> size, residual
 *   layer depth + 1    y   = conv(a_depth; w_(depth+1)) + b_(depth+1)        size -> 3, linear
 *
 *   x, y, dy, dx (P, N, 3) float32; every convolution has window `winlen` (odd), stride 1 and reads zeros outside
 *   [0, P), as nn.Conv1d behind a pad of winlen / 2 either side.  `params` and `grads` are HOST arrays of
 *   2 (depth + 2) device pointers, w_0, b_0, w_1, b_1, ...: weight (cout, cin, winlen) as nn.Conv1d keeps it, bias
 *   (cout).  No repacked copy is kept by the caller or made in device memory.
 *   `lengths`: device int32, one value per column (clamped to [0, P]), or NULL: every column has P positions.  With
 *   lengths every layer's activation of column n is 0 at and beyond lengths[n], so that the rows below it are what the
 *   column gives run alone at P = lengths[n]; y and `saved` are +0 there, dy there is ignored and dx there is 0.
 *
 * tk_squiggle_net_forward_dev    ONE launch.  A workgroup takes `tile` positions of one column and the halo of
 *     R = (depth + 2) (winlen / 2) positions either side that the layers between x and y consume (128 rows in all: tile =
 *     128 - 2 R), keeps the activations in LDS from the first layer to the last and writes y.  The weights of the
 *     size -> size layers are staged tap by tap.  float32 operands, float32 fused multiply-adds: every output element is
 *     b + per tap (ascending) the sum over the input channels (ascending, one chain per tap, added whole) -- an order
 *     that is a function of the layer and the channel only, not of N, of P, of the tile or of whether the row is a
 *     neighbour's halo row.
 *     `saved` (the training form; NULL under no_grad: y alone is written): (depth + 1, P, N, size) floats, the tanh
 *     OUTPUTS t_l = tanh(z_l) of layers 0 ... depth.
 * tk_squiggle_net_backward_dev   ONE launch over the same tiles plus the sum of its partial results.  The gradient walks
 *     the layers from last to first inside the launch.  The residual sums are REBUILT from the saved tanh outputs in the
 *     forward's order (a_l = ((t_0 + t_1) + ...) + t_l, the same bits the forward held), never recovered as a
 *     difference: 1 - t^2 is taken from the saved t itself.  Weight and bias gradients: every workgroup walks a run of
 *     tiles (tile i, i + grid, ...) and adds each tile's sums over its OWN positions into its slab of the workspace
 *     (written, not added, by its first tile), and a second launch adds the slabs in their order (in blocks of 16) into
 *     `grads`, in the parameters' own layout.  No atomics: two calls on the same inputs give the same bits whatever the
 *     workspace held.  dx: NULL when not wanted.
 *
 * tk_squiggle_net_supported: 1 for size 16, 32 or 64, winlen 5 or 9 and depth 1 ... 8; 0 otherwise.
 * tk_squiggle_net_workspace_bytes: the backward's workspace (the forward needs none), a function of its arguments only;
 *     0 where the shape is not supported, P or N is 0, or N x tiles reaches 2^31.
 *
 * Tensors are dense.  `saved` and the workspace must be 16-byte aligned (TK_ERR_BAD_ARG otherwise); everything else
 * needs float alignment.  A NULL entry of `params` or `grads` is TK_ERR_BAD_ARG.  Nothing is allocated or synchronised
 * inside; the calls can be captured into a hipGraph.
 */
#ifndef TAIYAKI_AMD_SQUIGGLE_NET_H
#define TAIYAKI_AMD_SQUIGGLE_NET_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_squiggle_net_supported(size_t size, size_t depth, size_t winlen);

size_t tk_squiggle_net_workspace_bytes(size_t P, size_t N, size_t size, size_t depth, size_t winlen, int cu_count);

int tk_squiggle_net_forward_dev(const float *x, void **params, const int *lengths, size_t P, size_t N, size_t size,
                                size_t depth, size_t winlen, int cu_count, float *saved, float *y, void *stream);

int tk_squiggle_net_backward_dev(const float *dy, const float *x, const float *saved, void **params,
                                 const int *lengths, size_t P, size_t N, size_t size, size_t depth, size_t winlen,
                                 int cu_count, float *dx, void **grads, void *workspace, size_t workspace_bytes,
                                 void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_squiggle_net_lab.so). */
/* the launch plan at a shape: out[8] = owned positions per tile, halo rows forward, halo rows backward, tiles per
 * column, forward grid, backward grid (= partial results), floats per partial result, workspace bytes.  0 where
 * tk_squiggle_net_workspace_bytes is 0 */
int tk_lab_squiggle_net_plan(size_t P, size_t N, size_t size, size_t depth, size_t winlen, int cu_count, size_t *out);
#endif

#ifdef __cplusplus
}
#endif

#endif

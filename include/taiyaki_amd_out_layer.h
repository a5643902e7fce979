/*
 * taiyaki_amd_out_layer.h -- C ABI of the models' output layer, GlobalNormFlipFlop and GlobalNormFlipFlopCatMod, forward
 * and backward, on the MI355X (gfx950).  A library of its own (libtaiyaki_amd_out_layer.so: the flip-flop ABI is
 * pinned); it shares that header's conventions and result codes.
 *
 *   x (rows, I), rows = T N;  w (L, I) and b (L) as nn.Linear keeps them;  z (rows, L) = x w^T + b is never written;
 *   y (rows, O).  An output column o reads the linear column src[o] and is
 *       group[o] = -1      y = scale tanh(z[src[o]])
 *       group[o] = g >= 0  y = z[src[o]] - log sum over the outputs o' of group g of exp(z[src[o']])   (log_softmax)
 *   The outputs of one group are contiguous in y; a linear column may feed several groups (the cat-mod layer's single
 *   canonical column feeds every base's group) or none.  `src` and `group` are HOST arrays of O ints: they travel in
 *   the kernels' arguments, nothing is uploaded.  Both NULL: the plain layer, O = L, src[o] = o, group[o] = -1.
 *
 * The arithmetic is that of taiyaki_amd_rnn_proj.h: every float32 operand split into three bf16 parts, six bf16 MFMAs
 * per product with float32 accumulation, the leading product and the five corrections in accumulators of their own,
 * added once; k in ascending blocks of 16 inside one wavefront; bias, tanh, exp and log in float32 at the end.
 *
 * tk_out_layer_forward_dev    one small launch writes the three bf16 parts of w in the order the GEMM reads them; one
 *     GEMM launch writes y finished.  A wavefront owns 32 rows and every column (L padded to 32 or 64): no operand
 *     passes through LDS, z crosses it once for the epilogue, whose stores are whole contiguous runs of y.
 * tk_out_layer_backward_dev   dz (rows, L) from dy and y alone, summed into column src[o] in ascending o:
 *         group -1:  dy (scale - y^2 / scale)       group g:  dy_o - exp(y_o) (sum over group g of dy)
 *     dx = dz w (NULL: not wanted), one launch, which also leaves dz in the workspace as bf16 operand fragments (dz is
 *     never a tensor of the caller's);  dw (L, I) = dz^T x and db = sum of dz: one launch over runs of rows, partial
 *     results in the workspace, and their sum in a fixed order -- no accumulation chain longer than 8192 rows.
 *
 *   - Row independence: the bits of a row of y and of dx are a function of that row of x (of dy and y) and of w and b
 *     only -- not of rows, of the row's position, of the other rows or of cu_count.
 *   - No atomics: two calls on the same inputs give the same bits, whatever the workspace held.
 *   - A non-finite element of x makes its own row of y non-finite and touches no other row.
 *   - Saturation: where |z| is beyond tanh's float32 saturation y is exactly +-scale, and dz is exactly 0 there.
 *   - Bad arguments are refused on the host before any launch: TK_ERR_BAD_ARG for a NULL pointer (dx alone may be
 *     NULL), a workspace that is not 16-byte aligned, one table without the other, a table entry out of range or a
 *     group that is not one contiguous run of outputs; TK_ERR_UNSUPPORTED for sizes outside tk_out_layer_supported or
 *     the workspace rule; TK_ERR_WORKSPACE for a workspace too small.
 *   - Nothing is allocated or synchronised inside; the calls can be captured into a hipGraph.
 *
 * tk_out_layer_supported: 1 for I in {16, 32, 64, 96, 128, 192, 256, 384} (the widths the recurrences and the
 *     projections admit), 1 <= L <= 64 and L <= O <= 64; 0 otherwise.
 * tk_out_layer_workspace_bytes: the workspace of either call (the weight images of both, dz's fragments, the partial
 *     results of cu_count x ceil(8 / ceil((I + 1) / 32)) runs of rows, each a multiple of 16 and at most 8192), a
 *     function of its four arguments only; 0 where the widths are not supported (any O), a size is 0, or
 *     rows x max(I, 64) reaches 2^31.
 *
 * Measured on an MI355X against the library path (nn.Linear and the element-wise launches behind it), the layer alone
 * at 102400 rows, sizes 96 / 256 / 384 (tools/outlayerbench.py, profiles/r44_out_layer.txt): the forward level or
 * ahead, plain and cat-mod; forward + backward of the cat-mod layer 1.9 to 4.9 x ahead at 1600, 12800 and 102400 rows
 * over three runs; of the plain layer ahead or level at 1600 and 12800 rows in most runs, at 102400 rows 1.2 to 1.35 x
 * behind at sizes 96 and 384 and between level and 1.3 x behind at 256 -- no crossover from which it is ahead.  taiyaki_amd/layers.py therefore takes these kernels under no_grad
 * at every supported shape, under grad mode for the cat-mod layer at every number of rows and for the plain layer never
 * (OUT_LAYER_GRAD_MIN_ROWS, OUT_LAYER_PLAIN_GRAD_MIN_ROWS).
 *
 * Tensors are dense and row-major.  x takes 16-byte loads where it is 16-byte aligned and guarded 4-byte loads
 * otherwise; w, b, dw, db need float alignment.
 */
#ifndef TAIYAKI_AMD_OUT_LAYER_H
#define TAIYAKI_AMD_OUT_LAYER_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_out_layer_supported(size_t I, size_t L, size_t O);

size_t tk_out_layer_workspace_bytes(size_t rows, size_t I, size_t L, int cu_count);

int tk_out_layer_forward_dev(const float *x, const float *w, const float *b, const int *src, const int *group,
                             size_t rows, size_t I, size_t L, size_t O, float scale, int cu_count, float *y,
                             void *workspace, size_t workspace_bytes, void *stream);

int tk_out_layer_backward_dev(const float *dy, const float *y, const float *x, const float *w, const int *src,
                              const int *group, size_t rows, size_t I, size_t L, size_t O, float scale, int cu_count,
                              float *dx, float *dw, float *db, void *workspace, size_t workspace_bytes, void *stream);

#ifdef TK_LAB
/* The lab build only (libtaiyaki_amd_out_layer_lab.so). */
/* the launch plan at a shape: out[7] = rows per workgroup (the row tile), columns per tile (L padded), k blocks of the
 * forward, forward grid, weight-gradient runs, rows per run, workspace bytes.  0 where tk_out_layer_workspace_bytes is
 * 0 or O is outside the rule */
int tk_lab_out_layer_plan(size_t rows, size_t I, size_t L, size_t O, int cu_count, size_t *out);
#endif

#ifdef __cplusplus
}
#endif

#endif

/*
 * taiyaki_amd_optim.h -- C ABI of the optimiser step on the MI355X (gfx950): gradient scaling, per-parameter maxima,
 * clip by value, L2-norm cap, AdamW and the zero fill of the gradient arena, in two launches.  A library of its own
 * (libtaiyaki_amd_optim.so: the flip-flop ABI is pinned); it shares that header's conventions and result codes.
 *
 * The gradients of all `nseg` parameter tensors live in one flat float32 arena (`grads`, `total` elements, segment s at
 * [seg_off[s], seg_off[s + 1])); `exp_avg` and `exp_avg_sq` are flat arrays of the same layout and the same offsets.  The
 * parameters stay where their owner allocated them: `params` is a DEVICE array of nseg pointers (float *) to contiguous float32.
 *
 * The segment description is a TILE TABLE, built once on the host from the HOST offsets (tk_optim_tiles) and uploaded by
 * the caller: TK_OPTIM_TILE_WORDS 32-bit words per tile -- segment, first element in the arena, count (at most
 * TK_OPTIM_TILE), first element inside the segment.  The tiles cover every element once, in order, and never cross a
 * segment; an empty segment has one tile of count 0 (its maximum, 0, is still written).
 *
 * `hyper`: TK_OPTIM_HYPER_WORDS float32 words on the device, read when the kernels RUN (a value filled in between two
 * replays of a captured graph is the value the next replay uses):
 *     inputs   TK_OPTIM_LR, TK_OPTIM_BETA1, TK_OPTIM_BETA2, TK_OPTIM_EPS, TK_OPTIM_WEIGHT_DECAY, TK_OPTIM_GRAD_SCALE,
 *              TK_OPTIM_MAX_NORM (+inf: no cap), TK_OPTIM_STEP (the number of updates made so far, float32 as torch's
 *              capturable step is)
 *     outputs  TK_OPTIM_GRAD_NORM, and TK_OPTIM_STEP advanced by one
 *     the words from TK_OPTIM_STEP_NOW on belong to the call (what its first launch hands its second).
 *
 * tk_adamw_step_dev, per element, in this order, with t = step + 1:
 *     1. g = grads * grad_scale
 *     2. maxs[s] = max |g| over segment s, before clipping; NaN if the segment holds a NaN (as tk_grad_maxabs_clip_dev)
 *     3. where thresh[s] is finite and >= 0:  g = fminf(fmaxf(g, -thresh[s]), thresh[s])   (that entry point's rule)
 *     4. grad_norm = sqrt(sum of g^2) over the arena, after the clamp (with_norm only)
 *     5. if max_norm is finite:  g *= min(1, max_norm / (grad_norm + 1e-6))   (torch.nn.utils.clip_grad_norm_; with_norm only)
 *     6. AdamW as torch.optim.AdamW states it:
 *            p *= 1 - lr wd;   m += (g - m)(1 - beta1);   v = beta2 v + (1 - beta2) g^2
 *            p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *     7. grads = 0 where zero_grads, otherwise the scaled, clamped, capped g
 *     8. step = t
 *   `thresh` and `maxs` (nseg floats each) may be NULL: no clamp, no maxima.  `with_norm` 0: steps 4 and 5 are left out
 *   (TK_OPTIM_MAX_NORM is not read, TK_OPTIM_GRAD_NORM not written) -- the host cannot look into the device block, so the
 *   caller says whether a norm is wanted.
 *
 * Launches: two.  The first (statistics) walks the tiles once: per tile the maximum and the sum of squares (in float64),
 * written to the workspace; its first thread turns the hyper block into the update's scalars (float64 arithmetic, rounded
 * once) and advances the step word.  With maxs NULL and with_norm 0 (thresh or not: the update clamps by itself) it
 * shrinks to that one thread.  The second (update) walks the tiles again; every workgroup adds the tile sums in one fixed
 * order (a function of the tile count), the workgroup that owns a segment's first tile folds that segment's tile maxima.
 * Nothing is handed between workgroups of one launch: no workgroup reads a word that another workgroup of the same
 * launch writes (the update reads TK_OPTIM_STEP_NOW and the derived words, which only the first launch writes), no
 * atomics, no counters.
 *
 *   - Every output's bits are a function of the arguments alone: not of cu_count (it only bounds the grids), of timing or
 *     of what the workspace held.
 *   - A NaN or infinity spreads as the arithmetic above spreads it; no step is skipped.
 *   - A tile whose four addresses (g, m, v, p) are 16-byte aligned moves as 16-byte accesses, any other as 4-byte ones.
 *   - Bad arguments are refused on the host before any launch: TK_ERR_BAD_ARG for a NULL pointer (thresh and maxs alone may
 *     be NULL), nseg == 0, ntiles == 0, cu_count <= 0, total above 2^31 or a workspace that is not 16-byte aligned;
 *     TK_ERR_WORKSPACE for a workspace smaller than tk_optim_workspace_bytes.
 *   - Nothing is allocated or synchronised inside; the call can be captured into a hipGraph (a straight chain).
 *   - Every workgroup of the update reads all tile sums (16 bytes per tile, from L2; with_norm only): 24 KB at 6 x 10^6
 *     elements.  The results are right up to the 2^31 elements the call admits; the cost grows with the arena (8 MB per
 *     workgroup there), and a caller with arenas beyond some 10^8 elements should expect the update launch to slow down.
 *
 * Host functions (no GPU): `seg_off` holds nseg + 1 ascending HOST offsets, seg_off[0] = 0.
 *   tk_optim_tile_count      tiles of that layout; 0 for NULL, nseg == 0, a first offset other than 0, offsets that decrease
 *                            or a total above 2^31
 *   tk_optim_tiles           writes them (capacity in tiles); TK_ERR_BAD_ARG for the same and for a capacity too small
 *   tk_optim_workspace_bytes 16 bytes per tile; 0 where tk_optim_tile_count is 0
 */
#ifndef TAIYAKI_AMD_OPTIM_H
#define TAIYAKI_AMD_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#define TK_OPTIM_TILE 4096
#define TK_OPTIM_TILE_WORDS 4

#define TK_OPTIM_LR 0
#define TK_OPTIM_BETA1 1
#define TK_OPTIM_BETA2 2
#define TK_OPTIM_EPS 3
#define TK_OPTIM_WEIGHT_DECAY 4
#define TK_OPTIM_GRAD_SCALE 5
#define TK_OPTIM_MAX_NORM 6
#define TK_OPTIM_STEP 7
#define TK_OPTIM_GRAD_NORM 8
#define TK_OPTIM_STEP_NOW 9
#define TK_OPTIM_HYPER_WORDS 16

#ifdef __cplusplus
extern "C" {
#endif

size_t tk_optim_tile_count(const int64_t *seg_off, size_t nseg);

int tk_optim_tiles(const int64_t *seg_off, size_t nseg, uint32_t *tiles, size_t capacity);

size_t tk_optim_workspace_bytes(const int64_t *seg_off, size_t nseg);

int tk_adamw_step_dev(float *grads, float *exp_avg, float *exp_avg_sq, const void *params, const uint32_t *tiles,
                      size_t ntiles, size_t nseg, size_t total, float *hyper, const float *thresh, float *maxs,
                      void *workspace, size_t workspace_bytes, int with_norm, int zero_grads, int cu_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif

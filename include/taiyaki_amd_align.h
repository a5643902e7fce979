/*
 * taiyaki_amd_align.h -- C ABI of the batched unit-cost global alignment on the MI355X (gfx950): how far a call is from
 * its reference, and how many of the alignment's columns match.  A library of its own (libtaiyaki_amd_align.so: the
 * flip-flop ABI is pinned); it shares that header's conventions and result codes.
 *
 * The quantity.  A query q (m codes) against a reference r (n codes), codes equal or not.  Over all global alignments,
 *   distance D  the least number of non-match columns (mismatch, insertion, deletion);
 *   matches  M  the greatest number of match columns among the alignments with D non-match columns;
 * the lexicographic minimum of (D, -M) under
 *   cell(i, j) = min(cell(i-1, j-1) + (q_i == r_j ? (0, -1) : (1, 0)), cell(i-1, j) + (1, 0), cell(i, j-1) + (1, 0)),
 *   cell(0, j) = (j, 0), cell(i, 0) = (i, 0);  the answer is cell(m, n).  columns = M + D, accuracy = M / columns.
 *
 * The band.  max_distance t >= 0 sweeps the diagonals j - i in [min(0, n - m) - p, max(0, n - m) + p] only,
 * p = floor((t - |n - m|) / 2); every alignment of cost <= t lies inside, so the pair's `exact` word is 1 exactly where
 * the band's D <= t, and D and M are then those of the full sweep.  t < |n - m|: nothing is swept, exact = 0,
 * D = max(m, n), M = 0.  t < 0: every diagonal, exact = 1.
 *
 * One wavefront per pair, every pair of the batch in one launch.  A row of the band lives in the wave's registers (bands
 * of up to TK_ALIGN_REG_BAND diagonals) or in LDS (beyond); nothing but the sequences is read and nothing but the three
 * words per pair is written.  No workspace, nothing shared between workgroups, nothing allocated or synchronised
 * inside: the calls can be captured into a hipGraph.
 *
 * Limits (the cell's key is D in the upper and 65535 - M in the lower half of 32 bits; sums saturate, nothing wraps):
 *   TK_ALIGN_MAX_LEN   the longest query or reference;
 *   TK_ALIGN_MAX_BAND  the widest band (diagonals that cross the matrix; a sweep of every diagonal has m + n + 1).
 * `band_cells` (0: TK_ALIGN_MAX_BAND) is the caller's bound on the band of every pair: it sizes the LDS row of the
 * launch (none up to TK_ALIGN_REG_BAND).  The host does not see lengths that live on the device, so a pair beyond a
 * limit or beyond `band_cells` is REPORTED, not swept: exact = 0, D = max(m, n) (at most INT32_MAX), M = 0.  What
 * the host does see is refused with TK_ERR_UNSUPPORTED before anything is launched: npair beyond INT32_MAX, band_cells
 * beyond TK_ALIGN_MAX_BAND; and for tk_align_calls_dev nblk + 1 beyond TK_ALIGN_MAX_CALL, nbase 0 or beyond 127.
 *
 * tk_align_band (host): the band of (m, n, t): first and last diagonal, clipped to the diagonals that cross the matrix
 *   (-m .. n), and the cells per lane of the sweep that takes it: ceil(band / 64) rounded up to 1, 2, 4, 8 or 16 (the
 *   register instantiations), and to the next odd number beyond 16 (the LDS sweep: odd strides keep the lanes on
 *   distinct banks).  Returns TK_OK; TK_ERR_BAD_ARG for a NULL result pointer; TK_ERR_UNSUPPORTED beyond the limits;
 *   for t in 0 .. |n - m| - 1 TK_OK with *first = 1, *last = 0 and *cells_per_lane = 0 (no diagonal).
 *
 * tk_align_pairs_dev
 *   query, ref        uint8 codes of all pairs, packed;  q_off, r_off (npair + 1) int64: pair k has
 *                     query[q_off[k] .. q_off[k + 1]) and ref[r_off[k] .. r_off[k + 1])  (a negative length counts as 0)
 *   pairs             NULL: the launch takes pairs 0 .. npair - 1.  Else (npair) int32 on the device: the launch takes
 *                     the pairs it names (each once), and every per-pair array below is indexed by the pair's number,
 *                     not by its place in `pairs` -- a later round over the pairs a first one left fills the same arrays
 *   max_distance      int32 per pair on the device, or NULL: then `shared_max_distance` holds for every pair
 *   distance, matches, exact   int32 per pair each
 *
 * tk_align_calls_dev  (the validation form: the Viterbi call of column n against that column's own labels)
 *   path              (nblk + 1, nbatch) int64 flip-flop states, as tk_flipflop_viterbi_dev writes them
 *   lengths           (nbatch) int32 or NULL: column n has lengths[n] (clamped to 0 .. nblk) blocks, lengths[n] + 1 states
 *   seqs, seq_off, seqlens   the loss's labels: int32 flip-flop codes, concatenated; (nbatch + 1) int64 start of each
 *                     column's labels; (nbatch) int32 label counts.  The reference is seqs % nbase.
 *   The query is the path collapsed in the wave (state % nbase where the state differs from its predecessor, first
 *   state included); it lives in LDS and never reaches memory.  The answer is that of every diagonal (exact = 1): the
 *   wave starts from the band of max_distance |n - m| + max(16, min(m, n) / 16) and doubles it until the band holds
 *   the answer, so a call close to its labels costs its band and not the table.  band_cells as above, against
 *   TK_ALIGN_MAX_CALL_BAND (a column whose last band is wider is reported with exact = 0).
 *
 * Checks before anything is launched: a NULL required pointer: TK_ERR_BAD_ARG (npair or nbatch 0: nothing to do, TK_OK,
 * checked first); the limits above: TK_ERR_UNSUPPORTED; TK_ERR_LAUNCH if the launch fails.
 */
#ifndef TAIYAKI_AMD_ALIGN_H
#define TAIYAKI_AMD_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#define TK_ALIGN_MAX_LEN 65534
#define TK_ALIGN_REG_BAND 1024
#define TK_ALIGN_MAX_BAND 16320
#define TK_ALIGN_MAX_CALL 4096
#define TK_ALIGN_MAX_CALL_BAND 8128

#ifdef __cplusplus
extern "C" {
#endif

int tk_align_band(size_t m, size_t n, int max_distance, int *first, int *last, int *cells_per_lane);

int tk_align_pairs_dev(const uint8_t *query, const int64_t *q_off, const uint8_t *ref, const int64_t *r_off,
                       size_t npair, const int32_t *pairs, const int32_t *max_distance, int shared_max_distance,
                       size_t band_cells, int32_t *distance, int32_t *matches, int32_t *exact, void *stream);

int tk_align_calls_dev(const int64_t *path, const int32_t *lengths, size_t nblk, size_t nbatch, size_t nbase,
                       const int32_t *seqs, const int64_t *seq_off, const int32_t *seqlens, size_t band_cells,
                       int32_t *distance, int32_t *matches, int32_t *exact, void *stream);

#ifdef __cplusplus
}
#endif

#endif

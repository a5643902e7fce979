/*
 * taiyaki_amd_chunks_seqlen.h -- C ABI of the squiggle trainer's batches on the MI355X (gfx950): training chunks of a
 * fixed number of BASES whose signal lengths differ, taken from the mapped-signal set resident in device memory
 * (tk_mapped_store).  A library of its own (libtaiyaki_amd_chunks_seqlen.so: the flip-flop ABI is pinned); it shares
 * that header's store, filter, reason codes, status word and result codes.
 *
 * The counterpart of tk_chunks_{locate,gather}_dev, which cut chunks of a fixed number of SAMPLES.  Restated here:
 *   taiyaki/signal_mapping.py:556-594   SignalMapping.get_chunk_with_sequence_length
 *   taiyaki/signal_mapping.py:479-513   _get_chunk (empty signal, max dwell)
 *   taiyaki/signal_mapping.py:680-716   Chunk.apply_filters
 *   bin/train_squiggle.py:201-209       embed_sequence per chunk, the currents concatenated, a length per chunk
 * A batch is three launches and never touches the host: this locate, tk_chunks_select_dev of the main library as it
 * stands (hand it the candidates' `siglen` where it takes `seqlen`: its `seqoff` is then `sigoff`, the exclusive
 * prefix sum of the accepted chunks' signal lengths), and this gather.  All array pointers are device pointers;
 * `store`, `filter` and `embed` are read on the host.  Nothing is allocated or synchronised inside: the calls can be
 * captured into a hipGraph.
 *
 * tk_chunks_seqlen_locate_dev   one wavefront per candidate
 *   mapped_ref   (nreads, 2) int32: get_mapped_reference_region (signal_mapping.py:353-368) of every read -- the first
 *                and the last INDEX of Ref_to_signal whose value lies in [0, siglen]; (0, 0) when nothing is mapped
 *   cand_read    (ncand) read numbers.  A number outside 0 .. nreads - 1 is not looked up: reason nullmapping
 *   cand_start   (ncand) start in bases into the mapped reference region, or NULL: then the start is
 *                floor(cand_frac[c] * spare), cand_frac (ncand) float64 uniform in [0, 1)
 *   Per candidate, lo and hi its read's mapped_ref:
 *     spare = (hi - lo) - chunk_bases;  spare <= 0, start >= spare or start < 0: tooshort
 *     refstart = lo + start, dacstart = rts[refstart], dacsend = rts[refstart + chunk_bases];
 *     dacsend == dacstart: emptysignal
 *     maxdwell = max of the chunk_bases - 1 differences of rts[refstart : refstart + chunk_bases] (the last base's
 *                dwell is not among them: the reference's slice); 1 when there is none (chunk_bases 1)
 *     the filter, where enabled, in float64 and in this order, sig_len = dacsend - dacstart, seq_len = chunk_bases:
 *       sig_len / (seq_len * model_stride) <= path_buffer                                    pathbuffer
 *       |sig_len / (seq_len + 1e-8) - median_meandwell| > filter_mean_dwell * mad_meandwell  meandwell
 *       maxdwell > filter_max_dwell * median_meandwell                                       maxdwell
 *   Outputs (ncand each): reason (the codes and order of TK_CHUNK_NREASON), refstart, dacstart (0 for tooshort and
 *   nullmapping), siglen (0 unless the reason is pass), maxdwell (1 unless the dwells were looked at).
 *
 * tk_chunks_seqlen_gather_dev   one launch; sel, sigoff, counts as tk_chunks_select_dev wrote them for nwant
 *   signal      (signal_cap) float32: chunk j of the accepted ones occupies [sigoff[j], sigoff[j + 1]) -- get_current's
 *               float64 arithmetic in the reference's order, rounded once to float32; with `reverse` written back to
 *               front.  Everything from sigoff[accepted] on is 0.  A chunk that would run past signal_cap is not written
 *               (what of its place lies inside the buffer is 0) and *status gets TK_STATUS_SEQS_OVERFLOW: a chunk
 *               batch's buffer was too small
 *   siglens     (nwant) int32, 0 beyond the accepted count
 *   seqs        (chunk_bases, nwant) int32: the chunks' bases, flipped with `reverse`
 *   seq_embed   (chunk_bases, nwant, 3) float32: row embed[base] of the 4 x 3 table `embed` (12 floats on the HOST,
 *               copied into the kernel's arguments); a base outside 0 .. 3 embeds as zeros
 *   Columns of seqs and seq_embed beyond the accepted count are 0.
 *
 * Checks before anything is launched: a NULL required pointer, chunk_bases 0: TK_ERR_BAD_ARG (ncand 0, or nwant 0:
 * nothing to do, TK_OK, checked after the pointers); ncand, nwant or chunk_bases beyond INT32_MAX, a grid beyond
 * INT32_MAX workgroups: TK_ERR_UNSUPPORTED; TK_ERR_LAUNCH if the launch fails.
 */
#ifndef TAIYAKI_AMD_CHUNKS_SEQLEN_H
#define TAIYAKI_AMD_CHUNKS_SEQLEN_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* tk_mapped_store, tk_chunk_filter, TK_CHUNK_NREASON, TK_STATUS_SEQS_OVERFLOW, TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

int tk_chunks_seqlen_locate_dev(const tk_mapped_store *store, const int32_t *mapped_ref, const int32_t *cand_read,
                                const int32_t *cand_start, const double *cand_frac, size_t ncand, size_t chunk_bases,
                                const tk_chunk_filter *filter, uint8_t *reason, int32_t *refstart, int32_t *dacstart,
                                int32_t *siglen, int32_t *maxdwell, void *stream);

int tk_chunks_seqlen_gather_dev(const tk_mapped_store *store, const int32_t *cand_read, const int32_t *refstart,
                                const int32_t *dacstart, const int32_t *siglen, const int32_t *sel,
                                const int64_t *sigoff, const int32_t *counts, size_t nwant, size_t chunk_bases,
                                int reverse, int standardize, const float *embed, float *signal, size_t signal_cap,
                                int32_t *siglens, int32_t *seqs, float *seq_embed, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif

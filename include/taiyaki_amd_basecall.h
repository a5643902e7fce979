/*
 * taiyaki_amd_basecall.h -- C ABI of the basecaller's device-side glue on the MI355X (gfx950): what sits between the
 * upload of raw signals and the download of finished FASTQ characters, around the network and the decode kernels of
 * taiyaki_amd_flipflop.h.  A library of its own (libtaiyaki_amd_basecall.so); it shares that header's result codes.
 *
 *   reference interface                                           replaced by
 *   ------------------------------------------------------------  ------------------------------
 *   taiyaki/maths.py:8-32 med_mad (on a float32 signal)           tk_signal_med_mad_dev
 *   taiyaki/basecall_helpers.py:11-43 chunk_read +
 *      bin/basecall.py:77-90 med_mad_norm / :198 --scaling        tk_basecall_gather_chunks_dev
 *   taiyaki/basecall_helpers.py:46-94 stitch_chunks +
 *      flipflopfings.py:81-97 path_to_str(include_first_source=False) +
 *      qscores.py:10-55,145-178 path_errprobs_to_qstring          tk_basecall_call_dev
 *   taiyaki/basecall_helpers.py:46-94 stitch_chunks of the
 *      transition scores (bin/basecall.py:216-218, --beam)        tk_basecall_stitch_scores_dev
 *   taiyaki/decodeutil/decodeutil.pyx:9-51 beamsearch +
 *      flipflopfings.py:81-97 path_to_str(include_first_source=False),
 *      for every read of a batch                                  tk_basecall_beamsearch_dev
 *   taiyaki/flipflopfings.py:100-143 extract_mod_weights on the
 *      stitched path and the stitched categorical columns of a
 *      cat-mod model, for every read of a batch                   tk_basecall_mod_weights_dev
 *
 * Conventions (those of taiyaki_amd_flipflop.h)
 *  - plain C; every pointer is a DEVICE pointer unless its comment says "host"; `stream` is a hipStream_t passed as
 *    void* (NULL = the default stream); work is enqueued, nothing is synchronised, nothing is allocated.
 *  - results: TK_OK or TK_ERR_*; data-dependent findings go to the nullable device-side `status` word (bits below,
 *    OR-ed in, never cleared).  This library's status word is its own: it shares no bit with the flip-flop one.
 *  - the caller owns every buffer, the workspace included (size from the matching *_workspace_bytes).
 *  - float32 contract: signals come in as float32 and every operation on them is a single IEEE float32 operation
 *    (no fused multiply-add, correctly rounded subtract / divide), so the normalised chunks are bit for bit what numpy
 *    gives on a float32 array.  Results do not depend on the batch a read is launched in, and repeat bit for bit.
 */
#ifndef TAIYAKI_AMD_BASECALL_H
#define TAIYAKI_AMD_BASECALL_H

#include <stddef.h>
#include <stdint.h>

#include "taiyaki_amd_flipflop.h" /* TK_OK, TK_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* bits of this library's device-side status word */
#define TK_STATUS_BAD_SIGNAL 128u   /* tk_signal_med_mad_dev: a read with a non-finite sample, no samples, or MAD == 0 */
#define TK_STATUS_CHUNK_PLAN 256u   /* tk_basecall_gather_chunks_dev: total_chunks is not what the lengths give;
                                       tk_basecall_call_dev: a read's call did not fit between its out_off entries;
                                       tk_basecall_stitch_scores_dev: a read's rows did not fit between its row_off
                                       entries; tk_basecall_beamsearch_dev: row_off does not fit total_rows;
                                       tk_basecall_mod_weights_dev: a read's rows did not fit between its out_off entries */

/* tk_basecall_mod_weights_dev: the most modifications an alphabet may have in all (sum of can_nmods) */
#define TK_BASECALL_MAX_NMOD 32

/* library / build identification, e.g. "taiyaki_amd basecall gfx950 r2" */
const char *tk_basecall_version(void);

/* ------------------------------------------------------------------------- *
 * (a) median and MAD per read (taiyaki/maths.py:8-32 on a float32 array)
 *   signal   (sig_off[nread]) f32, the reads laid back to back
 *   sig_off  (nread + 1) int64, ascending
 *   med, mad (nread) f32:
 *     med = the middle order statistic; for an even count the mean of the two middle values, (a + b) / 2 in float32
 *     mad = 1.4826f * median(|x - med|): subtraction, absolute value, median and the product in float32 (what numpy
 *           computes when the Python float 1.4826 meets a float32 value)
 * One workgroup per read; radix SELECTION on the order-preserving integer key of the floats (four 8-bit passes per
 * median, both middle ranks in one pass), histograms in LDS, integer counting only: no float atomics, bit-identical
 * from run to run and in any batch.
 * DEPARTURE from the reference: a read with a non-finite sample, with no samples, or with mad == 0 gets med = mad = NaN
 * and TK_STATUS_BAD_SIGNAL in *status (the caller reports an empty call for it).  The reference propagates the NaN
 * through the network, fails on the empty array, or divides by zero there.
 * ------------------------------------------------------------------------- */
int tk_signal_med_mad_dev(const float *signal, const int64_t *sig_off, size_t nread, float *med, float *mad,
                          uint32_t *status, void *stream);

/* ------------------------------------------------------------------------- *
 * (b) chunk_read (basecall_helpers.py:11-43) of the normalised signal, for every read of the batch at once
 *   chunks of read r, of length len >= chunk_size (samples; overlap < chunk_size):
 *     count  = tk_basecall_chunk_count(len, chunk_size, overlap) = (len - chunk_size + step - 1) / step + 1,
 *              step = chunk_size - overlap (a closed form of the length: the host sums it into total_chunks)
 *     ends   = chunk_size + i * step for all but the last chunk, len for the last; starts = ends - chunk_size
 *   a read with len < chunk_size has NO chunk here (count 0): the reference calls it as one chunk of its own length,
 *   and the network's result depends on that length, so the caller runs it alone -- with this entry point, for that
 *   read, at chunk_size = len and overlap = 0.
 *   signal, sig_off, nread  as in (a); nsignal = sig_off[nread] (bounds every read of `signal`)
 *   shift, scale  (nread) f32: (a)'s med / mad, or the caller's own (bin/basecall.py:198, --scaling)
 *   chunks        (chunk_size, total_chunks, 1) f32 = (x - shift[r]) / scale[r], IEEE float32 subtract and divide;
 *                 where shift[r] or scale[r] is NaN (a read that (a) refused) the chunk is all zeros
 *   chunk_starts, chunk_ends (total_chunks) int64, in samples of their read; read_chunk_off (nread + 1) int64
 *   workspace     tk_basecall_gather_workspace_bytes(total_chunks) bytes, 16-byte aligned
 * Two kernels are enqueued: the plan (offsets, starts, ends: one workgroup) and the gather (a tiled transpose:
 * coalesced reads along the signal, coalesced writes along the chunks).  If total_chunks disagrees with the lengths,
 * TK_STATUS_CHUNK_PLAN is set, chunks the lengths do not give are zero-filled and chunks beyond total_chunks are
 * not written.
 * ------------------------------------------------------------------------- */
size_t tk_basecall_chunk_count(size_t siglen, size_t chunk_size, size_t overlap);    /* host arithmetic, no device work */
size_t tk_basecall_gather_workspace_bytes(size_t total_chunks);
int tk_basecall_gather_chunks_dev(const float *signal, const int64_t *sig_off, size_t nread, size_t nsignal,
                                  const float *shift, const float *scale, size_t chunk_size, size_t overlap,
                                  size_t total_chunks, float *chunks, int64_t *chunk_starts, int64_t *chunk_ends,
                                  int64_t *read_chunk_off, void *workspace, size_t workspace_bytes, uint32_t *status,
                                  void *stream);

/* ------------------------------------------------------------------------- *
 * (c) the tail: stitch, collapse, quality characters -- one workgroup per read
 *   path      (nblk + 1, nchunks) int64 flip-flop states (tk_flipflop_viterbi_dev)
 *   errprobs  (nblk + 1, nchunks) f32 (tk_flipflop_errprobs_dev), or NULL: fasta, `qual` is not touched
 *   chunk_starts, chunk_ends (nchunks) int64; read_chunk_off (nread + 1) int64: read r owns chunks
 *             [read_chunk_off[r], read_chunk_off[r + 1]) (as (b) wrote them)
 *   read_scale (nread) f32 or NULL: a read whose entry is NaN ((a) refused it) gets seqlen 0
 *   stride    samples per block; nbase, alphabet: `alphabet` is a HOST pointer to nbase <= 16 bytes
 *   seq, qual uint8; read r's characters start at out_off[r]; out_off (nread + 1) int64: the caller sizes read r's
 *             room from its stitched row count, which bounds the call length; seqlen (nread) int32
 * Stitching is stitch_chunks with path_stitching=False (as bin/basecall.py:223-231 calls it) on both tensors; the cuts
 * are computed here with the reference's integer floor divisions for the first, middle and last chunk, and a read of
 * one chunk keeps all its rows.  Stitched row k >= 1 is a MOVE when its state differs from stitched row k - 1, also
 * across a cut, where the two rows come from different chunks.  A move emits alphabet[state % nbase] and, with
 * errprobs e, the character (qscores.py:10-55, numpy's float32 arithmetic, one operation at a time)
 *     q = qscore_scale * (-10 * log10(e)) + qscore_offset;  code = (int)((q + 33) + 0.5)   (truncated toward zero)
 * TWO DEPARTURES from the reference, both where it has no defined answer:
 *   - the code is clamped to [33, 126] ('!' .. '~'): at e == 0 the reference converts +inf to int8;
 *   - a NaN q gives '!': e < 0 is the -1 that row 0 of the error probabilities holds, which only a later chunk with a
 *     zero overlap can select.
 * The device's log10f is the one operation that may differ from numpy's in the last place, so a character may sit one
 * step away from numpy's where q + 33.5 lies on an integer.
 * ------------------------------------------------------------------------- */
int tk_basecall_call_dev(const int64_t *path, const float *errprobs, size_t nblk, size_t nchunks,
                         const int64_t *chunk_starts, const int64_t *chunk_ends, const int64_t *read_chunk_off,
                         const float *read_scale, size_t nread, size_t stride, size_t nbase, const char *alphabet,
                         float qscore_scale, float qscore_offset, const int64_t *out_off, uint8_t *seq, uint8_t *qual,
                         int32_t *seqlen, uint32_t *status, void *stream);

/* ------------------------------------------------------------------------- *
 * (d) the stitched transition scores of every read of a batch: stitch_chunks(trans, starts, ends, stride) with
 *     path_stitching=False (basecall_helpers.py:46-94, as bin/basecall.py:216-218 calls it for --beam), all reads at once
 *   trans     (nblk, nchunks, ntrans) f32: the network's scores or the log transition weights of every chunk
 *   chunk_starts, chunk_ends, read_chunk_off, read_scale, stride   as in (c)
 *   row_off   (nread + 1) int64: read r's rows go to [row_off[r], row_off[r + 1]) of `stitched`; the caller sizes the
 *             room from the read's stitched row count (a closed form of its length, as for (c))
 *   stitched  (total_rows, ntrans) f32, packed: row stride ntrans;  total_rows bounds every read
 *   nrows     (nread) int32: the rows read r actually got
 * The cuts are (c)'s -- the same device function.  A read of one chunk keeps all its rows; a read without chunks, or
 * whose read_scale entry is NaN, gets no rows.  A pure copy: every output float is bit for bit an input float, rows of
 * `stitched` past a read's count are not touched.  If a read has more rows than room, TK_STATUS_CHUNK_PLAN is set,
 * the rows that fit are written and nrows[r] is the room.
 * ------------------------------------------------------------------------- */
int tk_basecall_stitch_scores_dev(const float *trans, size_t nblk, size_t nchunks, size_t ntrans,
                                  const int64_t *chunk_starts, const int64_t *chunk_ends,
                                  const int64_t *read_chunk_off, const float *read_scale, size_t nread, size_t stride,
                                  const int64_t *row_off, size_t total_rows, float *stitched, int32_t *nrows,
                                  uint32_t *status, void *stream);

/* ------------------------------------------------------------------------- *
 * (e) the hash beam search (decodeutil.pyx:9-51, c_hashdecode.c:346-507) for reads of different lengths in ONE launch,
 *     one wavefront per read -- the kernel body of tk_flipflop_beamsearch_dev, and its results to the last bit -- and
 *     each read's call
 *   scores    (total_rows, ntrans) f32 packed as (d) writes it, ntrans = 2 nbase (nbase + 1); row_off as in (d)
 *   nrows     (nread) int32, DEVICE: the rows of read r (clamped to [0, row_off[r + 1] - row_off[r]])
 *   max_rows  the longest room of the launch (host arithmetic on row_off): sizes the back-pointer window in LDS; reads
 *             past 3584 rows walk their back-pointers in HBM
 *   nbase 1..4; beam_width 1..12 with beam_width * (nbase + 1) <= 64 (else TK_ERR_UNSUPPORTED); beam_cut in [0, 1]
 *             (else TK_ERR_BAD_ARG); guided: 0 / 1; alphabet: a HOST pointer to nbase bytes
 *   states    int8, read r's flip-flop states from row_off[r]; nstate (nread) int32 their count; score (nread) f32
 *   seq       uint8, from row_off[r]: alphabet[state % nbase] of every state after the first that differs from its
 *             predecessor (path_to_str(states, include_first_source=False)); seqlen (nread) int32 its length
 *   workspace tk_basecall_beamsearch_workspace_bytes(total_rows, nread, nbase) bytes: the guiding backward matrix and
 *             the back-pointer table of every read, at the prefix offsets row_off gives
 * A read of 0 rows gives nstate 0, seqlen 0, score 0.  Nothing is written past a read's counts.  The launch lasts as
 * long as its longest read.  A row_off entry outside [0, total_rows] sets TK_STATUS_CHUNK_PLAN and its read gets 0 rows.
 * ------------------------------------------------------------------------- */
size_t tk_basecall_beamsearch_workspace_bytes(size_t total_rows, size_t nread, size_t nbase);
int tk_basecall_beamsearch_dev(const float *scores, const int64_t *row_off, const int32_t *nrows, size_t nread,
                               size_t total_rows, size_t max_rows, size_t nbase, const char *alphabet, int beam_width,
                               float beam_cut, int guided, int8_t *states, int32_t *nstate, float *score, uint8_t *seq,
                               int32_t *seqlen, void *workspace, size_t workspace_bytes, uint32_t *status,
                               void *stream);

/* ------------------------------------------------------------------------- *
 * (f) the modified-base weights of every read's call: flipflopfings.py:100-143 extract_mod_weights(W, P, can_nmods)
 *     without its first row, on P = stitch_chunks(path) and W = stitch_chunks(mod_weights) (path_stitching=False, the
 *     cuts of (c): the same device function) -- all reads of a batch in one launch, one workgroup per read
 *   path        (nblk + 1, nchunks) int64, as in (c)
 *   mod_weights (nblk, nchunks, ncat) f32, contiguous: the columns of a GlobalNormFlipFlopCatMod output from
 *               2 nbase (nbase + 1) on, ncat = nbase + nmod log-probabilities in the layer's grouped order
 *               [base 0 unmodified, its modifications ..., base 1 unmodified, its modifications ..., ...]
 *               (nblk == 0, a read too short for a block: may be NULL, nothing is read from it)
 *   chunk_starts, chunk_ends, read_chunk_off, read_scale, nread, stride   as in (c)
 *   can_nmods   a HOST pointer to nbase <= 16 ints >= 0: the modifications of each canonical base;
 *               nmod = their sum, 1 .. TK_BASECALL_MAX_NMOD (0, a negative entry or NULL: TK_ERR_BAD_ARG; more:
 *               TK_ERR_UNSUPPORTED)
 *   out_off     (nread + 1) int64, in rows: the offsets (c) takes for `seq`
 *   mods        f32, packed: read r's rows start at row out_off[r], row stride nmod
 *   seqlen      (nread) int32: the rows of read r, which is what (c) writes there -- both kernels run the same walk
 * Stitched row k >= 1 is a move when P[k] != P[k - 1] ((c)'s rule, also across a cut).  The i-th move, into base
 * b = P[k] % nbase, writes row i: column j of the nmod columns, if it is the m-th modification of base b, gets
 * W[k - 1][off_b + 1 + m] with off_b = sum over b' < b of (can_nmods[b'] + 1) -- the weight row of stitched row k - 1,
 * from the chunk that holds it; every other column gets the quiet NaN 0x7fc00000.  Row i belongs to character i of (c)'s
 * call (the reference's row 0, the never-entered first state, is the row path_to_str(include_first_source=False) drops).
 * A read of one chunk keeps all its rows: P has nblk + 1 of them, W nblk.  With more chunks every kept row of a chunk
 * lies below nblk for any chunk geometry (b) produces; should a cut keep a chunk's path row nblk, which has no weight
 * row, a move out of it gets NaN in every column.
 * A pure selection: every finite output float is bit for bit an input float; nothing is written past a read's seqlen
 * rows; a read without chunks, or whose read_scale entry is NaN, gets seqlen 0 and no rows; results do not depend on
 * the batch and repeat bit for bit.  A read with more moves than room sets TK_STATUS_CHUNK_PLAN, gets the rows that fit,
 * and seqlen[r] is the room.
 * ------------------------------------------------------------------------- */
int tk_basecall_mod_weights_dev(const int64_t *path, const float *mod_weights, size_t nblk, size_t nchunks,
                                const int64_t *chunk_starts, const int64_t *chunk_ends, const int64_t *read_chunk_off,
                                const float *read_scale, size_t nread, size_t stride, size_t nbase,
                                const int *can_nmods, const int64_t *out_off, float *mods, int32_t *seqlen,
                                uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TAIYAKI_AMD_BASECALL_H */

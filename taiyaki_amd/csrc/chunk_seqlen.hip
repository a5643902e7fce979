// chunk_seqlen.hip -- training chunks of a fixed number of BASES from the device-resident mapped-signal set, and the
// squiggle trainer's batch of them (gfx950).  The C ABI of include/taiyaki_amd_chunks_seqlen.h, a library of its own.
//
// Replaces the per-batch host work of the reference's squiggle trainer, one Python object per chunk:
//   taiyaki/signal_mapping.py:556-594  SignalMapping.get_chunk_with_sequence_length
//   taiyaki/signal_mapping.py:479-513  get_current, _get_chunk (empty signal, max dwell)
//   taiyaki/signal_mapping.py:680-716  Chunk.apply_filters
//   bin/train_squiggle.py:201-209      embed_sequence per chunk, np.concatenate of the currents, H2D copies
// The sibling of chunk_kernels.hip (chunks of a fixed number of samples); the accept loop between the two launches
// here is that file's chunk_select_kernel through tk_chunks_select_dev, fed the signal lengths.
//   1. seqlen_locate   one wave per candidate (read, start base): two Ref_to_signal lookups, the wave-parallel
//                      maximum of the dwells, the three filters -> reason code
//   2. seqlen_gather   the ragged batch.  Signal: one workgroup per GS consecutive samples of the FLAT vector; a
//                      lane finds its sample's chunk by bisecting sigoff (at most 32 probes of an array that sits
//                      in L2), so int16 reads run along a read's signal and float32 writes along the flat vector,
//                      both coalesced, 6 B per sample.  Sequences: further workgroups of the same launch, one lane
//                      per (base, chunk): the base, its row of the embedding table (kernel arguments), and the
//                      chunk's length from base 0's lane.
// No atomics on data (the status word's flag is an atomicOr, like every operator's), no workgroup waits for another,
// every loop is bounded by an argument.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/taiyaki_amd_chunks_seqlen.h"

#pragma clang fp contract(off)

namespace tk {

constexpr int WAVE = 64;
// reason codes: chunk_kernels.hip's, signal_mapping.py:611-623
enum : uint8_t { CH_PASS = 0, CH_EMPTY_SEQ, CH_EMPTY_SIG, CH_SHORT, CH_NULL_MAP, CH_PATH_BUFFER, CH_MEAN_DWELL,
                 CH_MAX_DWELL, CH_NREASON };
static_assert(CH_NREASON == TK_CHUNK_NREASON, "reason codes");
constexpr double CH_TINY = 0.00000001;      // signal_mapping.py:607

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, WAVE));
    return v;
}

constexpr int LOC_WAVES = 4;

__global__ __launch_bounds__(LOC_WAVES *WAVE) void seqlen_locate_kernel(
    tk_mapped_store st, const int32_t *__restrict__ mapped_ref, const int32_t *__restrict__ cand_read,
    const int32_t *__restrict__ cand_start, const double *__restrict__ cand_frac, int ncand, int chunk_bases,
    tk_chunk_filter fp, uint8_t *__restrict__ reason, int32_t *__restrict__ refstart,
    int32_t *__restrict__ dacstart, int32_t *__restrict__ siglen, int32_t *__restrict__ maxdwell) {
    const int c = blockIdx.x * LOC_WAVES + (threadIdx.x >> 6);
    if (c >= ncand) return;                     // wave-uniform
    const int lane = threadIdx.x & (WAVE - 1);
    const int r = cand_read[c];
    uint8_t why = CH_PASS;
    int r0 = 0, d0 = 0, len = 0, mx = 1;
    if (r < 0 || (size_t)r >= st.nreads) {
        why = CH_NULL_MAP;
    } else {
        const int32_t *rts = st.ref_to_signal + st.rts_off[r];
        const int lo = mapped_ref[2 * r], hi = mapped_ref[2 * r + 1];
        const long long spare = (long long)hi - lo - chunk_bases;      // signal_mapping.py:576-578
        long long start = 0;
        if (spare > 0) {
            // start_base: given, or the fraction of the spare length a uniform draw selects
            start = cand_start ? (long long)cand_start[c]
                               : min((long long)(cand_frac[c] * (double)spare), spare - 1);
        }
        if (spare <= 0 || start >= spare || start < 0) {                // :581-583
            why = CH_SHORT;
        } else {
            // lo <= r0 and r0 + chunk_bases < hi: both lookups lie inside the read's mapped region
            r0 = lo + (int)start;
            d0 = rts[r0];                                               // :590-591
            const int d1 = rts[r0 + chunk_bases];
            if (d1 == d0) {                                             // :500-501
                why = CH_EMPTY_SIG;
            } else {
                // np.max(np.diff(Ref_to_signal[r0 : r0 + chunk_bases])) (:505-511), 1 when there is no difference
                int m = INT32_MIN;
                for (int i = r0 + lane; i + 1 < r0 + chunk_bases; i += WAVE) m = max(m, rts[i + 1] - rts[i]);
                m = wave_max_i32(m);
                mx = (chunk_bases > 1) ? m : 1;
                len = d1 - d0;
                if (fp.enabled) {                                       // :691-716, Python float arithmetic = double
                    const double sig_len = (double)len, seq_len = (double)chunk_bases;
                    const double mean_dwell = sig_len / (seq_len + CH_TINY);
                    if (sig_len / (seq_len * (double)fp.model_stride) <= fp.path_buffer) why = CH_PATH_BUFFER;
                    else if (fabs(mean_dwell - fp.median_meandwell) > fp.filter_mean_dwell * fp.mad_meandwell)
                        why = CH_MEAN_DWELL;
                    else if ((double)mx > fp.filter_max_dwell * fp.median_meandwell) why = CH_MAX_DWELL;
                }
            }
        }
    }
    if (lane == 0) {
        reason[c] = why;
        refstart[c] = r0;
        dacstart[c] = d0;
        siglen[c] = (why == CH_PASS) ? len : 0;
        maxdwell[c] = mx;
    }
}

// ---------------------------------------------------------------------------
// the batch
// ---------------------------------------------------------------------------
constexpr int GS = 256;             // samples of the flat vector per workgroup, and (base, chunk) cells per workgroup

struct EmbedTable {
    float v[4][3];                  // squiggle_match's tetrahedron, one row per base
};

__global__ __launch_bounds__(GS) void seqlen_gather_kernel(
    tk_mapped_store st, const int32_t *__restrict__ cand_read, const int32_t *__restrict__ refstart,
    const int32_t *__restrict__ dacstart, const int32_t *__restrict__ siglen, const int32_t *__restrict__ sel,
    const int64_t *__restrict__ sigoff, const int32_t *__restrict__ counts, int nwant, int chunk_bases, int reverse,
    int standardize, EmbedTable embed, unsigned sig_blocks, int64_t signal_cap, float *__restrict__ signal,
    int32_t *__restrict__ siglens, int32_t *__restrict__ seqs, float *__restrict__ seq_embed,
    uint32_t *__restrict__ status) {
    const int nsel = min(max(counts[CH_NREASON], 0), nwant);
    if (blockIdx.x < sig_blocks) {              // block-uniform
        const int64_t p = (int64_t)blockIdx.x * GS + threadIdx.x;
        if (p >= signal_cap) return;
        float v = 0.f;
        if (p < sigoff[nsel]) {
            // the chunk that holds sample p: the last j with sigoff[j] <= p (every accepted chunk has samples)
            int lo = 0, hi = nsel;              // sigoff[lo] <= p < sigoff[hi]
            for (int it = 0; it < 32 && hi - lo > 1; ++it) {
                const int mid = (lo + hi) >> 1;
                if (sigoff[mid] <= p) lo = mid;
                else hi = mid;
            }
            const int64_t end = sigoff[lo + 1];
            if (end <= signal_cap) {            // a chunk that does not fit is not written
                const int cnd = sel[lo], r = cand_read[cnd];
                const int64_t t = p - sigoff[lo];
                const int64_t pos = reverse ? (end - sigoff[lo] - 1 - t) : t;       // np.flip of the chunk
                const int16_t d = st.dacs[st.dacs_off[r] + dacstart[cnd] + pos];
                const double *sc = st.scaling + 5 * (size_t)r;
                // signal_mapping.py:474-476, float64 like numpy's int16 array (+) Python float
                double cur = ((double)d + sc[0]) * sc[1] / sc[2];
                if (standardize) cur = (cur - sc[3]) / sc[4];
                v = (float)cur;
            }
        }
        signal[p] = v;
        return;
    }
    // sequences: cell e = (base k, chunk n) of the (chunk_bases, nwant) arrays
    const int64_t e = (int64_t)(blockIdx.x - sig_blocks) * GS + threadIdx.x;
    if (e >= (int64_t)chunk_bases * nwant) return;
    const int k = (int)(e / nwant), n = (int)(e - (int64_t)k * nwant);
    int base = 0;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (n < nsel) {
        const int cnd = sel[n], r = cand_read[cnd];
        // the Reference of read r starts rts_off[r] - r entries in (one fewer entry per read)
        const int16_t *ref = st.reference + (st.rts_off[r] - r) + refstart[cnd];
        base = ref[reverse ? (chunk_bases - 1 - k) : k];
        if (base >= 0 && base < 4) {
            x0 = embed.v[base][0];
            x1 = embed.v[base][1];
            x2 = embed.v[base][2];
        }
    }
    seqs[e] = base;
    seq_embed[3 * e] = x0;
    seq_embed[3 * e + 1] = x1;
    seq_embed[3 * e + 2] = x2;
    if (k == 0) {
        siglens[n] = (n < nsel) ? siglen[sel[n]] : 0;
        if (n < nsel && sigoff[n + 1] > signal_cap && status) atomicOr(status, TK_STATUS_SEQS_OVERFLOW);
    }
}

static bool store_ok(const tk_mapped_store *s) {
    return s && s->dacs && s->dacs_off && s->ref_to_signal && s->rts_off && s->reference && s->scaling &&
           s->nreads > 0;
}

}  // namespace tk

// ---------------------------------------------------------------------------

extern "C" {

int tk_chunks_seqlen_locate_dev(const tk_mapped_store *store, const int32_t *mapped_ref, const int32_t *cand_read,
                                const int32_t *cand_start, const double *cand_frac, size_t ncand, size_t chunk_bases,
                                const tk_chunk_filter *filter, uint8_t *reason, int32_t *refstart, int32_t *dacstart,
                                int32_t *siglen, int32_t *maxdwell, void *stream) {
    if (!tk::store_ok(store) || !mapped_ref || !filter || !cand_read || (!cand_start && !cand_frac) || !reason ||
        !refstart || !dacstart || !siglen || !maxdwell || chunk_bases == 0)
        return TK_ERR_BAD_ARG;
    if (ncand == 0) return TK_OK;
    if (ncand > (size_t)INT32_MAX || chunk_bases > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    const unsigned blocks = (unsigned)((ncand + tk::LOC_WAVES - 1) / tk::LOC_WAVES);
    hipLaunchKernelGGL(tk::seqlen_locate_kernel, dim3(blocks), dim3(tk::LOC_WAVES * tk::WAVE), 0,
                       static_cast<hipStream_t>(stream), *store, mapped_ref, cand_read, cand_start, cand_frac,
                       (int)ncand, (int)chunk_bases, *filter, reason, refstart, dacstart, siglen, maxdwell);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

int tk_chunks_seqlen_gather_dev(const tk_mapped_store *store, const int32_t *cand_read, const int32_t *refstart,
                                const int32_t *dacstart, const int32_t *siglen, const int32_t *sel,
                                const int64_t *sigoff, const int32_t *counts, size_t nwant, size_t chunk_bases,
                                int reverse, int standardize, const float *embed, float *signal, size_t signal_cap,
                                int32_t *siglens, int32_t *seqs, float *seq_embed, uint32_t *status, void *stream) {
    if (!tk::store_ok(store) || !cand_read || !refstart || !dacstart || !siglen || !sel || !sigoff || !counts ||
        !embed || (signal_cap > 0 && !signal) || !siglens || !seqs || !seq_embed || chunk_bases == 0)
        return TK_ERR_BAD_ARG;
    if (nwant == 0) return TK_OK;
    if (nwant > (size_t)INT32_MAX || chunk_bases > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    const size_t sig_blocks = (signal_cap + tk::GS - 1) / tk::GS;
    const size_t seq_blocks = (nwant * chunk_bases + tk::GS - 1) / tk::GS;
    if (sig_blocks > (size_t)INT32_MAX || seq_blocks > (size_t)INT32_MAX || sig_blocks + seq_blocks > (size_t)INT32_MAX)
        return TK_ERR_UNSUPPORTED;
    tk::EmbedTable table;
    for (int b = 0; b < 4; ++b)
        for (int k = 0; k < 3; ++k) table.v[b][k] = embed[3 * b + k];
    hipLaunchKernelGGL(tk::seqlen_gather_kernel, dim3((unsigned)(sig_blocks + seq_blocks)), dim3(tk::GS), 0,
                       static_cast<hipStream_t>(stream), *store, cand_read, refstart, dacstart, siglen, sel, sigoff,
                       counts, (int)nwant, (int)chunk_bases, reverse, standardize, table, (unsigned)sig_blocks,
                       (int64_t)signal_cap, signal, siglens, seqs, seq_embed, status);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // extern "C"

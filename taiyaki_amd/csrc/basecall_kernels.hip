// basecall_kernels.hip -- the basecaller's device-side glue (gfx950) and its extern "C" boundary
// (include/taiyaki_amd_basecall.h): per-read median / MAD by radix selection, normalise + chunk, and the tail
// (stitch the Viterbi paths of overlapping chunks, collapse them into bases, quality characters); for the beam search,
// the stitched transition scores of every read, packed row after row (the search itself: basecall_beam.hip); the C entry
// of the modified-base weights (the kernel: basecall_mods.hip).
//
// Compiled with -ffp-contract=off: every float operation on a signal or an error probability is ONE IEEE float32
// operation, which is what makes the normalised chunks bit-equal to numpy's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/taiyaki_amd_basecall.h"
#include "basecall_walk.h"
#include "dispatch.h"

namespace tk {

// ------------------------------------------------------------------------------------------------------------------
// (a) median and MAD: radix select
// ------------------------------------------------------------------------------------------------------------------
// order-preserving key: float a < float b  <=>  key(a) < key(b) as unsigned integers (finite values; -0 is made +0 first)
__device__ __forceinline__ uint32_t key_of(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// one count into an LDS histogram per participating lane.  The lanes that share the first participating lane's bin --
// on a real signal's leading bytes that is nearly all of them -- are counted by ONE atomic; the rest add one each.
__device__ __forceinline__ void hist_add(uint32_t *h, uint32_t bin, bool pend) {
    const uint64_t want = __ballot(pend);
    if (want == 0) return;
    const int first = __ffsll((unsigned long long)want) - 1;
    const uint32_t lead = (uint32_t)__shfl((int)bin, first);
    const bool with_lead = pend && bin == lead;
    const uint64_t same = __ballot(with_lead);
    if ((int)(threadIdx.x & (BC_WAVE - 1)) == first) atomicAdd(&h[lead], (uint32_t)__popcll(same));
    if (pend && !with_lead) atomicAdd(&h[bin], 1u);
}

struct SelectShared {
    uint32_t hist[2][256];
    uint32_t prefix[2];     // the key bits fixed so far, per rank
    uint32_t rank[2];       // the rank that remains inside the prefix's bucket
    uint32_t bad;
};

// The keys of the two order statistics rank0 <= rank1 of v[i] = ABS ? |x[i] - centre| : x[i] + 0, i < n.
template <bool ABS>
__device__ void select_two(const float *__restrict__ x, size_t n, float centre, uint32_t rank0, uint32_t rank1,
                           SelectShared &s, uint32_t *key0, uint32_t *key1) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        s.prefix[0] = s.prefix[1] = 0;
        s.rank[0] = rank0;
        s.rank[1] = rank1;
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 512; i += BC_THREADS) (&s.hist[0][0])[i] = 0;
        __syncthreads();
        const uint32_t p0 = s.prefix[0], p1 = s.prefix[1];
        const uint32_t fixed = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        const bool split = p0 != p1;                            // the two ranks have parted: a histogram each
        const size_t nround = (n + BC_THREADS - 1) / BC_THREADS * BC_THREADS;     // whole waves reach the ballots
        for (size_t i = tid; i < nround; i += BC_THREADS) {
            const bool live = i < n;
            const float xi = live ? x[i] : 0.f;
            if (!ABS && pass == 0 && live && (__float_as_uint(xi) & 0x7f800000u) == 0x7f800000u) s.bad = 1;
            const float v = ABS ? fabsf(xi - centre) : xi + 0.f;
            const uint32_t k = key_of(v), bin = (k >> shift) & 255u;
            hist_add(s.hist[0], bin, live && ((k ^ p0) & fixed) == 0);
            if (split) hist_add(s.hist[1], bin, live && ((k ^ p1) & fixed) == 0);
        }
        __syncthreads();
        if (tid < 2) {          // one lane per rank walks its 256 counts
            const uint32_t *h = s.hist[(split && tid == 1) ? 1 : 0];
            uint32_t left = s.rank[tid], b = 0;
            while (b < 255 && left >= h[b]) left -= h[b++];
            s.rank[tid] = left;
            s.prefix[tid] |= b << shift;
        }
        __syncthreads();
    }
    *key0 = s.prefix[0];
    *key1 = s.prefix[1];
    __syncthreads();
}

__device__ __forceinline__ float middle_of(uint32_t k0, uint32_t k1, bool even) {
    const float a = float_of(k0);
    return even ? (a + float_of(k1)) / 2.0f : a;        // np.median: the mean of the two, in float32
}

__global__ __launch_bounds__(BC_THREADS) void med_mad_kernel(const float *__restrict__ signal,
                                                             const int64_t *__restrict__ sig_off,
                                                             float *__restrict__ med, float *__restrict__ mad,
                                                             uint32_t *__restrict__ status) {
    __shared__ SelectShared s;
    const int r = blockIdx.x;
    const int64_t lo = sig_off[r], hi = sig_off[r + 1];
    const size_t n = hi > lo ? (size_t)(hi - lo) : 0;
    const float nan = __uint_as_float(0x7fc00000u);
    if (threadIdx.x == 0) s.bad = 0;
    __syncthreads();
    float m = nan, d = nan;
    bool bad = n == 0 || n > 0xffffffffull;
    if (!bad) {
        const float *x = signal + lo;
        const uint32_t r0 = (uint32_t)((n - 1) / 2), r1 = (uint32_t)(n / 2);
        uint32_t k0, k1;
        select_two<false>(x, n, 0.f, r0, r1, s, &k0, &k1);
        bad = s.bad != 0;               // uniform: read after the barriers of the selection
        if (!bad) {
            m = middle_of(k0, k1, r0 != r1);
            select_two<true>(x, n, m, r0, r1, s, &k0, &k1);
            d = 1.4826f * middle_of(k0, k1, r0 != r1);
            bad = d == 0.f;
        }
    }
    if (threadIdx.x == 0) {
        med[r] = bad ? nan : m;
        mad[r] = bad ? nan : d;
        if (bad && status) atomicOr(status, TK_STATUS_BAD_SIGNAL);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// (b) chunk plan + normalise / gather
// ------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int64_t chunk_count(int64_t len, int64_t chunk_size, int64_t overlap) {
    if (len < chunk_size) return 0;
    const int64_t step = chunk_size - overlap;
    return (len - chunk_size + step - 1) / step + 1;
}

// one workgroup: read_chunk_off by a block scan over the reads, then every read's starts / ends / owner
__global__ __launch_bounds__(BC_THREADS) void chunk_plan_kernel(const int64_t *__restrict__ sig_off, int nread,
                                                                int64_t chunk_size, int64_t overlap,
                                                                int64_t total_chunks, int64_t *__restrict__ starts,
                                                                int64_t *__restrict__ ends,
                                                                int64_t *__restrict__ read_chunk_off,
                                                                int32_t *__restrict__ owner,
                                                                uint32_t *__restrict__ status) {
    __shared__ int64_t scan[BC_THREADS];
    const int tid = threadIdx.x;
    const int64_t step = chunk_size - overlap;
    int64_t carry = 0;
    for (int base = 0; base < nread; base += BC_THREADS) {
        const int r = base + tid;
        const int64_t len = r < nread ? sig_off[r + 1] - sig_off[r] : 0;
        const int64_t cnt = r < nread ? chunk_count(len, chunk_size, overlap) : 0;
        scan[tid] = cnt;
        __syncthreads();
        for (int d = 1; d < BC_THREADS; d <<= 1) {      // inclusive Hillis-Steele scan
            const int64_t add = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const int64_t first = carry + scan[tid] - cnt;
        if (r < nread) {
            read_chunk_off[r] = first;
            for (int64_t i = 0; i < cnt; ++i) {
                const int64_t c = first + i;
                if (c >= total_chunks) break;
                const int64_t e = i == cnt - 1 ? len : chunk_size + i * step;
                starts[c] = e - chunk_size;
                ends[c] = e;
                owner[c] = r;
            }
        }
        carry += scan[BC_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) {
        read_chunk_off[nread] = carry;
        if (carry != total_chunks && status) atomicOr(status, TK_STATUS_CHUNK_PLAN);
    }
    for (int64_t c = carry + tid; c < total_chunks; c += BC_THREADS) {      // chunks the lengths do not give
        starts[c] = ends[c] = 0;
        owner[c] = -1;
    }
}

constexpr int GT = 64;      // tile edge of the gather's transpose

// chunks[t][c] = (signal[read(c)][starts[c] + t] - shift) / scale: lanes along t when reading, along c when writing
__global__ __launch_bounds__(BC_THREADS) void chunk_gather_kernel(const float *__restrict__ signal,
                                                                  const int64_t *__restrict__ sig_off, int nread,
                                                                  int64_t nsignal, const float *__restrict__ shift,
                                                                  const float *__restrict__ scale,
                                                                  int64_t chunk_size, int64_t total_chunks,
                                                                  const int64_t *__restrict__ starts,
                                                                  const int32_t *__restrict__ owner,
                                                                  float *__restrict__ chunks) {
    __shared__ float tile[GT][GT + 1];
    const int64_t c0 = (int64_t)blockIdx.x * GT, t0 = (int64_t)blockIdx.y * GT;
    const int a = threadIdx.x & (GT - 1), b = threadIdx.x / GT;
    for (int cc = b; cc < GT; cc += BC_THREADS / GT) {
        const int64_t c = c0 + cc, t = t0 + a;
        float v = 0.f;
        if (c < total_chunks && t < chunk_size) {
            const int r = owner[c];
            if (r >= 0 && r < nread) {
                const int64_t lo = sig_off[r], len = sig_off[r + 1] - lo, pos = starts[c] + t;
                const float sh = shift[r], sc = scale[r];
                if (pos >= 0 && pos < len && lo >= 0 && lo + pos < nsignal && sh == sh && sc == sc)
                    v = (signal[lo + pos] - sh) / sc;
            }
        }
        tile[cc][a] = v;
    }
    __syncthreads();
    for (int tt = b; tt < GT; tt += BC_THREADS / GT) {
        const int64_t c = c0 + a, t = t0 + tt;
        if (c < total_chunks && t < chunk_size) chunks[t * total_chunks + c] = tile[a][tt];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// (c) the tail
// ------------------------------------------------------------------------------------------------------------------
// (the stitching cuts, `chunk_cut`, and the walk over a read's stitched rows, `walk_moves`: basecall_walk.h)
struct Alphabet {
    uint8_t ch[16];
};

// qscores.py:10-55 in float32, one operation at a time; clamped to '!' .. '~', NaN -> '!'
__device__ __forceinline__ uint8_t qchar(float e, float qscale, float qoffset) {
    const float q = qscale * (-10.0f * log10f(e)) + qoffset;
    const float code = (q + 33.0f) + 0.5f;
    if (!(code >= 33.0f)) return 33;        // NaN too
    if (code >= 127.0f) return 126;
    return (uint8_t)(int)code;
}

__global__ __launch_bounds__(BC_THREADS) void call_kernel(const int64_t *__restrict__ path,
                                                          const float *__restrict__ errprobs, int64_t nrow,
                                                          int64_t nchunks, const int64_t *__restrict__ starts,
                                                          const int64_t *__restrict__ ends,
                                                          const int64_t *__restrict__ read_chunk_off,
                                                          const float *__restrict__ read_scale, int64_t stride,
                                                          uint32_t nbase, Alphabet alpha, float qscale, float qoffset,
                                                          const int64_t *__restrict__ out_off,
                                                          uint8_t *__restrict__ seq, uint8_t *__restrict__ qual,
                                                          int32_t *__restrict__ seqlen,
                                                          uint32_t *__restrict__ status) {
    __shared__ WalkShared ws;
    const int r = blockIdx.x;
    const int64_t obeg = out_off[r], room = out_off[r + 1] - obeg;
    const WalkArgs walk = {path, nrow, nchunks, starts, ends, read_chunk_off, read_scale, stride};
    bool overflow = false;
    const int64_t count = walk_moves(
        walk, r, room, ws, &overflow,
        [&](int64_t at, int64_t st, int64_t row, int64_t c, int64_t, int64_t) {
            seq[obeg + at] = alpha.ch[(uint32_t)((uint64_t)st % nbase)];
            if (errprobs) qual[obeg + at] = qchar(errprobs[row * nchunks + c], qscale, qoffset);
        },
        [](int64_t, int64_t) {});
    if (overflow && status) atomicOr(status, TK_STATUS_CHUNK_PLAN);
    if (threadIdx.x == 0) seqlen[r] = call_length(count, room);
}

// ------------------------------------------------------------------------------------------------------------------
// (d) the stitched scores of every read, for the beam search
// ------------------------------------------------------------------------------------------------------------------
constexpr int STITCH_SPLIT = 8;     // workgroups per read: workgroup y copies the chunks i = y, y + 8, ... of its read

// stitched[row_off[r] + k][:] = the k-th row that stitching keeps of read r's chunks.  Every workgroup walks the cuts
// of all its read's chunks (a few integer divisions per chunk) for the row each chunk starts at, and copies its own:
// flat over (rows, S), so a row's S floats are read side by side and the writes are one contiguous run.
__global__ __launch_bounds__(BC_THREADS) void stitch_scores_kernel(const uint32_t *__restrict__ trans, int64_t nrow,
                                                                   int64_t nchunks, uint32_t S,
                                                                   const int64_t *__restrict__ starts,
                                                                   const int64_t *__restrict__ ends,
                                                                   const int64_t *__restrict__ read_chunk_off,
                                                                   const float *__restrict__ read_scale, int64_t stride,
                                                                   const int64_t *__restrict__ row_off,
                                                                   int64_t total_rows, uint32_t *__restrict__ stitched,
                                                                   int32_t *__restrict__ nrows,
                                                                   uint32_t *__restrict__ status) {
    const int r = blockIdx.x, tid = threadIdx.x;
    int64_t cbeg = read_chunk_off[r], cend = read_chunk_off[r + 1];
    cbeg = cbeg < 0 ? 0 : cbeg;
    cend = cend > nchunks ? nchunks : cend;
    const bool refused = read_scale && read_scale[r] != read_scale[r];
    const int64_t nch = refused ? 0 : cend - cbeg;
    const int64_t obeg = row_off[r];
    int64_t room = row_off[r + 1] - obeg;
    if (obeg < 0 || room < 0 || obeg + room > total_rows) room = 0;     // (nothing is written out of range)
    int64_t at = 0;             // stitched rows before chunk i
    for (int64_t i = 0; i < nch; ++i) {
        const int64_t c = cbeg + i;
        int64_t lo, hi;
        chunk_cut(starts, ends, c, i, nch, stride, nrow, &lo, &hi);
        const int64_t keep = hi > lo ? hi - lo : 0;
        if (i % STITCH_SPLIT == blockIdx.y) {
            const int64_t fit = at + keep <= room ? keep : (room > at ? room - at : 0);
            const uint32_t *src = trans + (lo * nchunks + c) * S;
            uint32_t *dst = stitched + (obeg + at) * S;
            for (int64_t e = tid; e < fit * S; e += BC_THREADS) {
                const int64_t row = e / S;
                dst[e] = src[row * nchunks * S + (e - row * S)];
            }
        }
        at += keep;
    }
    if (blockIdx.y == 0 && tid == 0) {
        nrows[r] = (int32_t)(at < room ? at : room);
        if (at > room && status) atomicOr(status, TK_STATUS_CHUNK_PLAN);
    }
}

}  // namespace tk

// ------------------------------------------------------------------------------------------------------------------
// the C ABI
// ------------------------------------------------------------------------------------------------------------------
static int launched() { return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH; }

extern "C" {

const char *tk_basecall_version(void) { return "taiyaki_amd basecall gfx950 r2"; }

int tk_signal_med_mad_dev(const float *signal, const int64_t *sig_off, size_t nread, float *med, float *mad,
                          uint32_t *status, void *stream) {
    if (!sig_off || !med || !mad) return TK_ERR_BAD_ARG;
    if (nread == 0) return TK_OK;
    if (!signal) return TK_ERR_BAD_ARG;
    if (nread > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tk::med_mad_kernel, dim3((unsigned)nread), dim3(tk::BC_THREADS), 0,
                       static_cast<hipStream_t>(stream), signal, sig_off, med, mad, status);
    return launched();
}

size_t tk_basecall_chunk_count(size_t siglen, size_t chunk_size, size_t overlap) {
    if (chunk_size == 0 || overlap >= chunk_size || siglen > (size_t)INT64_MAX) return 0;
    return (size_t)tk::chunk_count((int64_t)siglen, (int64_t)chunk_size, (int64_t)overlap);
}

size_t tk_basecall_gather_workspace_bytes(size_t total_chunks) {
    return (total_chunks * sizeof(int32_t) + 15) / 16 * 16;
}

int tk_basecall_gather_chunks_dev(const float *signal, const int64_t *sig_off, size_t nread, size_t nsignal,
                                  const float *shift, const float *scale, size_t chunk_size, size_t overlap,
                                  size_t total_chunks, float *chunks, int64_t *chunk_starts, int64_t *chunk_ends,
                                  int64_t *read_chunk_off, void *workspace, size_t workspace_bytes, uint32_t *status,
                                  void *stream) {
    if (!sig_off || !shift || !scale || !read_chunk_off || chunk_size == 0 || overlap >= chunk_size || nread == 0)
        return TK_ERR_BAD_ARG;
    if (total_chunks > 0 && (!signal || !chunks || !chunk_starts || !chunk_ends || !workspace)) return TK_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return TK_ERR_BAD_ARG;
    if (workspace_bytes < tk_basecall_gather_workspace_bytes(total_chunks)) return TK_ERR_WORKSPACE;
    const size_t ctiles = (total_chunks + tk::GT - 1) / tk::GT, ttiles = (chunk_size + tk::GT - 1) / tk::GT;
    if (nread > (size_t)INT32_MAX || nsignal > (size_t)INT64_MAX || chunk_size > (size_t)INT32_MAX ||
        ctiles > (size_t)INT32_MAX || ttiles > 65535)
        return TK_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t *owner = static_cast<int32_t *>(workspace);
    hipLaunchKernelGGL(tk::chunk_plan_kernel, dim3(1), dim3(tk::BC_THREADS), 0, s, sig_off, (int)nread,
                       (int64_t)chunk_size, (int64_t)overlap, (int64_t)total_chunks, chunk_starts, chunk_ends,
                       read_chunk_off, owner, status);
    if (launched() != TK_OK) return TK_ERR_LAUNCH;
    if (total_chunks == 0) return TK_OK;
    hipLaunchKernelGGL(tk::chunk_gather_kernel, dim3((unsigned)ctiles, (unsigned)ttiles), dim3(tk::BC_THREADS), 0, s,
                       signal, sig_off, (int)nread, (int64_t)nsignal, shift, scale, (int64_t)chunk_size,
                       (int64_t)total_chunks, chunk_starts, owner, chunks);
    return launched();
}

int tk_basecall_call_dev(const int64_t *path, const float *errprobs, size_t nblk, size_t nchunks,
                         const int64_t *chunk_starts, const int64_t *chunk_ends, const int64_t *read_chunk_off,
                         const float *read_scale, size_t nread, size_t stride, size_t nbase, const char *alphabet,
                         float qscore_scale, float qscore_offset, const int64_t *out_off, uint8_t *seq, uint8_t *qual,
                         int32_t *seqlen, uint32_t *status, void *stream) {
    if (!path || !chunk_starts || !chunk_ends || !read_chunk_off || !alphabet || !out_off || !seq || !seqlen ||
        stride == 0 || nbase == 0 || nchunks == 0)
        return TK_ERR_BAD_ARG;
    if (errprobs && !qual) return TK_ERR_BAD_ARG;
    if (nread == 0) return TK_OK;
    if (nbase > sizeof(tk::Alphabet) || nread > (size_t)INT32_MAX || nblk >= (size_t)INT32_MAX ||
        nchunks > (size_t)INT32_MAX || stride > (size_t)INT32_MAX)
        return TK_ERR_UNSUPPORTED;
    tk::Alphabet alpha;
    memset(&alpha, 0, sizeof(alpha));
    memcpy(alpha.ch, alphabet, nbase);
    hipLaunchKernelGGL(tk::call_kernel, dim3((unsigned)nread), dim3(tk::BC_THREADS), 0,
                       static_cast<hipStream_t>(stream), path, errprobs, (int64_t)nblk + 1, (int64_t)nchunks,
                       chunk_starts, chunk_ends, read_chunk_off, read_scale, (int64_t)stride, (uint32_t)nbase, alpha,
                       qscore_scale, qscore_offset, out_off, seq, qual, seqlen, status);
    return launched();
}

int tk_basecall_stitch_scores_dev(const float *trans, size_t nblk, size_t nchunks, size_t ntrans,
                                  const int64_t *chunk_starts, const int64_t *chunk_ends,
                                  const int64_t *read_chunk_off, const float *read_scale, size_t nread, size_t stride,
                                  const int64_t *row_off, size_t total_rows, float *stitched, int32_t *nrows,
                                  uint32_t *status, void *stream) {
    if (!trans || !chunk_starts || !chunk_ends || !read_chunk_off || !row_off || !nrows || stride == 0 ||
        ntrans == 0 || nchunks == 0)
        return TK_ERR_BAD_ARG;
    if (total_rows > 0 && !stitched) return TK_ERR_BAD_ARG;
    if (nread == 0) return TK_OK;
    if (nread > (size_t)INT32_MAX || nblk >= (size_t)INT32_MAX || nchunks > (size_t)INT32_MAX ||
        stride > (size_t)INT32_MAX || ntrans > 65535 || total_rows > (size_t)INT64_MAX / 65536)
        return TK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tk::stitch_scores_kernel, dim3((unsigned)nread, tk::STITCH_SPLIT), dim3(tk::BC_THREADS), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const uint32_t *>(trans), (int64_t)nblk,
                       (int64_t)nchunks, (uint32_t)ntrans, chunk_starts, chunk_ends, read_chunk_off, read_scale,
                       (int64_t)stride, row_off, (int64_t)total_rows, reinterpret_cast<uint32_t *>(stitched), nrows,
                       status);
    return launched();
}

int tk_basecall_mod_weights_dev(const int64_t *path, const float *mod_weights, size_t nblk, size_t nchunks,
                                const int64_t *chunk_starts, const int64_t *chunk_ends, const int64_t *read_chunk_off,
                                const float *read_scale, size_t nread, size_t stride, size_t nbase,
                                const int *can_nmods, const int64_t *out_off, float *mods, int32_t *seqlen,
                                uint32_t *status, void *stream) {
    if (!path || !chunk_starts || !chunk_ends || !read_chunk_off || !can_nmods || !out_off || !mods || !seqlen ||
        stride == 0 || nbase == 0 || nchunks == 0)
        return TK_ERR_BAD_ARG;
    if (nblk > 0 && !mod_weights) return TK_ERR_BAD_ARG;    // (no block, no weight row: nothing is read from it)
    if (nbase > sizeof(tk::Alphabet)) return TK_ERR_UNSUPPORTED;
    tk::ModColumns cols;
    memset(&cols, 0, sizeof(cols));
    size_t nmod = 0, off = 0;       // off: where base b's {unmodified, its modifications} start in a weight row
    for (size_t b = 0; b < nbase; ++b) {
        if (can_nmods[b] < 0) return TK_ERR_BAD_ARG;
        if ((size_t)can_nmods[b] > TK_BASECALL_MAX_NMOD - nmod) return TK_ERR_UNSUPPORTED;
        for (int m = 0; m < can_nmods[b]; ++m, ++nmod) {
            cols.base[nmod] = (uint8_t)b;
            cols.src[nmod] = (uint8_t)(off + 1 + m);
        }
        off += 1 + can_nmods[b];
    }
    if (nmod == 0) return TK_ERR_BAD_ARG;
    if (nread == 0) return TK_OK;
    if (nread > (size_t)INT32_MAX || nblk >= (size_t)INT32_MAX || nchunks > (size_t)INT32_MAX ||
        stride > (size_t)INT32_MAX)
        return TK_ERR_UNSUPPORTED;
    return tk::mod_weights_dispatch(path, mod_weights, nblk, nchunks, nbase + nmod, chunk_starts, chunk_ends,
                                    read_chunk_off, read_scale, nread, stride, nbase, nmod, cols, out_off, mods, seqlen,
                                    status, static_cast<hipStream_t>(stream));
}

}  // extern "C"

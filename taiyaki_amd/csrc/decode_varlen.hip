// decode_varlen.hip -- include/taiyaki_amd_decode_varlen.h (libtaiyaki_amd_decode_varlen.so): the decode operators for
// batches whose columns have different lengths -- reads shorter than a chunk as zero-padded columns of one batch.
//
//   gather_columns_kernel     reads -> normalised, zero-padded columns: the tiled transpose of chunk_gather_kernel
//                             (basecall_kernels.hip), a column's read taken from a list
//   viterbi_varlen_kernel     decode.py:75-115 over lengths[n] rows: ONE WAVEFRONT PER COLUMN, lane = (to, from) =
//                             (lane / 8, lane % 8) as in viterbi_kernels.hip -- one fp32 add per candidate, the maximum
//                             over `from` inside the 8-lane group, "first index wins" from the ballot -- and that file's
//                             64-step traceback scan; the rows behind the column's length repeat its last state
//   posterior_varlen_kernel   cupy_extensions/flipflop.py:10-368 over lengths[n] rows in the linear domain: the same
//                             lane layout, the sums over a group where the Viterbi has maxima; the forward vectors go
//                             to the workspace and come back in the backward sweep, which writes the probabilities
//
// The tuned kernels of viterbi_kernels.hip and logz_kernels.hip are not touched: short reads are at most one chunk long
// and there are few of them, so these are the plain one-wave forms, written with builtins only.  A launch lasts as long
// as its longest column; no wave waits for another.
#include <stdint.h>

#include "../../include/taiyaki_amd_decode_varlen.h"
#include "ff_common.h"

namespace tk {

constexpr int DV_GRP = 8;       // lanes per state: lane = (grp, sub) = (lane / 8, lane % 8)
constexpr int DV_PF = 8;        // score rows in flight
constexpr float DV_NEG_INF = -__builtin_huge_valf();

__device__ __forceinline__ int dv_length(const int32_t *__restrict__ lengths, int n, int T) {
    return min(max(lengths[n], 0), T);
}

// decode.py:99-105 / layers.py:1253-1274: a flip state is reached from every state, flop b from flip b and from itself
template <int NB>
__device__ __forceinline__ bool dv_valid(int to, int from) {
    return to < 2 * NB && from < 2 * NB && (to < NB || from == to - NB || from == to);
}
template <int NB>
__device__ __forceinline__ int dv_sidx(int to, int from) {
    using F = FF<NB>;
    return (to < NB ? to * F::NS : F::FLOP0) + min(from, F::NS - 1);
}

// over the 8-lane group, the result in all eight lanes (and the same bits in all of them: each level adds the two
// halves' sums, and the sum of two floats does not depend on their order)
__device__ __forceinline__ float dv_grp_max(float x) {
    x = fmaxf(x, dpp_f32<0xB1>(x, x));
    x = fmaxf(x, dpp_f32<0x4E>(x, x));
    return fmaxf(x, dpp_f32<0x141>(x, x));
}
__device__ __forceinline__ float dv_grp_sum(float x) {
    x += dpp_f32<0xB1>(x, x);
    x += dpp_f32<0x4E>(x, x);
    return x + dpp_f32<0x141>(x, x);
}
// lane (grp, sub) takes the value of group `sub`
__device__ __forceinline__ float dv_transpose(float x, int tr4) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(tr4, __float_as_int(x)));
}

// ------------------------------------------------------------------------------------------------------------------
// (a) columns
// ------------------------------------------------------------------------------------------------------------------
constexpr int DV_GT = 64;           // tile edge of the transpose
constexpr int DV_THREADS = 256;

__global__ __launch_bounds__(DV_THREADS) void gather_columns_kernel(const float *__restrict__ signal,
                                                                    const int64_t *__restrict__ sig_off, int nread,
                                                                    int64_t nsignal, const float *__restrict__ shift,
                                                                    const float *__restrict__ scale,
                                                                    const int32_t *__restrict__ read_index,
                                                                    int64_t ncol, int64_t tmax,
                                                                    float *__restrict__ columns,
                                                                    int32_t *__restrict__ lengths,
                                                                    uint32_t *__restrict__ status) {
    __shared__ float tile[DV_GT][DV_GT + 1];
    const int64_t c0 = (int64_t)blockIdx.x * DV_GT, t0 = (int64_t)blockIdx.y * DV_GT;
    const int a = threadIdx.x & (DV_GT - 1), b = threadIdx.x / DV_GT;
    if (blockIdx.y == 0 && threadIdx.x < DV_GT && c0 + threadIdx.x < ncol) {       // the column's length, once
        const int r = read_index[c0 + threadIdx.x];
        int64_t len = 0;
        bool bad = r < 0 || r >= nread;
        if (!bad) {
            len = sig_off[r + 1] - sig_off[r];
            bad = len < 0 || len > tmax;
            len = min(max(len, (int64_t)0), tmax);
        }
        lengths[c0 + threadIdx.x] = (int32_t)len;
        if (bad && status) atomicOr(status, TK_STATUS_CHUNK_PLAN);
    }
    for (int cc = b; cc < DV_GT; cc += DV_THREADS / DV_GT) {                        // lanes along the signal
        const int64_t c = c0 + cc, t = t0 + a;
        float v = 0.f;
        if (c < ncol && t < tmax) {
            const int r = read_index[c];
            if (r >= 0 && r < nread) {
                const int64_t lo = sig_off[r], len = sig_off[r + 1] - lo;
                const float sh = shift[r], sc = scale[r];
                if (t < len && lo >= 0 && lo + t < nsignal && sh == sh && sc == sc) v = (signal[lo + t] - sh) / sc;
            }
        }
        tile[cc][a] = v;
    }
    __syncthreads();
    for (int tt = b; tt < DV_GT; tt += DV_THREADS / DV_GT) {                        // lanes along the columns
        const int64_t c = c0 + a, t = t0 + tt;
        if (c < ncol && t < tmax) columns[t * ncol + c] = tile[a][tt];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// A column's score rows in step order, DV_PF of them in flight: step j is row j (forward) or row len - 1 - j (REV); steps
// past the end re-read the last one (clamped, never branched).  `second`: a value of the workspace's row beside it.
// ------------------------------------------------------------------------------------------------------------------
template <bool REV>
__device__ __forceinline__ size_t dv_row(int j, int len) {
    const int jj = min(j, len - 1);
    return (size_t)(REV ? len - 1 - jj : jj);
}

// ------------------------------------------------------------------------------------------------------------------
// (b) Viterbi.  `words`: the traceback, one 8-byte word per (row, column): byte `to` = the source state of `to`.
// ------------------------------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(WAVE) void viterbi_varlen_kernel(const float *__restrict__ scores,
                                                              const int32_t *__restrict__ lengths, int T, int N,
                                                              int64_t *__restrict__ path,
                                                              unsigned char *__restrict__ tb) {
    using F = FF<NB>;
    static_assert(F::NS <= DV_GRP, "one lane group per state");
    const int lane = lane_id(), to = lane >> 3, from = lane & 7, n = blockIdx.x;
    const int len = dv_length(lengths, n, T);
    const bool valid = dv_valid<NB>(to, from);
    const float *src = scores + (size_t)n * F::S + dv_sidx<NB>(to, from);
    const size_t rowstride = (size_t)N * F::S;
    const int tr4 = 4 * ((from << 3) | to);
    unsigned char *const tb_lane = tb + (size_t)n * DV_GRP + to;
    const size_t tbstride = (size_t)N * DV_GRP;

    float f = (from < NB) ? 0.f : ((from < F::NS) ? NEG_LARGE : DV_NEG_INF);       // decode.py:93-95
    float m = DV_NEG_INF;
    if (len > 0) {
        float sc[DV_PF];
#pragma unroll
        for (int k = 0; k < DV_PF; ++k) sc[k] = src[dv_row<false>(k, len) * rowstride];
        for (int t0 = 0; t0 < len; t0 += DV_PF) {
#pragma unroll
            for (int k = 0; k < DV_PF; ++k) {
                if (t0 + k < len) {                                                 // (wave-uniform)
                    const float cand = f + (valid ? sc[k] : DV_NEG_INF);
                    sc[k] = src[dv_row<false>(t0 + k + DV_PF, len) * rowstride];
                    m = dv_grp_max(cand);
                    f = dv_transpose(m, tr4);
                    // "first index wins": the lowest set bit of the group's byte of the ballot (candidate == maximum)
                    const unsigned long long eq = __ballot(cand == m);
                    const unsigned bits = (unsigned)(eq >> (8 * to));
                    const unsigned arg = (unsigned)__builtin_ctz((bits & 0xffu) | 0x100u) & 7u;
                    if (from == 0) tb_lane[(size_t)(t0 + k) * tbstride] = (unsigned char)arg;
                }
            }
        }
    }
    // ---- decode.py:108-113: argmax of the last row = first maximal state (group s holds state s)
    unsigned st = 0;
    {
        float top = __shfl(m, 0, WAVE);
        if (len == 0) top = 0.f;
#pragma unroll
        for (int s = 1; s < F::NS; ++s) {
            float v = __shfl(m, s * DV_GRP, WAVE);
            if (len == 0) v = (s < NB) ? 0.f : NEG_LARGE;
            if (v > top) {
                top = v;
                st = s;
            }
        }
    }
    for (int t = len + lane; t <= T; t += WAVE) path[(size_t)t * N + n] = (int64_t)st;      // row len and the padding
    if (len == 0) return;
    // ---- the walk, 64 steps at a time (viterbi_kernels.hip): a step's word IS the table state -> previous state and
    // v_perm_b32 composes two tables, so an inclusive scan over the lanes leaves in lane k the composition of steps
    // 0..k of the batch; one look-up with the batch's start state gives every lane its own state.  The bytes were
    // stored by this wave: they have to have landed before its loads.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long *words = reinterpret_cast<const unsigned long long *>(tb) + n;
    auto load_batch = [&](int thi) {                            // lane k: the word of step thi - 1 - k
        const int t = max(thi - 1 - lane, 0);                   // clamped, never branched
        return words[(size_t)t * N];
    };
    unsigned long long next = load_batch(len);
    for (int thi = len; thi > 0; thi -= WAVE) {
        const unsigned long long cur = next;
        next = load_batch(thi - WAVE);
        unsigned lo = (unsigned)cur, hi = (unsigned)(cur >> 32);
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const int src4 = 4 * (lane - d);                    // (wraps for lane < d: not used there)
            const unsigned blo = (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)lo);
            const unsigned bhi = (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)hi);
            // (this step's table) o (the steps before): entry s = mine[theirs[s]]
            const unsigned nlo = __builtin_amdgcn_perm(hi, lo, blo), nhi = __builtin_amdgcn_perm(hi, lo, bhi);
            if (lane >= d) {
                lo = nlo;
                hi = nhi;
            }
        }
        const unsigned mine = __builtin_amdgcn_perm(hi, lo, st) & 0xffu;
        const int t = thi - 1 - lane;
        if (t >= 0) path[(size_t)t * N + n] = (int64_t)mine;
        st = (unsigned)__builtin_amdgcn_readlane((int)mine, WAVE - 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// (c) posterior.  w = exp(s - row maximum) for every transition of a row; the forward sweep keeps the state vector f_t
// (before row t) in `fws` [t][n][8]; the backward sweep holds b_{t+1} and writes, for row t,
//     trans[to, from] = f_t[from] w[to, from] b_{t+1}[to] / (their sum over the row).
// Both vectors are rescaled at every step by the power of two of their sum: exact, and every row is normalised by its
// own sum, so the scales never meet a result.
// ------------------------------------------------------------------------------------------------------------------
// exp(d) for d <= 0 with the product d * log2(e) carried in two floats: a relative error of an ulp or two of v_exp_f32
__device__ __forceinline__ float dv_exp(float d) {
    constexpr float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.925963033500822e-8f;
    const float hi = d * L2E_HI;
    const float lo = __builtin_fmaf(d, L2E_HI, -hi) + d * L2E_LO;
    const float w = fast_exp2(hi);
    return __builtin_fmaf(w, lo * LN2, w);
}

// exact: x / 2^e; *e_out = the exponent of the group's sum of x (0 where the sum is not a positive finite number)
__device__ __forceinline__ float dv_rescale(float x, int *e_out) {
    const float tot = dv_grp_sum(x);
    const int e = (tot > 0.f && tot < __builtin_huge_valf()) ? __builtin_amdgcn_frexp_expf(tot) : 0;
    *e_out = e;
    return __builtin_amdgcn_ldexpf(x, -e);
}

template <int NB>
__global__ __launch_bounds__(WAVE) void posterior_varlen_kernel(const float *__restrict__ scores,
                                                                const int32_t *__restrict__ lengths, int T, int N,
                                                                float *__restrict__ trans, float *__restrict__ logz,
                                                                float *__restrict__ fws,
                                                                uint32_t *__restrict__ status) {
    using F = FF<NB>;
    static_assert(F::NS <= DV_GRP && F::S <= WAVE, "one lane group per state, one lane per transition");
    const int lane = lane_id(), grp = lane >> 3, sub = lane & 7, n = blockIdx.x;
    const int len = dv_length(lengths, n, T);
    const size_t rowstride = (size_t)N * F::S, fstride = (size_t)N * DV_GRP;
    const int tr4 = 4 * ((sub << 3) | grp);
    float *const f_col = fws + (size_t)n * DV_GRP;
    bool bad = false;

    // ---- forward: lane (to, from) = (grp, sub); f = f_t[from]
    {
        const bool valid = dv_valid<NB>(grp, sub);
        const float *src = scores + (size_t)n * F::S + dv_sidx<NB>(grp, sub);
        float f = (sub < NB) ? 1.f : 0.f;                       // flipflop.py:115-118: exp(0) for a flip, exp(-LARGE) for a flop
        double lz = 0.0;
        int esum = 0;
        if (len > 0) {
            float sc[DV_PF];
#pragma unroll
            for (int k = 0; k < DV_PF; ++k) sc[k] = src[dv_row<false>(k, len) * rowstride];
            for (int t0 = 0; t0 < len; t0 += DV_PF) {
#pragma unroll
                for (int k = 0; k < DV_PF; ++k) {
                    if (t0 + k < len) {                                             // (wave-uniform)
                        const float s = valid ? sc[k] : DV_NEG_INF;
                        sc[k] = src[dv_row<false>(t0 + k + DV_PF, len) * rowstride];
                        if (grp == 0) f_col[(size_t)(t0 + k) * fstride + sub] = f;
                        const float mx = wave_allmax_dpp(s);                        // (off the chain)
                        const float w = valid ? dv_exp(s - mx) : 0.f;
                        const float a = dv_grp_sum(f * w);                          // the new state `to`, in its group
                        int e;
                        f = dv_rescale(dv_transpose(a, tr4), &e);
                        lz += (double)mx;
                        esum += e;
                    }
                }
            }
        }
        const float last = dv_grp_sum(f);
        const float z = (float)(lz + (double)esum * 0.6931471805599453 + log((double)last));
        if (!(z - z == 0.f)) bad = true;
        if (logz != nullptr && lane == 0) logz[n] = z;
        if (bad && status && lane == 0) atomicOr(status, TK_STATUS_NONFINITE_SCORE);
    }

    // ---- the rows behind the column's length: exactly 0
    for (int t = len; t < T; ++t)
        if (lane < F::S) trans[(size_t)t * rowstride + (size_t)n * F::S + lane] = 0.f;
    if (len == 0) return;
    // the forward vectors were stored by this wave: they have to have landed before its loads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);

    // ---- backward: lane (from, to) = (grp, sub); b = b_{t+1}[to]
    {
        const bool valid = dv_valid<NB>(sub, grp);
        const int sidx = dv_sidx<NB>(sub, grp);
        const float *src = scores + (size_t)n * F::S + sidx;
        float *dst = trans + (size_t)n * F::S + sidx;
        float b = (sub < F::NS) ? 1.f : 0.f;                    // flipflop.py:163-166: uniform (its scale cancels)
        bool nonfinite = false;
        float sc[DV_PF], ft[DV_PF];
#pragma unroll
        for (int k = 0; k < DV_PF; ++k) {
            sc[k] = src[dv_row<true>(k, len) * rowstride];
            ft[k] = f_col[dv_row<true>(k, len) * fstride + grp];
        }
        for (int j0 = 0; j0 < len; j0 += DV_PF) {
#pragma unroll
            for (int k = 0; k < DV_PF; ++k) {
                if (j0 + k < len) {                                                 // (wave-uniform)
                    const size_t t = (size_t)(len - 1 - (j0 + k));
                    const float s = valid ? sc[k] : DV_NEG_INF, fr = ft[k];
                    sc[k] = src[dv_row<true>(j0 + k + DV_PF, len) * rowstride];
                    ft[k] = f_col[dv_row<true>(j0 + k + DV_PF, len) * fstride + grp];
                    const float mx = wave_allmax_dpp(s);
                    const float w = valid ? dv_exp(s - mx) : 0.f;
                    const float wb = w * b;
                    // ---- off the chain: the row's probabilities
                    const float num = fr * wb;
                    const float p = num / wave_allsum(num);
                    if (valid) dst[t * rowstride] = p;
                    nonfinite |= valid && !(p - p == 0.f);
                    // ---- the chain: b_t[from] in its group, then by `to` again
                    int e;
                    b = dv_rescale(dv_transpose(dv_grp_sum(wb), tr4), &e);
                }
            }
        }
        if (__ballot(nonfinite) != 0ull && status && lane == 0) atomicOr(status, TK_STATUS_NONFINITE_GRAD);
    }
}

static int dv_launched() { return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH; }

}  // namespace tk

extern "C" {

int tk_basecall_gather_columns_dev(const float *signal, const int64_t *sig_off, size_t nread, size_t nsignal,
                                   const float *shift, const float *scale, const int32_t *read_index, size_t ncol,
                                   size_t tmax, float *columns, int32_t *lengths, uint32_t *status, void *stream) {
    if (!sig_off || !shift || !scale || nread == 0) return TK_ERR_BAD_ARG;
    if (ncol == 0) return TK_OK;
    if (!read_index || !lengths || (nsignal > 0 && !signal) || (tmax > 0 && !columns)) return TK_ERR_BAD_ARG;
    const size_t ctiles = (ncol + tk::DV_GT - 1) / tk::DV_GT, ttiles = (tmax + tk::DV_GT - 1) / tk::DV_GT;
    if (nread > (size_t)INT32_MAX || nsignal > (size_t)INT64_MAX || tmax > (size_t)INT32_MAX ||
        ctiles > (size_t)INT32_MAX || ttiles > 65535)
        return TK_ERR_UNSUPPORTED;
    // (tmax == 0: one row of tiles all the same, for the lengths)
    hipLaunchKernelGGL(tk::gather_columns_kernel, dim3((unsigned)ctiles, (unsigned)(ttiles ? ttiles : 1)),
                       dim3(tk::DV_THREADS), 0, static_cast<hipStream_t>(stream), signal, sig_off, (int)nread,
                       (int64_t)nsignal, shift, scale, read_index, (int64_t)ncol, (int64_t)tmax, columns, lengths,
                       status);
    return tk::dv_launched();
}

size_t tk_decode_varlen_workspace_bytes(size_t nblk, size_t nbatch, size_t nbase) {
    if (nbase < 1 || nbase > 4) return 0;
    // (b): 8 bytes per row and column; (c): 8 floats per row and column
    return (nblk ? nblk : 1) * (nbatch ? nbatch : 1) * tk::DV_GRP * sizeof(float);
}

int tk_flipflop_viterbi_varlen_dev(const float *scores, const int32_t *lengths, size_t nblk, size_t nbatch,
                                   size_t nbase, int64_t *path, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    if (nbase < 1 || nbase > 4) return TK_ERR_UNSUPPORTED;
    if (nbatch == 0) return TK_OK;
    if (!lengths || !path || !workspace || (nblk > 0 && !scores)) return TK_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return TK_ERR_BAD_ARG;
    if (workspace_bytes < tk_decode_varlen_workspace_bytes(nblk, nbatch, nbase)) return TK_ERR_WORKSPACE;
    if (nblk >= (size_t)INT32_MAX || nbatch > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char *tb = static_cast<unsigned char *>(workspace);
#define TK_DV_VITERBI(NB)                                                                                              \
    hipLaunchKernelGGL(tk::viterbi_varlen_kernel<NB>, dim3((unsigned)nbatch), dim3(tk::WAVE), 0, s, scores, lengths,   \
                       (int)nblk, (int)nbatch, path, tb)
    switch (nbase) {
        case 1: TK_DV_VITERBI(1); break;
        case 2: TK_DV_VITERBI(2); break;
        case 3: TK_DV_VITERBI(3); break;
        default: TK_DV_VITERBI(4); break;
    }
#undef TK_DV_VITERBI
    return tk::dv_launched();
}

int tk_flipflop_posterior_varlen_dev(const float *scores, const int32_t *lengths, size_t nblk, size_t nbatch,
                                     size_t nbase, float *trans, float *logz, void *workspace,
                                     size_t workspace_bytes, uint32_t *status, void *stream) {
    if (nbase < 1 || nbase > 4) return TK_ERR_UNSUPPORTED;
    if (nbatch == 0) return TK_OK;
    if (!lengths || !workspace || (nblk > 0 && (!scores || !trans))) return TK_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return TK_ERR_BAD_ARG;
    if (workspace_bytes < tk_decode_varlen_workspace_bytes(nblk, nbatch, nbase)) return TK_ERR_WORKSPACE;
    if (nblk >= (size_t)INT32_MAX || nbatch > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *fws = static_cast<float *>(workspace);
#define TK_DV_POSTERIOR(NB)                                                                                            \
    hipLaunchKernelGGL(tk::posterior_varlen_kernel<NB>, dim3((unsigned)nbatch), dim3(tk::WAVE), 0, s, scores, lengths, \
                       (int)nblk, (int)nbatch, trans, logz, fws, status)
    switch (nbase) {
        case 1: TK_DV_POSTERIOR(1); break;
        case 2: TK_DV_POSTERIOR(2); break;
        case 3: TK_DV_POSTERIOR(3); break;
        default: TK_DV_POSTERIOR(4); break;
    }
#undef TK_DV_POSTERIOR
    return tk::dv_launched();
}

}  // extern "C"

// loss_varlen_fused.h -- the body of the fused loss with a time length per column, ONE copy for its two entry points:
// tk_flipflop_loss_fused_varlen_labels_dev (loss_varlen_api.hip: the log-partition is the one-wave posterior with lengths)
// and tk_flipflop_loss_fused_varlen_blocks_labels_dev (logz_varlen_api.hip: kernel B's -DTK_LOGZ_VARLEN build).  Both files
// are compiled -DTK_LOSS_VARLEN (CrfCall::lengths); the log-partition call is the only thing they differ in.
#pragma once
#include "../../include/taiyaki_amd_flipflop.h"
#include "crf_band.h"
#include "dispatch.h"

namespace {

bool labels_ok(const tk_seq_labels *labels, const int32_t *modidx, tk::SeqLabels *out) {
    if (labels == nullptr || labels->nbase == 0 || (labels->seqs == nullptr && labels->total_len != 0)) return false;
    if ((labels->mod_cats != nullptr) != (modidx != nullptr)) return false;
    *out = tk::SeqLabels{labels->seqs, labels->total_len, labels->nbase, labels->mod_cats, labels->can_mods_offsets,
                         labels->mod_cat_weights, labels->bulk_seqlen};
    return true;
}

// rows of S floats -> their first S0 columns, contiguous (the canonical block of a cat-mod tensor)
__global__ void slice_cols_kernel(const float *__restrict__ src, float *__restrict__ dst, size_t nrows, int S, int S0) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows * (size_t)S0) return;
    const size_t r = i / (size_t)S0;
    dst[i] = src[r * (size_t)S + (i - r * (size_t)S0)];
}

size_t compact_bytes(size_t nblk, size_t nbatch, size_t ncan) { return (nblk * nbatch * ncan * sizeof(float) + 255) / 256 * 256; }

// the log-partition's gradient on the canonical columns; cat-mod: a compact copy of those columns in front of it
size_t loss_varlen_aux_bytes(size_t nblk, size_t nbatch, size_t nbase, size_t ntrans) {
    const size_t ncan = 2 * nbase * (nbase + 1);
    return ntrans < ncan ? 0 : (ntrans > ncan ? 2 : 1) * compact_bytes(nblk, nbatch, ncan);
}

// `logz_varlen`: (scores, lengths, nblk, nbatch, nbase, trans, logz, workspace, workspace_bytes, status, stream) -> TK_*,
// the contract of tk_flipflop_posterior_varlen_dev; `supported`: (nblk, nbatch, nbase) -> whether that call takes the
// shape, asked before anything is launched
template <class LogzVarlen, class Supported>
int loss_fused_varlen_body(const float *scores, size_t nblk, size_t nbatch, size_t ntrans, const tk_seq_labels *labels,
                           const int32_t *seqlen, int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx,
                           float *modfact, size_t max_seqlen, float sharpfact, float grad_scale,
                           const float *grad_scale_per_read, float *lossvector, float *grad, float *logz,
                           void *crf_workspace, size_t crf_workspace_bytes, void *logz_workspace, size_t logz_workspace_bytes,
                           void *aux, size_t aux_bytes, uint32_t *status, void *stream, const int32_t *lengths,
                           LogzVarlen logz_varlen, Supported supported) {
    tk::SeqLabels lab;
    if (!labels_ok(labels, modidx, &lab)) return TK_ERR_BAD_ARG;
    if (!scores || !stayidx || !moveidx || !seqlen || !seqoff || !lossvector || !grad || !logz || !crf_workspace ||
        !logz_workspace || !aux || !lengths || nblk == 0 || nbatch == 0 || !(sharpfact > 0.f))
        return TK_ERR_BAD_ARG;
    if (!tk::aligned16(scores) || !tk::aligned16(grad) || !tk::aligned16(aux)) return TK_ERR_BAD_ARG;
    if ((modidx == nullptr) != (modfact == nullptr)) return TK_ERR_BAD_ARG;
    const size_t nbase = labels->nbase, ncan = 2 * nbase * (nbase + 1);
    const bool catmod = modidx != nullptr;
    if (nbase > 4) return TK_ERR_UNSUPPORTED;
    if (!catmod && ntrans != ncan) return TK_ERR_BAD_ARG;
    if (catmod && (ntrans <= ncan || ntrans > 62)) return TK_ERR_BAD_ARG;
    const size_t one = compact_bytes(nblk, nbatch, ncan);
    if (aux_bytes < (catmod ? 2 : 1) * one) return TK_ERR_WORKSPACE;
    if (!supported(nblk, nbatch, nbase)) return TK_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the log-partition with lengths first, into the compact buffers: logZ_n and d logZ_n / d scores, zeros beyond T_n
    float *x40 = catmod ? static_cast<float *>(aux) : nullptr;
    float *g40 = reinterpret_cast<float *>(static_cast<char *>(aux) + (catmod ? one : 0));
    if (catmod) {
        const size_t n = nblk * nbatch * ncan;
        hipLaunchKernelGGL(slice_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scores, x40, nblk * nbatch,
                           (int)ntrans, (int)ncan);
        if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    }
    int rc = logz_varlen(catmod ? x40 : scores, lengths, nblk, nbatch, nbase, g40, logz, logz_workspace, logz_workspace_bytes,
                         status, stream);
    if (rc != TK_OK) return rc;
    // kernel A: ctc.pyx:258-303 -- only the canonical columns are sharpened; cost / sharp.  It adds logZ_n / T_n to its
    // costs and (d logZ_n) / T_n, times the gradient multiplier, to the canonical columns of the rows it writes
    tk::CrfCall c;
    c.lp = scores;
    c.ntrans = ntrans;
    c.nblk = nblk;
    c.nbatch = nbatch;
    c.max_seqlen = max_seqlen;
    c.ncan = ncan;
    c.stay = stayidx;
    c.move = moveidx;
    c.mod = modidx;
    c.modfact = modfact;
    c.seqlen = seqlen;
    c.seqoff = seqoff;
    c.labels = &lab;
    c.sharp_can = sharpfact;
    c.sharp_mod = catmod ? 1.0f : sharpfact;
    c.out_scale = 1.0f / sharpfact;
    c.grad_scale = grad_scale;
    c.grad_scale_vec = grad_scale_per_read;
    c.cost = lossvector;
    c.grad = grad;
    c.workspace = crf_workspace;
    c.workspace_bytes = crf_workspace_bytes;
    c.status = status;
    c.stream = st;
    c.mod_col_weights = catmod ? labels->mod_cat_weights : nullptr;
    c.add_grad = g40;
    c.add_cost = logz;
    c.add_S = (int)ncan;
    c.add_scale = 1.0f / (float)nblk;       // (unused under lengths: 1 / T_n per column)
    c.lengths = lengths;
    return tk::crf_dispatch(c);
}

}  // namespace

// loss_varlen_api.hip -- the C entries of include/taiyaki_amd_loss_varlen.h (libtaiyaki_amd_loss_varlen.so).  Kernel A is
// crf_band.hip and crf_kernels.hip compiled for this library with -DTK_LOSS_VARLEN (CrfCall::lengths, crf_band.h; the
// kernels' VL = true instantiations); the log-partition half is decode_varlen.o as it is (tk_flipflop_posterior_varlen_dev).
// This file holds the argument checks, the compact copy of a cat-mod tensor's canonical columns, and the calls.
#include "../../include/taiyaki_amd_loss_varlen.h"

#include "../../include/taiyaki_amd_decode_varlen.h"
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

}  // namespace

extern "C" {

int tk_crf_flipflop_varlen_labels_dev(const float *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                                      const tk_seq_labels *labels, const int32_t *seqlen,
                                      int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                                      size_t max_seqlen, size_t ncan, float sharp_can, float sharp_mod,
                                      float out_scale, float *cost, float *grad, void *workspace,
                                      size_t workspace_bytes, uint32_t *status, void *stream, const int32_t *lengths) {
    tk::SeqLabels lab;
    if (!labels_ok(labels, modidx, &lab)) return TK_ERR_BAD_ARG;
    if (!logprob || !stayidx || !moveidx || !seqlen || !seqoff || !cost || !workspace) return TK_ERR_BAD_ARG;
    if (ntrans == 0 || nblk == 0 || nbatch == 0) return TK_ERR_BAD_ARG;
    if ((modidx == nullptr) != (modfact == nullptr)) return TK_ERR_BAD_ARG;
    tk::CrfCall c;
    c.lp = logprob;
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
    c.sharp_can = sharp_can;
    c.sharp_mod = sharp_mod;
    c.out_scale = out_scale;
    c.cost = cost;
    c.grad = grad;
    c.workspace = workspace;
    c.workspace_bytes = workspace_bytes;
    c.status = status;
    c.stream = static_cast<hipStream_t>(stream);
    // (modfact is filled from mod_cat_weights by column: the per-column form of the cat-mod kernels applies)
    c.mod_col_weights = modidx != nullptr ? labels->mod_cat_weights : nullptr;
    c.lengths = lengths;
    return tk::crf_dispatch(c);
}

size_t tk_flipflop_loss_varlen_aux_bytes(size_t nblk, size_t nbatch, size_t nbase, size_t ntrans, int which) {
    const size_t ncan = 2 * nbase * (nbase + 1);
    if (which == 1) return tk_decode_varlen_workspace_bytes(nblk, nbatch, nbase);
    if (which != 0 || ntrans < ncan) return 0;
    // the log-partition's gradient on the canonical columns; cat-mod: a compact copy of those columns in front of it
    return (ntrans > ncan ? 2 : 1) * compact_bytes(nblk, nbatch, ncan);
}

int tk_flipflop_loss_fused_varlen_labels_dev(const float *scores, size_t nblk, size_t nbatch, size_t ntrans,
                                             const tk_seq_labels *labels, const int32_t *seqlen,
                                             int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                                             size_t max_seqlen, float sharpfact, float grad_scale,
                                             const float *grad_scale_per_read, float *lossvector,
                                             float *grad, float *logz, void *crf_workspace, size_t crf_workspace_bytes,
                                             void *logz_workspace, size_t logz_workspace_bytes, void *aux, size_t aux_bytes,
                                             uint32_t *status, void *stream, const int32_t *lengths) {
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
    int rc = tk_flipflop_posterior_varlen_dev(catmod ? x40 : scores, lengths, nblk, nbatch, nbase, g40, logz, logz_workspace,
                                              logz_workspace_bytes, status, stream);
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

int tk_crf_varlen_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, int form,
                       int want_grad, float sharp, size_t workspace_bytes, size_t *out) {
    if (out == nullptr || form < 0 || form > 1) return 0;
    return tk::crf_lab_plan(ntrans, nblk, nbatch, max_seqlen, bulk_seqlen, form, want_grad, sharp, workspace_bytes, out) ? 1 : 0;
}

}  // extern "C"

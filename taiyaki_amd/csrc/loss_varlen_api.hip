// loss_varlen_api.hip -- the C entries of include/taiyaki_amd_loss_varlen.h (libtaiyaki_amd_loss_varlen.so).  Kernel A is
// crf_band.hip and crf_kernels.hip compiled for this library with -DTK_LOSS_VARLEN (CrfCall::lengths, crf_band.h; the
// kernels' VL = true instantiations); the log-partition half is decode_varlen.o as it is (tk_flipflop_posterior_varlen_dev).
// This file holds the argument checks and the calls; the fused loss's body (the compact copy of a cat-mod tensor's canonical
// columns, the log-partition call, kernel A) is loss_varlen_fused.h, shared with logz_varlen_api.hip.
#include "../../include/taiyaki_amd_loss_varlen.h"

#include "../../include/taiyaki_amd_decode_varlen.h"
#include "loss_varlen_fused.h"

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
    if (which == 1) return tk_decode_varlen_workspace_bytes(nblk, nbatch, nbase);
    return which == 0 ? loss_varlen_aux_bytes(nblk, nbatch, nbase, ntrans) : 0;
}

int tk_flipflop_loss_fused_varlen_labels_dev(const float *scores, size_t nblk, size_t nbatch, size_t ntrans,
                                             const tk_seq_labels *labels, const int32_t *seqlen,
                                             int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                                             size_t max_seqlen, float sharpfact, float grad_scale,
                                             const float *grad_scale_per_read, float *lossvector,
                                             float *grad, float *logz, void *crf_workspace, size_t crf_workspace_bytes,
                                             void *logz_workspace, size_t logz_workspace_bytes, void *aux, size_t aux_bytes,
                                             uint32_t *status, void *stream, const int32_t *lengths) {
    // (loss_varlen_fused.h: the body this entry shares with libtaiyaki_amd_logz_varlen.so's; here the log-partition is the
    // one-wave posterior with lengths, which takes every shape)
    return loss_fused_varlen_body(scores, nblk, nbatch, ntrans, labels, seqlen, seqoff, stayidx, moveidx, modidx, modfact,
                                  max_seqlen, sharpfact, grad_scale, grad_scale_per_read, lossvector, grad, logz, crf_workspace,
                                  crf_workspace_bytes, logz_workspace, logz_workspace_bytes, aux, aux_bytes, status, stream,
                                  lengths, tk_flipflop_posterior_varlen_dev, [](size_t, size_t, size_t) { return true; });
}

int tk_crf_varlen_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, int form,
                       int want_grad, float sharp, size_t workspace_bytes, size_t *out) {
    if (out == nullptr || form < 0 || form > 1) return 0;
    return tk::crf_lab_plan(ntrans, nblk, nbatch, max_seqlen, bulk_seqlen, form, want_grad, sharp, workspace_bytes, out) ? 1 : 0;
}

}  // extern "C"

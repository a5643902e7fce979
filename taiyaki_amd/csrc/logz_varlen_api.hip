// logz_varlen_api.hip -- the C entries of include/taiyaki_amd_logz_varlen.h (libtaiyaki_amd_logz_varlen.so).  Kernel B is
// logz_kernels.hip compiled for this library with -DTK_LOGZ_VARLEN (LogzWs::lengths, the kernels' VL = true instantiations);
// kernel A is the -DTK_LOSS_VARLEN objects of libtaiyaki_amd_loss_varlen.so as they are.  This file holds the argument
// checks and the calls; the fused loss's body is loss_varlen_fused.h, shared with loss_varlen_api.hip.
#include "../../include/taiyaki_amd_logz_varlen.h"

#include "loss_varlen_fused.h"

extern "C" {

size_t tk_flipflop_logz_varlen_workspace_bytes(size_t nblk, size_t nbatch, size_t nbase) {
    return tk::logz_workspace_bytes(nblk, nbatch, nbase);
}

int tk_flipflop_logz_varlen_dev(const float *scores, const int32_t *lengths, size_t nblk, size_t nbatch, size_t nbase,
                                float *trans, float *logz, void *workspace, size_t workspace_bytes, uint32_t *status,
                                void *stream) {
    if (!scores || !logz || !workspace || nblk == 0 || nbatch == 0) return TK_ERR_BAD_ARG;
    if (!tk::aligned16(scores) || (trans && !tk::aligned16(trans))) return TK_ERR_BAD_ARG;
    return tk::logz_varlen_dispatch(scores, lengths, nblk, nbatch, nbase, logz, trans, workspace, workspace_bytes, status,
                                    static_cast<hipStream_t>(stream));
}

size_t tk_flipflop_loss_varlen_blocks_aux_bytes(size_t nblk, size_t nbatch, size_t nbase, size_t ntrans, int which) {
    if (which == 1) return tk::logz_workspace_bytes(nblk, nbatch, nbase);
    if (which != 0 || nbase == 0 || nbase > 4) return 0;
    return loss_varlen_aux_bytes(nblk, nbatch, nbase, ntrans);
}

int tk_flipflop_loss_fused_varlen_blocks_labels_dev(const float *scores, size_t nblk, size_t nbatch, size_t ntrans,
                                                    const tk_seq_labels *labels, const int32_t *seqlen,
                                                    int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                                                    size_t max_seqlen, float sharpfact, float grad_scale,
                                                    const float *grad_scale_per_read, float *lossvector,
                                                    float *grad, float *logz, void *crf_workspace, size_t crf_workspace_bytes,
                                                    void *logz_workspace, size_t logz_workspace_bytes, void *aux, size_t aux_bytes,
                                                    uint32_t *status, void *stream, const int32_t *lengths) {
    return loss_fused_varlen_body(scores, nblk, nbatch, ntrans, labels, seqlen, seqoff, stayidx, moveidx, modidx, modfact,
                                  max_seqlen, sharpfact, grad_scale, grad_scale_per_read, lossvector, grad, logz, crf_workspace,
                                  crf_workspace_bytes, logz_workspace, logz_workspace_bytes, aux, aux_bytes, status, stream,
                                  lengths, tk_flipflop_logz_varlen_dev, tk::logz_varlen_supported);
}

}  // extern "C"

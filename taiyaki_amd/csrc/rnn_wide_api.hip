// rnn_wide_api.hip -- the C entries of include/taiyaki_amd_rnn_wide.h (libtaiyaki_amd_rnn_wide.so).  The slab loop and
// the launches are in lstm_kernels.hip and gru_kernels.hip, compiled for this library with -DTK_RNN_WIDE: this file
// holds nothing but the calls.
#include "../../include/taiyaki_amd_rnn_wide.h"
#include "dispatch.h"

extern "C" {

size_t tk_rnn_wide_workspace_bytes(int kind, size_t nbatch, size_t size, int cu_count) {
    if (kind == TK_RNN_KIND_LSTM) return tk::lstm_wide_workspace_bytes(nbatch, size, cu_count);
    if (kind == TK_RNN_KIND_GRU) return tk::gru_wide_workspace_bytes(nbatch, size, cu_count);
    return 0;
}

size_t tk_rnn_wide_slab(int kind, size_t nbatch, size_t size, int cu_count) {
    if (kind == TK_RNN_KIND_LSTM) return tk::lstm_wide_slab(nbatch, size, cu_count);
    if (kind == TK_RNN_KIND_GRU) return tk::gru_wide_slab(nbatch, size, cu_count);
    return 0;
}

int tk_lstm_forward_wide_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                             size_t size, int reverse, int cu_count, float *y, float *gates, float *cell,
                             void *workspace, size_t workspace_bytes, uint32_t *status, void *stream) {
    return tk::lstm_forward_wide_dispatch(gx, w_hh, lengths, nblk, nbatch, size, reverse, cu_count, y, gates, cell,
                                          workspace, workspace_bytes, status, static_cast<hipStream_t>(stream));
}

int tk_lstm_backward_wide_dev(const float *w_hh, const float *gates, const float *cell, const float *dy,
                              const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                              int cu_count, float *dgates, void *workspace, size_t workspace_bytes, uint32_t *status,
                              void *stream) {
    return tk::lstm_backward_wide_dispatch(w_hh, gates, cell, dy, lengths, nblk, nbatch, size, reverse, cu_count,
                                           dgates, workspace, workspace_bytes, status,
                                           static_cast<hipStream_t>(stream));
}

int tk_gru_forward_wide_dev(const float *gx, const float *w_hh, const float *b_hh, const int32_t *lengths, size_t nblk,
                            size_t nbatch, size_t size, int reverse, int cu_count, float *y, float *gates, float *q,
                            void *workspace, size_t workspace_bytes, uint32_t *status, void *stream) {
    return tk::gru_forward_wide_dispatch(gx, w_hh, b_hh, lengths, nblk, nbatch, size, reverse, cu_count, y, gates, q,
                                         workspace, workspace_bytes, status, static_cast<hipStream_t>(stream));
}

int tk_gru_backward_wide_dev(const float *w_hh, const float *y, const float *gates, const float *q, const float *dy,
                             const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                             int cu_count, float *dgates, float *dq, void *workspace, size_t workspace_bytes,
                             uint32_t *status, void *stream) {
    return tk::gru_backward_wide_dispatch(w_hh, y, gates, q, dy, lengths, nblk, nbatch, size, reverse, cu_count, dgates,
                                          dq, workspace, workspace_bytes, status, static_cast<hipStream_t>(stream));
}

}  // extern "C"

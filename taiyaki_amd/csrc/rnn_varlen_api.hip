// rnn_varlen_api.hip -- the C entries of include/taiyaki_amd_rnn_varlen.h (libtaiyaki_amd_rnn_varlen.so).  The launches
// are in lstm_kernels.hip and gru_kernels.hip, compiled for this library with -DTK_RNN_VARLEN: this file holds nothing
// but the calls.
#include "../../include/taiyaki_amd_rnn_varlen.h"
#include "dispatch.h"

extern "C" {

size_t tk_rnn_varlen_workspace_bytes(int kind, size_t nbatch, size_t size, int cu_count) {
    if (kind == TK_RNN_KIND_LSTM) return tk::lstm_varlen_workspace_bytes(nbatch, size, cu_count);
    if (kind == TK_RNN_KIND_GRU) return tk::gru_varlen_workspace_bytes(nbatch, size, cu_count);
    return 0;
}

int tk_lstm_forward_varlen_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                               size_t size, int reverse, int cu_count, float *y, void *workspace,
                               size_t workspace_bytes, uint32_t *status, void *stream) {
    return tk::lstm_forward_varlen_dispatch(gx, w_hh, lengths, nblk, nbatch, size, reverse, cu_count, y, workspace,
                                            workspace_bytes, status, static_cast<hipStream_t>(stream));
}

int tk_gru_forward_varlen_dev(const float *gx, const float *w_hh, const float *b_hh, const int32_t *lengths,
                              size_t nblk, size_t nbatch, size_t size, int reverse, int cu_count, float *y,
                              void *workspace, size_t workspace_bytes, uint32_t *status, void *stream) {
    return tk::gru_forward_varlen_dispatch(gx, w_hh, b_hh, lengths, nblk, nbatch, size, reverse, cu_count, y,
                                           workspace, workspace_bytes, status, static_cast<hipStream_t>(stream));
}

}  // extern "C"

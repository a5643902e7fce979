// lstm_large_api.hip -- the C entries of include/taiyaki_amd_lstm_large.h (libtaiyaki_amd_lstm_large.so).  The geometry,
// the slab loop and the launches are in lstm_kernels.hip, compiled for this library with -DTK_LSTM_LARGE: this file
// holds nothing but the calls.
#include "../../include/taiyaki_amd_lstm_large.h"
#include "dispatch.h"

extern "C" {

int tk_lstm_large_supported(size_t size) { return tk::lstm_large_supported(size); }

size_t tk_lstm_large_slab(size_t nbatch, size_t size, int cu_count) {
    return tk::lstm_large_slab(nbatch, size, cu_count);
}

size_t tk_lstm_large_workspace_bytes(size_t nbatch, size_t size, int cu_count) {
    return tk::lstm_large_workspace_bytes(nbatch, size, cu_count);
}

int tk_lstm_large_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                              size_t size, int reverse, int cu_count, float *y, float *gates, float *cell,
                              void *workspace, size_t workspace_bytes, uint32_t *status, void *stream) {
    return tk::lstm_forward_large_dispatch(gx, w_hh, lengths, nblk, nbatch, size, reverse, cu_count, y, gates, cell,
                                           workspace, workspace_bytes, status, static_cast<hipStream_t>(stream));
}

int tk_lstm_large_backward_dev(const float *w_hh, const float *gates, const float *cell, const float *dy,
                               const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                               int cu_count, float *dgates, void *workspace, size_t workspace_bytes, uint32_t *status,
                               void *stream) {
    return tk::lstm_backward_large_dispatch(w_hh, gates, cell, dy, lengths, nblk, nbatch, size, reverse, cu_count,
                                            dgates, workspace, workspace_bytes, status,
                                            static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
void tk_lab_lstm_large_cols(int cols) { tk::lstm_large_lab_cols(cols); }

int tk_lab_lstm_large_geometry(size_t nbatch, size_t size, int cu_count, size_t *out) {
    return tk::lstm_large_lab_geometry(nbatch, size, cu_count, out) ? 1 : 0;
}
#endif

}  // extern "C"

// lstm_wgrad.hip -- the parameter gradients of one LSTM layer, dG^T [x | y shifted | 1], as one split-K GEMM on the
// bf16 matrix cores, every float32 operand split into three bf16 parts, and one reduction
// (include/taiyaki_amd_lstm_wgrad.h; libtaiyaki_amd_lstm_wgrad.so).  The plan, the kernel and the reduction are
// wgrad_common.h's, shared with gru_wgrad.hip; this file is the LSTM's cell and its entries.
#include "wgrad_common.h"

#include "../../include/taiyaki_amd_lstm_wgrad.h"

namespace tk {
namespace {

// A is dG (K x 4H) for every tile; the bias sum is db (4H)
struct LstmCell {
    static constexpr int GATES = 4;
    static constexpr bool SEAM = false;
    static constexpr int EXTRA_BIAS = 0;
    static constexpr bool VEC4_EDGE = false;    // the two instantiations it has always had
    typedef WgradArgs Args;
    typedef float *Bias;
    static bool takes(size_t) { return true; }
    static __device__ __forceinline__ void store_bias(float *db, size_t i, float v, int, int) { db[i] = v; }
};

}  // namespace

size_t lstm_wgrad_workspace_bytes(size_t T, size_t N, size_t H, size_t I, int cu_count) {
    return wgrad_workspace_bytes<LstmCell>(T, N, H, I, cu_count);
}

int lstm_wgrad_dispatch(const float *dgates, const float *x, const float *y, size_t T, size_t N, size_t H, size_t I,
                        int reverse, int cu_count, float *dw_ih, float *dw_hh, float *db, void *ws, size_t wsb,
                        hipStream_t stream) {
    if (!dgates || !x || !y || !dw_ih || !dw_hh || !db || !ws || !aligned16(ws)) return TK_ERR_BAD_ARG;
    WgradArgs a;
    a.dg = dgates, a.x = x, a.y = y;
    return wgrad_launch<LstmCell>(a, aligned16(dgates) && aligned16(x) && aligned16(y), T, N, H, I, reverse, cu_count,
                                  dw_ih, dw_hh, db, ws, wsb, stream);
}

}  // namespace tk

extern "C" {

size_t tk_lstm_weight_grad_workspace_bytes(size_t nblk, size_t nbatch, size_t size, size_t insize, int cu_count) {
    return tk::lstm_wgrad_workspace_bytes(nblk, nbatch, size, insize, cu_count);
}

int tk_lstm_weight_grad_dev(const float *dgates, const float *x, const float *y, size_t nblk, size_t nbatch,
                            size_t size, size_t insize, int reverse, int cu_count, float *dw_ih, float *dw_hh,
                            float *db, void *workspace, size_t workspace_bytes, void *stream) {
    return tk::lstm_wgrad_dispatch(dgates, x, y, nblk, nbatch, size, insize, reverse, cu_count, dw_ih, dw_hh, db,
                                   workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
void tk_lab_lstm_wgrad_splits(int splits) { tk::g_lab_splits = splits; }

int tk_lab_lstm_wgrad_plan(size_t nblk, size_t nbatch, size_t size, size_t insize, int cu_count, size_t *out) {
    return tk::wgrad_lab_plan<tk::LstmCell>(nblk, nbatch, size, insize, cu_count, out);
}

int tk_lab_lstm_wgrad_loads(size_t size, size_t insize, int aligned) {
    return tk::wgrad_loads<tk::LstmCell>(aligned != 0, size, insize);
}
#endif

}  // extern "C"

// gru_wgrad.hip -- the parameter gradients of one GRU layer as one split-K GEMM on the bf16 matrix cores, every float32
// operand split into three bf16 parts, and one reduction (include/taiyaki_amd_gru_wgrad.h;
// libtaiyaki_amd_gru_wgrad.so).  The plan, the kernel and the reduction are wgrad_common.h's, shared with
// lstm_wgrad.hip; this file is the GRU's cell and its entries.
//
//   dW_ih (3H, I) = dG^T x,  db_ih (3H) = the column sums of dG           (the x tiles; their first column of tiles)
//   dW_hh (3H, H) = [dG[:, :2H] | dq]^T y shifted,  db_hh[2H:] = the column sums of dq       (the y tiles; theirs)
//   db_hh[:2H]    = db_ih[:2H], written by the thread of the reduction that writes db_ih
#include "wgrad_common.h"

#include "../../include/taiyaki_amd_gru_wgrad.h"

namespace tk {
namespace {

struct GruWgradArgs : WgradArgs {
    const float *dq;
};

struct GruBias {
    float *ih, *hh;     // hh may be NULL
};

struct GruCell {
    static constexpr int GATES = 3;
    static constexpr bool SEAM = true;
    static constexpr int EXTRA_BIAS = 1;
    static constexpr bool VEC4_EDGE = true;     // H = 96 and 192 are no multiples of the tile
    typedef GruWgradArgs Args;
    typedef GruBias Bias;
    static bool takes(size_t H) { return H % 2 == 0; }     // the seam at 2H falls between two float4s
    // entry i of [the column sums of dG (M)] | [the column sums of dq (H)]
    static __device__ __forceinline__ void store_bias(GruBias db, size_t i, float v, int M, int H) {
        if (i < (size_t)M) {
            db.ih[i] = v;
            if (db.hh && i < (size_t)(2 * H)) db.hh[i] = v;
        } else if (db.hh) {
            db.hh[i - M + 2 * H] = v;
        }
    }
};

}  // namespace

size_t gru_wgrad_workspace_bytes(size_t T, size_t N, size_t H, size_t I, int cu_count) {
    return wgrad_workspace_bytes<GruCell>(T, N, H, I, cu_count);
}

int gru_wgrad_dispatch(const float *dgates, const float *dq, const float *x, const float *y, size_t T, size_t N,
                       size_t H, size_t I, int reverse, int cu_count, float *dw_ih, float *dw_hh, float *db_ih,
                       float *db_hh, void *ws, size_t wsb, hipStream_t stream) {
    if (!dgates || !dq || !x || !y || !dw_ih || !dw_hh || !db_ih || !ws || !aligned16(ws)) return TK_ERR_BAD_ARG;
    GruWgradArgs a;
    a.dg = dgates, a.dq = dq, a.x = x, a.y = y;
    return wgrad_launch<GruCell>(a, aligned16(dgates) && aligned16(dq) && aligned16(x) && aligned16(y), T, N, H, I,
                                 reverse, cu_count, dw_ih, dw_hh, GruBias{db_ih, db_hh}, ws, wsb, stream);
}

}  // namespace tk

extern "C" {

size_t tk_gru_weight_grad_workspace_bytes(size_t nblk, size_t nbatch, size_t size, size_t insize, int cu_count) {
    return tk::gru_wgrad_workspace_bytes(nblk, nbatch, size, insize, cu_count);
}

int tk_gru_weight_grad_dev(const float *dgates, const float *dq, const float *x, const float *y, size_t nblk,
                           size_t nbatch, size_t size, size_t insize, int reverse, int cu_count, float *dw_ih,
                           float *dw_hh, float *db_ih, float *db_hh, void *workspace, size_t workspace_bytes,
                           void *stream) {
    return tk::gru_wgrad_dispatch(dgates, dq, x, y, nblk, nbatch, size, insize, reverse, cu_count, dw_ih, dw_hh, db_ih,
                                  db_hh, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
void tk_lab_gru_wgrad_splits(int splits) { tk::g_lab_splits = splits; }

int tk_lab_gru_wgrad_plan(size_t nblk, size_t nbatch, size_t size, size_t insize, int cu_count, size_t *out) {
    return tk::wgrad_lab_plan<tk::GruCell>(nblk, nbatch, size, insize, cu_count, out);
}

int tk_lab_gru_wgrad_loads(size_t size, size_t insize, int aligned) {
    return tk::wgrad_loads<tk::GruCell>(aligned != 0, size, insize);
}
#endif

}  // extern "C"

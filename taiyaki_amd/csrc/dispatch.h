// dispatch.h -- the host entries of the kernel files (the CRF's and the squiggle match's: crf_band.h, squiggle_match.h),
// declared ONCE: included by the file that defines a function and by c_api.hip, which calls it.  A definition that
// disagrees with its declaration here does not compile, or does not link (the libraries are linked with --no-undefined).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/taiyaki_amd_basecall.h"
#include "../../include/taiyaki_amd_flipflop.h"

namespace tk {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// logz_kernels.hip, viterbi_kernels.hip
// What the logZ launcher makes of a shape: rows per chunk after the LDS fallback (8 / 16 / 32), the form of the
// transfer kernel, the middle kernel's chunks per super (8 / 16), and whether the posterior kernel keeps the hand-off
// slots of its chains in a tail behind the waves' buffers (or inside them)
enum { LOGZ_COOP = 0, LOGZ_RING = 1, LOGZ_PLAIN = 2, LOGZ_STREAM = 3 };
struct LogzPlan {
    int ch, transfer, super;
    bool chain_tail;
};
size_t logz_workspace_bytes(size_t T, size_t N, size_t nbase);
int logz_dispatch(const float *scores, size_t T, size_t N, size_t nbase, float *logz, float *grad, void *workspace,
                  size_t workspace_bytes, uint32_t *status, hipStream_t stream, float *loss_acc = nullptr,
                  float acc_scale = 0.f, float grad_scale = 1.f, const float *grad_scale_vec = nullptr);
bool logz_side_stream(hipStream_t *s, hipEvent_t *fork, hipEvent_t *join);
size_t viterbi_workspace_bytes(size_t T, size_t N, size_t nbase);
int viterbi_dispatch(const float *scores, size_t T, size_t N, size_t nbase, float *fwd, int64_t *tb, int64_t *path,
                     void *workspace, size_t workspace_bytes, hipStream_t stream);

// beam_kernels.hip
size_t beam_workspace_bytes(size_t T, size_t N, size_t nbase);
int lattice_dispatch(const float *scores, size_t T, size_t N, size_t nbase, int forward, const float *init, float *out,
                     float *total, hipStream_t stream);
int beam_dispatch(const float *scores, size_t T, size_t N, size_t nbase, int width, float beam_cut, int guided,
                  signed char *seq, int *seqlen, float *score, void *workspace, size_t workspace_bytes,
                  hipStream_t stream);

// clip_kernels.hip, qscore_kernels.hip, crf_kernels.hip
int grad_clip_dispatch(float *grads, const int64_t *seg_off, size_t nseg, size_t max_seg_len, const float *thresh,
                       float *maxs, hipStream_t stream);
int errprobs_dispatch(const float *trans, const int64_t *path, size_t T, size_t N, size_t nbase, float *out,
                      hipStream_t stream);
int build_indices_dispatch(const int32_t *seqs, const int32_t *seqlen, size_t nbatch, size_t nbase,
                           const int32_t *mod_cats, const int32_t *can_mods_offsets, const float *mod_cat_weights,
                           int64_t *seqoff, int32_t *stay, int32_t *move, int32_t *mod, float *fact, size_t total_len,
                           uint32_t *status, hipStream_t stream);

// chunk_kernels.hip
int chunks_locate_dispatch(const tk_mapped_store *st, const int32_t *cand_read, const int32_t *cand_start,
                           const double *cand_frac, size_t ncand, size_t chunk_len, const tk_chunk_filter *fp,
                           uint8_t *reason, int32_t *dacstart, int32_t *seqstart, int32_t *seqlen, int32_t *maxdwell,
                           hipStream_t stream);
int chunks_select_dispatch(const uint8_t *reason, const int32_t *seqlen, size_t ncand, size_t nwant, int32_t *sel,
                           int64_t *seqoff, int32_t *counts, hipStream_t stream);
int chunks_gather_dispatch(const tk_mapped_store *st, const int32_t *cand_read, const int32_t *dacstart,
                           const int32_t *seqstart, const int32_t *seqlen, const int32_t *sel, const int64_t *seqoff,
                           const int32_t *counts, size_t nwant, size_t chunk_len, int reverse, int standardize,
                           size_t ncan, const int32_t *can_labels, const int32_t *mod_labels, float *indata,
                           int32_t *seqs, size_t seqs_cap, int32_t *seqlens_out, int32_t *mod_cats, uint32_t *status,
                           hipStream_t stream);

// remap_kernels.hip
struct RemapArgs {
    const float *scores;        // concatenated (sum T_i, K)
    const int64_t *row_off;     // (nread + 1) row offsets
    const int32_t *stay_index;  // concatenated, M_i per read
    const int32_t *step_index;  // concatenated, M_i - 1 per read (read i starts at seq_off[i] - i)
    const int64_t *seq_off;     // (nread + 1)
    const double *localpen;     // per read
    int K;
    double *score;              // (nread)
    int64_t *path;              // concatenated, T_i + 1 per read (read i starts at row_off[i] + i)
    uint64_t *tb;               // traceback bits
    const int64_t *tb_off;      // (nread) offsets into tb, in 64-bit words
};
int remap_dispatch(const RemapArgs &a, size_t nread, size_t max_M, hipStream_t stream);
int path_to_reftosignal_dispatch(const int64_t *path, const int64_t *path_off, const int64_t *ref_off,
                                 const int64_t *signalstart, const int64_t *siglen, int stride, size_t nread,
                                 int32_t *rts, hipStream_t stream);

// lstm_kernels.hip, gru_kernels.hip
size_t lstm_workspace_bytes(size_t N, size_t H, int cu_count);
int lstm_forward_dispatch(const float *gx, const float *whh, size_t T, size_t N, size_t H, int reverse, int cu_count,
                          float *y, float *gates, float *cell, void *ws, size_t wsb, uint32_t *status,
                          hipStream_t stream);
int lstm_backward_dispatch(const float *whh, const float *gates, const float *cell, const float *dy, size_t T, size_t N,
                           size_t H, int reverse, int cu_count, float *dgates, void *ws, size_t wsb, uint32_t *status,
                           hipStream_t stream);
size_t gru_workspace_bytes(size_t N, size_t H, int cu_count);
int gru_forward_dispatch(const float *gx, const float *whh, const float *bhh, size_t T, size_t N, size_t H, int reverse,
                         int cu_count, float *y, float *gates, float *q, void *ws, size_t wsb, uint32_t *status,
                         hipStream_t stream);
int gru_backward_dispatch(const float *whh, const float *y, const float *gates, const float *q, const float *dy,
                          size_t T, size_t N, size_t H, int reverse, int cu_count, float *dgates, float *dq, void *ws,
                          size_t wsb, uint32_t *status, hipStream_t stream);

// ... and their -DTK_RNN_VARLEN build (libtaiyaki_amd_rnn_varlen.so; rnn_varlen_api.hip defines the C entries)
size_t lstm_varlen_workspace_bytes(size_t N, size_t H, int cu_count);
int lstm_forward_varlen_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N,
                                 size_t H, int reverse, int cu_count, float *y, void *ws, size_t wsb,
                                 uint32_t *status, hipStream_t stream);
size_t gru_varlen_workspace_bytes(size_t N, size_t H, int cu_count);
int gru_forward_varlen_dispatch(const float *gx, const float *whh, const float *bhh, const int32_t *lengths, size_t T,
                                size_t N, size_t H, int reverse, int cu_count, float *y, void *ws, size_t wsb,
                                uint32_t *status, hipStream_t stream);

// ... and their -DTK_RNN_VARLEN_TRAIN build (libtaiyaki_amd_rnn_varlen_train.so; rnn_varlen_train_api.hip defines the C
// entries)
size_t lstm_varlen_train_workspace_bytes(size_t N, size_t H, int cu_count);
int lstm_forward_varlen_save_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N,
                                      size_t H, int reverse, int cu_count, float *y, float *gates, float *cell,
                                      void *ws, size_t wsb, uint32_t *status, hipStream_t stream);
int lstm_backward_varlen_dispatch(const float *whh, const float *gates, const float *cell, const float *dy,
                                  const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                                  float *dgates, void *ws, size_t wsb, uint32_t *status, hipStream_t stream);
size_t gru_varlen_train_workspace_bytes(size_t N, size_t H, int cu_count);
int gru_forward_varlen_save_dispatch(const float *gx, const float *whh, const float *bhh, const int32_t *lengths,
                                     size_t T, size_t N, size_t H, int reverse, int cu_count, float *y, float *gates,
                                     float *q, void *ws, size_t wsb, uint32_t *status, hipStream_t stream);
int gru_backward_varlen_dispatch(const float *whh, const float *y, const float *gates, const float *q,
                                 const float *dy, const int32_t *lengths, size_t T, size_t N, size_t H, int reverse,
                                 int cu_count, float *dgates, float *dq, void *ws, size_t wsb, uint32_t *status,
                                 hipStream_t stream);

// ... and their -DTK_RNN_WIDE build (libtaiyaki_amd_rnn_wide.so; rnn_wide_api.hip defines the C entries): every batch
// width, as slabs of columns; gates and cell (q) of the forwards may both be NULL
size_t lstm_wide_slab(size_t N, size_t H, int cu_count);
size_t lstm_wide_workspace_bytes(size_t N, size_t H, int cu_count);
int lstm_forward_wide_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N, size_t H,
                               int reverse, int cu_count, float *y, float *gates, float *cell, void *ws, size_t wsb,
                               uint32_t *status, hipStream_t stream);
int lstm_backward_wide_dispatch(const float *whh, const float *gates, const float *cell, const float *dy,
                                const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                                float *dgates, void *ws, size_t wsb, uint32_t *status, hipStream_t stream);

// ... and lstm_kernels.hip's -DTK_LSTM_LARGE build (libtaiyaki_amd_lstm_large.so; lstm_large_api.hip defines the C
// entries): hidden size 512 at every batch width, as slabs of columns; gates and cell of the forward may both be NULL
int lstm_large_supported(size_t H);
size_t lstm_large_slab(size_t N, size_t H, int cu_count);
size_t lstm_large_workspace_bytes(size_t N, size_t H, int cu_count);
int lstm_forward_large_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N, size_t H,
                                int reverse, int cu_count, float *y, float *gates, float *cell, void *ws, size_t wsb,
                                uint32_t *status, hipStream_t stream);
int lstm_backward_large_dispatch(const float *whh, const float *gates, const float *cell, const float *dy,
                                 const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                                 float *dgates, void *ws, size_t wsb, uint32_t *status, hipStream_t stream);
size_t gru_wide_slab(size_t N, size_t H, int cu_count);
size_t gru_wide_workspace_bytes(size_t N, size_t H, int cu_count);
int gru_forward_wide_dispatch(const float *gx, const float *whh, const float *bhh, const int32_t *lengths, size_t T,
                              size_t N, size_t H, int reverse, int cu_count, float *y, float *gates, float *q, void *ws,
                              size_t wsb, uint32_t *status, hipStream_t stream);
int gru_backward_wide_dispatch(const float *whh, const float *y, const float *gates, const float *q, const float *dy,
                               const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                               float *dgates, float *dq, void *ws, size_t wsb, uint32_t *status, hipStream_t stream);

// conv_kernels.hip
bool conv_small_supported(size_t cin, size_t cout, size_t winlen, size_t stride);
size_t conv_small_workspace_bytes(size_t T, size_t N, size_t cin, size_t cout, size_t winlen, int cu_count);
int conv_small_forward_dispatch(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cin,
                                size_t cout, size_t winlen, int cu_count, float *y, hipStream_t stream);
int conv_small_backward_dispatch(const float *dy, const float *x, const float *w, const float *b, size_t T, size_t N,
                                 size_t cin, size_t cout, size_t winlen, int cu_count, float *dx, float *dw, float *db,
                                 void *ws, size_t wsb, hipStream_t stream);

// lstm_wgrad.hip (a library of its own, include/taiyaki_amd_lstm_wgrad.h: the file defines its C entries itself)
size_t lstm_wgrad_workspace_bytes(size_t T, size_t N, size_t H, size_t I, int cu_count);
int lstm_wgrad_dispatch(const float *dgates, const float *x, const float *y, size_t T, size_t N, size_t H, size_t I,
                        int reverse, int cu_count, float *dw_ih, float *dw_hh, float *db, void *ws, size_t wsb,
                        hipStream_t stream);

// lstm_local.hip (a library of its own too, include/taiyaki_amd_lstm_local.h: the file defines its C entries itself).
// One workgroup owns every unit of its columns: no workspace, no status word.  gates and cell may both be NULL
int lstm_local_supported(size_t H);
int lstm_local_columns(size_t N, size_t H, int cu_count);
int lstm_local_forward_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N, size_t H,
                                int reverse, int cu_count, float *y, float *gates, float *cell, hipStream_t stream);
int lstm_local_backward_dispatch(const float *whh, const float *gates, const float *cell, const float *dy,
                                 const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                                 float *dgates, hipStream_t stream);

// gru_wgrad.hip (a library of its own too, include/taiyaki_amd_gru_wgrad.h; db_hh may be NULL)
size_t gru_wgrad_workspace_bytes(size_t T, size_t N, size_t H, size_t I, int cu_count);
int gru_wgrad_dispatch(const float *dgates, const float *dq, const float *x, const float *y, size_t T, size_t N,
                       size_t H, size_t I, int reverse, int cu_count, float *dw_ih, float *dw_hh, float *db_ih,
                       float *db_hh, void *ws, size_t wsb, hipStream_t stream);

// rnn_proj.hip (a library of its own too, include/taiyaki_amd_rnn_proj.h): out (rows, nout) = a (rows, k) B^T + bias, B
// (nout, k) = w, or for transposed != 0 the transpose of w (k, nout); bias may be NULL
size_t rnn_proj_workspace_bytes(size_t rows, size_t k, size_t nout, int cu_count);
int rnn_proj_dispatch(const float *a, const float *w, const float *bias, int transposed, size_t rows, size_t k,
                      size_t nout, int cu_count, float *out, void *ws, size_t wsb, hipStream_t stream);

// basecall_mods.hip (libtaiyaki_amd_basecall.so; basecall_kernels.hip defines the C entry and fills the column map)
struct ModColumns {
    uint8_t base[TK_BASECALL_MAX_NMOD];     // the canonical base that output column j belongs to
    uint8_t src[TK_BASECALL_MAX_NMOD];      // ... and its column in a weight row: off_b + 1 + m
};
int mod_weights_dispatch(const int64_t *path, const float *mod_weights, size_t nblk, size_t nchunks, size_t ncat,
                         const int64_t *chunk_starts, const int64_t *chunk_ends, const int64_t *read_chunk_off,
                         const float *read_scale, size_t nread, size_t stride, size_t nbase, size_t nmod,
                         const ModColumns &cols, const int64_t *out_off, float *mods, int32_t *seqlen,
                         uint32_t *status, hipStream_t stream);

// crf_kernels.hip and crf_band.hip built -DTK_LOSS_VARLEN (libtaiyaki_amd_loss_varlen.so; loss_varlen_api.hip defines the C
// entries): crf_dispatch takes CrfCall::lengths (crf_band.h), and the lab build's plan query is that library's own
#ifdef TK_LOSS_VARLEN
bool crf_lab_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, int form, int want_grad,
                  float sharp, size_t workspace_bytes, size_t *out);
#endif

#ifdef TK_LAB
// what the lab hooks below set (crf_band.hip, lstm_kernels.hip, gru_kernels.hip)
void crf_band_lab_phase(int phase);
void lstm_lab_cols(int cols);
void lstm_lab_units(int units);
bool lstm_lab_geometry(size_t N, size_t H, int cu_count, size_t *out);
void gru_lab_cols(int cols);
void lstm_local_lab_cols(int cols);
void lstm_large_lab_cols(int cols);
bool lstm_large_lab_geometry(size_t N, size_t H, int cu_count, size_t *out);
bool logz_lab_plan(size_t T, size_t N, size_t nbase, size_t score_bytes, LogzPlan *p);
int viterbi_lab_waves(size_t N);
bool crf_lab_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, int form, int want_grad,
                  float sharp, size_t workspace_bytes, size_t *out);
#endif

}  // namespace tk

// The lab hooks: exported by the lab build only (c_api.hip defines them), kept out of the public header.  The block
// below is also what taiyaki_amd/_lib.py reads LAB_SIGNATURES from: plain C declarators, as in the public header.
#ifdef TK_LAB
extern "C" {
/* kernel A's phases on their own, for timing (crf_band.hip) */
void tk_lab_crf_band_phase(int phase);
/* the LSTM recurrence's batch columns per workgroup, 8 or 16 (0: the launcher's rule; lstm_kernels.hip) */
void tk_lab_lstm_cols(int cols);
/* the LSTM recurrence's hidden units per workgroup, 16, 32 or 64 (0: the launcher's rule) */
void tk_lab_lstm_units(int units);
/* the LSTM recurrence's launch plan at (nbatch, size, cu_count): out[8] = admitted C and groups, U, C, groups,
 * grid, forward and backward granule bytes; 0 where the kernels do not run */
int tk_lab_lstm_geometry(size_t nbatch, size_t size, int cu_count, size_t *out);
/* the GRU recurrence's batch columns per workgroup at sizes <= 128: 1 or 2 (0: the launcher's rule; gru_kernels.hip) */
void tk_lab_gru_cols(int cols);
/* the logZ launch plan at (nblk, nbatch, nbase) for a score tensor of score_bytes: out[4] = rows per chunk after the
 * LDS fallback, the transfer form (0 cooperative, 1 LDS ring, 2 one wave per chunk through registers, 3 its
 * streaming-load instantiation), chunks per super, 1 where the posterior kernel keeps its chains in the tail;
 * 0 where the launch refuses the shape (logz_kernels.hip) */
int tk_lab_logz_plan(size_t nblk, size_t nbatch, size_t nbase, size_t score_bytes, size_t *out);
/* the Viterbi's waves per read at nbatch reads: 5, 3 or 1 (viterbi_kernels.hip) */
int tk_lab_viterbi_plan(size_t nbatch);
/* kernel A's choices for a call under the environment as it stands (crf_kernels.hip: crf_choose; form 0 the plain CRF,
 * 1 cat-mod with per-column factors, 2 cat-mod with per-position factors; max_seqlen 0: nblk + 1; bulk_seqlen 0: unknown):
 * out[20] = 0 the linear path / 1 the log-domain kernel on every read; the log-domain form's R, W and checkpoint spacing
 * (behind the linear path: the tail launch's); the batch launch's R, W, block length, 2 x weight bias, frame slope, 1 with
 * a row maker, wave-count class; the retry's block length (0: none), 2 x bias, slope, R, W, 1 where its sweeps run side by
 * side; the tail's log-domain R; the slots; the tail launch's R.  0 where the call is refused */
int tk_lab_crf_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, int form,
                    int want_grad, float sharp, size_t workspace_bytes, size_t *out);
}
#endif

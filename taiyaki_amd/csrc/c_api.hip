// c_api.hip -- the extern "C" boundary declared in include/taiyaki_amd_flipflop.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/taiyaki_amd_flipflop.h"
#include "crf_band.h"
#include "dispatch.h"
#include "squiggle_match.h"

extern "C" {

const char *tk_version(void) { return "taiyaki_amd flipflop gfx950 r3"; }

int tk_flipflop_build_indices_dev(const int32_t *seqs, const int32_t *seqlen, size_t nbatch,
                                  size_t total_len, size_t nbase, const int32_t *mod_cats,
                                  const int32_t *can_mods_offsets,
                                  const float *mod_cat_weights, int64_t *seqoff,
                                  int32_t *stayidx, int32_t *moveidx, int32_t *modidx,
                                  float *modfact, uint32_t *status, void *stream) {
    if (!seqlen || !seqoff || !stayidx || !moveidx || nbatch == 0 || nbase == 0) return TK_ERR_BAD_ARG;
    if (total_len > 0 && !seqs) return TK_ERR_BAD_ARG;
    if (mod_cats && (!can_mods_offsets || !mod_cat_weights || !modidx || !modfact)) return TK_ERR_BAD_ARG;
    return tk::build_indices_dispatch(seqs, seqlen, nbatch, nbase, mod_cats, can_mods_offsets,
                                      mod_cat_weights, seqoff, stayidx, moveidx, modidx,
                                      modfact, total_len, status, static_cast<hipStream_t>(stream));
}

int tk_grad_maxabs_clip_dev(float *grads, const int64_t *seg_off, size_t nseg, size_t max_seg_len,
                            const float *thresh, float *maxs, void *stream) {
    if (!grads || !seg_off || !maxs) return TK_ERR_BAD_ARG;
    return tk::grad_clip_dispatch(grads, seg_off, nseg, max_seg_len, thresh, maxs, static_cast<hipStream_t>(stream));
}

int tk_flipflop_remap_dev(const float *scores, const int64_t *row_off, size_t ntrans,
                          const int32_t *stay_index, const int32_t *step_index, const int64_t *seq_off,
                          const double *localpen, size_t nread, size_t max_seqlen, double *score,
                          int64_t *path, uint64_t *traceback, const int64_t *tb_off, void *stream) {
    if (!row_off || !stay_index || !seq_off || !localpen || !score || !path || !tb_off || ntrans == 0)
        return TK_ERR_BAD_ARG;
    if (nread == 0) return TK_OK;
    if (max_seqlen > 1 && !step_index) return TK_ERR_BAD_ARG;
    if (nread > (size_t)INT32_MAX || ntrans > 4096) return TK_ERR_UNSUPPORTED;
    tk::RemapArgs a{scores, row_off, stay_index, step_index, seq_off, localpen, (int)ntrans, score, path,
                    traceback, tb_off};
    return tk::remap_dispatch(a, nread, max_seqlen, static_cast<hipStream_t>(stream));
}

int tk_remap_path_to_ref_to_signal_dev(const int64_t *path, const int64_t *path_off, const int64_t *ref_off,
                                       const int64_t *signalstart, const int64_t *siglen, size_t stride,
                                       size_t nread, int32_t *ref_to_signal, void *stream) {
    if (!path || !path_off || !ref_off || !signalstart || !siglen || !ref_to_signal || stride == 0)
        return TK_ERR_BAD_ARG;
    if (nread == 0) return TK_OK;
    if (nread > (size_t)INT32_MAX || stride > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    return tk::path_to_reftosignal_dispatch(path, path_off, ref_off, signalstart, siglen, (int)stride, nread,
                                            ref_to_signal, static_cast<hipStream_t>(stream));
}

// squiggle match: the checks every entry shares (lengths themselves are checked on the device)
static int sq_args(tk::SqArgs &a, const float *params, const float *signal, const int32_t *siglen,
                   const int64_t *sig_off, size_t npos, size_t nbatch, size_t nsignal, float back_prob,
                   uint32_t *status) {
    if (!params || !signal || !siglen || !sig_off || npos == 0 || nbatch == 0) return TK_ERR_BAD_ARG;
    if (tk::sq_positions_per_lane(npos) == 0 || nbatch > (size_t)INT32_MAX || nsignal > (size_t)INT64_MAX / 2)
        return TK_ERR_UNSUPPORTED;
    a = tk::SqArgs{};
    a.params = params;
    a.signal = signal;
    a.siglen = siglen;
    a.sig_off = sig_off;
    a.nbatch = (int)nbatch;
    a.npos = (int)npos;
    a.nsignal = (int64_t)nsignal;
    a.prob_back = back_prob;
    a.status = status;
    return TK_OK;
}

size_t tk_squiggle_match_workspace_bytes(int op, size_t npos, size_t nbatch, size_t nsignal) {
    if (op == 1) return tk::sq_lattice_bytes(npos, nbatch, nsignal);
    if (op == 2) return tk::sq_path_bytes(npos, nsignal);
    return 0;
}

int tk_squiggle_match_cost_dev(const float *params, const float *signal, const int32_t *siglen,
                               const int64_t *sig_off, size_t npos, size_t nbatch, size_t nsignal,
                               float back_prob, float *cost, void *workspace, size_t workspace_bytes,
                               uint32_t *status, void *stream) {
    tk::SqArgs a;
    int rc = sq_args(a, params, signal, siglen, sig_off, npos, nbatch, nsignal, back_prob, status);
    if (rc != TK_OK) return rc;
    if (!cost) return TK_ERR_BAD_ARG;
    a.cost = cost;
    if (workspace) {
        if (workspace_bytes < tk::sq_lattice_bytes(npos, nbatch, nsignal)) return TK_ERR_WORKSPACE;
        a.lattice = static_cast<float *>(workspace);
    }
    return tk::squiggle_dispatch(workspace ? 1 : 0, a, static_cast<hipStream_t>(stream));
}

int tk_squiggle_match_grad_dev(const float *params, const float *signal, const int32_t *siglen,
                               const int64_t *sig_off, size_t npos, size_t nbatch, size_t nsignal,
                               float back_prob, int have_forward, float *cost, float *grad, void *workspace,
                               size_t workspace_bytes, uint32_t *status, void *stream) {
    tk::SqArgs a;
    int rc = sq_args(a, params, signal, siglen, sig_off, npos, nbatch, nsignal, back_prob, status);
    if (rc != TK_OK) return rc;
    if (!grad || !workspace) return TK_ERR_BAD_ARG;
    if (workspace_bytes < tk::sq_lattice_bytes(npos, nbatch, nsignal)) return TK_ERR_WORKSPACE;
    a.cost = cost;
    a.grad = grad;
    a.lattice = static_cast<float *>(workspace);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (!have_forward && (rc = tk::squiggle_dispatch(1, a, s)) != TK_OK) return rc;
    return tk::squiggle_dispatch(2, a, s);
}

int tk_squiggle_match_path_dev(const float *params, const float *signal, const int32_t *siglen,
                               const int64_t *sig_off, size_t npos, size_t nbatch, size_t nsignal,
                               float back_prob, float localpen, float minscore, float *cost, int32_t *path,
                               void *workspace, size_t workspace_bytes, uint32_t *status, void *stream) {
    tk::SqArgs a;
    int rc = sq_args(a, params, signal, siglen, sig_off, npos, nbatch, nsignal, back_prob, status);
    if (rc != TK_OK) return rc;
    if (!cost || !path || !workspace) return TK_ERR_BAD_ARG;
    if (workspace_bytes < tk::sq_path_bytes(npos, nsignal)) return TK_ERR_WORKSPACE;
    a.localpen = localpen;
    a.minscore = minscore;
    a.cost = cost;
    a.path = path;
    a.tb = static_cast<uint8_t *>(workspace);
    a.endtb = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(workspace) +
                                          nsignal * 64 * (size_t)tk::sq_positions_per_lane(npos));
    return tk::squiggle_dispatch(3, a, static_cast<hipStream_t>(stream));
}

static bool store_ok(const tk_mapped_store *s) {
    return s && s->dacs && s->dacs_off && s->ref_to_signal && s->rts_off && s->reference && s->scaling &&
           s->mapped && s->nreads > 0;
}

int tk_chunks_locate_dev(const tk_mapped_store *store, const int32_t *cand_read, const int32_t *cand_start,
                         const double *cand_frac, size_t ncand, size_t chunk_len,
                         const tk_chunk_filter *filter, uint8_t *reason, int32_t *dacstart,
                         int32_t *seqstart, int32_t *seqlen, int32_t *maxdwell, void *stream) {
    if (!store_ok(store) || !filter || !cand_read || (!cand_start && !cand_frac) || !reason || !dacstart ||
        !seqstart || !seqlen || !maxdwell)
        return TK_ERR_BAD_ARG;
    if (ncand == 0) return TK_OK;
    if (ncand > (size_t)INT32_MAX || chunk_len > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    return tk::chunks_locate_dispatch(store, cand_read, cand_start, cand_frac, ncand, chunk_len, filter, reason,
                                      dacstart, seqstart, seqlen, maxdwell, static_cast<hipStream_t>(stream));
}

int tk_chunks_select_dev(const uint8_t *reason, const int32_t *seqlen, size_t ncand, size_t nwant,
                         int32_t *sel, int64_t *seqoff, int32_t *counts, void *stream) {
    if (!seqoff || !counts || (nwant > 0 && !sel) || (ncand > 0 && (!reason || !seqlen))) return TK_ERR_BAD_ARG;
    if (ncand > (size_t)INT32_MAX || nwant > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    return tk::chunks_select_dispatch(reason, seqlen, ncand, nwant, sel, seqoff, counts,
                                      static_cast<hipStream_t>(stream));
}

int tk_chunks_gather_dev(const tk_mapped_store *store, const int32_t *cand_read, const int32_t *dacstart,
                         const int32_t *seqstart, const int32_t *seqlen, const int32_t *sel,
                         const int64_t *seqoff, const int32_t *counts, size_t nwant, size_t chunk_len,
                         int reverse, int standardize, size_t ncan, const int32_t *can_labels,
                         const int32_t *mod_labels, float *indata, int32_t *seqs, size_t seqs_cap,
                         int32_t *seqlens, int32_t *mod_cats, uint32_t *status, void *stream) {
    if (!store_ok(store) || !cand_read || !dacstart || !seqstart || !seqlen || !sel || !seqoff || !counts ||
        !indata || !seqs || !seqlens || ncan == 0)
        return TK_ERR_BAD_ARG;
    if ((can_labels == nullptr) != (mod_labels == nullptr) || (mod_cats && !mod_labels)) return TK_ERR_BAD_ARG;
    if (nwant == 0 || chunk_len == 0) return TK_OK;
    if (nwant > 65535u * 16u || chunk_len > (size_t)INT32_MAX) return TK_ERR_UNSUPPORTED;
    return tk::chunks_gather_dispatch(store, cand_read, dacstart, seqstart, seqlen, sel, seqoff, counts, nwant,
                                      chunk_len, reverse, standardize, ncan, can_labels, mod_labels, indata,
                                      seqs, seqs_cap, seqlens, mod_cats, status,
                                      static_cast<hipStream_t>(stream));
}

int tk_flipflop_errprobs_dev(const float *trans, const int64_t *path, size_t nblk, size_t nbatch,
                             size_t nbase, float *errprobs, void *stream) {
    if (!trans || !path || !errprobs || nblk == 0 || nbatch == 0) return TK_ERR_BAD_ARG;
    if (!tk::aligned16(trans)) return TK_ERR_BAD_ARG;
    return tk::errprobs_dispatch(trans, path, nblk, nbatch, nbase, errprobs, static_cast<hipStream_t>(stream));
}

size_t tk_crf_flipflop_workspace_bytes(size_t ntrans, size_t nblk, size_t nbatch,
                                       size_t max_seqlen, int want_grad) {
    return tk::crf_workspace_bytes_sharp(ntrans, nblk, nbatch, max_seqlen, want_grad, 1.0f);
}

size_t tk_crf_flipflop_workspace_bytes_sharp(size_t ntrans, size_t nblk, size_t nbatch,
                                             size_t max_seqlen, int want_grad, float sharpfact) {
    return tk::crf_workspace_bytes_sharp(ntrans, nblk, nbatch, max_seqlen, want_grad, sharpfact);
}

static bool labels_ok(const tk_seq_labels *labels, const int32_t *modidx, tk::SeqLabels *out) {
    if (labels == nullptr || labels->nbase == 0 || (labels->seqs == nullptr && labels->total_len != 0)) return false;
    if ((labels->mod_cats != nullptr) != (modidx != nullptr)) return false;
    *out = tk::SeqLabels{labels->seqs, labels->total_len, labels->nbase, labels->mod_cats, labels->can_mods_offsets,
                         labels->mod_cat_weights, labels->bulk_seqlen};
    return true;
}

static int crf_flipflop_impl(const float *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                             const int32_t *stayidx, const int32_t *moveidx, const int32_t *modidx,
                             const float *modfact, const int32_t *seqlen, const int64_t *seqoff,
                             size_t max_seqlen, size_t ncan, float sharp_can, float sharp_mod,
                             float out_scale, float *cost, float *grad, void *workspace,
                             size_t workspace_bytes, uint32_t *status, void *stream, const float *mod_col_weights,
                             const tk::SeqLabels *labels) {
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
    c.labels = labels;
    c.sharp_can = sharp_can;
    c.sharp_mod = sharp_mod;
    c.out_scale = out_scale;
    c.cost = cost;
    c.grad = grad;
    c.workspace = workspace;
    c.workspace_bytes = workspace_bytes;
    c.status = status;
    c.stream = static_cast<hipStream_t>(stream);
    c.mod_col_weights = modidx != nullptr ? mod_col_weights : nullptr;
    return tk::crf_dispatch(c);
}

int tk_crf_flipflop_dev(const float *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                        const int32_t *stayidx, const int32_t *moveidx, const int32_t *modidx,
                        const float *modfact, const int32_t *seqlen, const int64_t *seqoff,
                        size_t max_seqlen, size_t ncan, float sharp_can, float sharp_mod,
                        float out_scale, float *cost, float *grad, void *workspace,
                        size_t workspace_bytes, uint32_t *status, void *stream, const float *mod_col_weights) {
    return crf_flipflop_impl(logprob, ntrans, nblk, nbatch, stayidx, moveidx, modidx, modfact, seqlen, seqoff, max_seqlen,
                             ncan, sharp_can, sharp_mod, out_scale, cost, grad, workspace, workspace_bytes, status, stream,
                             mod_col_weights, nullptr);
}

int tk_crf_flipflop_labels_dev(const float *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                               const tk_seq_labels *labels, const int32_t *seqlen,
                               int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                               size_t max_seqlen, size_t ncan, float sharp_can, float sharp_mod,
                               float out_scale, float *cost, float *grad, void *workspace,
                               size_t workspace_bytes, uint32_t *status, void *stream) {
    tk::SeqLabels lab;
    if (!labels_ok(labels, modidx, &lab)) return TK_ERR_BAD_ARG;
    // (modfact is filled from mod_cat_weights by column: the per-column form of the cat-mod kernels applies)
    return crf_flipflop_impl(logprob, ntrans, nblk, nbatch, stayidx, moveidx, modidx, modfact, seqlen, seqoff, max_seqlen,
                             ncan, sharp_can, sharp_mod, out_scale, cost, grad, workspace, workspace_bytes, status, stream,
                             labels->mod_cat_weights, &lab);
}

// rows of S floats -> their first S0 columns, contiguous (the canonical block of a cat-mod tensor)
__global__ void slice_cols_kernel(const float *__restrict__ src, float *__restrict__ dst, size_t nrows, int S, int S0) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows * (size_t)S0) return;
    const size_t r = i / (size_t)S0;
    dst[i] = src[r * (size_t)S + (i - r * (size_t)S0)];
}

// Kernel B beside kernel A's sweeps.  The sweeps are one workgroup per CU issuing one instruction every ~5
// cycles: they leave the chip's memory system and most of its issue slots idle, and kernel B's three launches
// (~30 us at the train step's shape) do not depend on them.  With an aux buffer for kernel B's gradient, B runs
// on a second hardware queue (the side stream of logz_kernels.hip) while the sweeps run, and kernel A's
// gradient pass, which waits for it, folds logZ / nblk and (d logZ) / nblk into the rows it writes anyway.
// Measured (round 4, LABNOTES R4.6, profiles/r4_overlap_timeline.txt): the sweeps do not slow down (57.4 ->
// 58.7 us), the fork and the join cost ~7 + ~6 us of queue idle, the fold 3 us in A's gradient pass: loss path
// 136 -> 127-129 us (plain), 180 -> 157 us (cat-mod), 226 -> 210 us (T=1600).  Mode 1 (the default; TK_LOSS_OVERLAP=0
// or tk_flipflop_loss_overlap(0) turn it off): on unless the caller's stream is CAPTURING -- a captured
// train step replays the one-queue form: a captured fork / join replays correctly but 150 us SLOWER than the
// one-queue graph (384 against 234 us for the operator with its index preparation, tools/overlap_capture_probe.py,
// profiles/r4_overlap_capture_probe.txt; mode 2 keeps that experiment reachable).
static std::atomic<int> &loss_overlap_mode() {
    static std::atomic<int> mode([] {
        const char *e = getenv("TK_LOSS_OVERLAP");      // (the one variable the release build reads: once, here)
        return (e != nullptr && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1;
    }());
    return mode;
}
int tk_flipflop_loss_overlap(int mode) {
    std::atomic<int> &m = loss_overlap_mode();
    return (mode >= 0 && mode <= 2) ? m.exchange(mode) : m.load();
}
static bool loss_overlap_enabled(hipStream_t st) {
    const int mode = loss_overlap_mode().load();
    if (mode == 0) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (mode == 1 && st != nullptr && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return false;
    return true;
}
// (the side queue and its two events are one per device: calls from several host threads take turns enqueueing)
static std::mutex loss_overlap_mu;

size_t tk_flipflop_loss_fused_aux_bytes(size_t nblk, size_t nbatch, size_t nbase, size_t ntrans) {
    const size_t ncan = 2 * nbase * (nbase + 1);
    const size_t one = (nblk * nbatch * ncan * sizeof(float) + 255) / 256 * 256;
    if (ntrans <= ncan) return loss_overlap_enabled(nullptr) ? one : 0;    // plain CRF: in place (the experiment: kernel B's gradient)
    return 2 * one;                                             // canonical scores + their logZ gradient
}

static int loss_fused_impl(const float *scores, size_t nblk, size_t nbatch, size_t nbase, size_t ntrans,
                           const int32_t *stayidx, const int32_t *moveidx, const int32_t *modidx,
                           const float *modfact, const int32_t *seqlen,
                           const int64_t *seqoff, size_t max_seqlen, float sharpfact, float grad_scale,
                           const float *grad_scale_per_read, float *lossvector,
                           float *grad, float *logz, void *crf_workspace, size_t crf_workspace_bytes,
                           void *logz_workspace, size_t logz_workspace_bytes, void *aux, size_t aux_bytes,
                           uint32_t *status, void *stream, const float *mod_col_weights, const tk::SeqLabels *labels) {
    if (!scores || !stayidx || !moveidx || !seqlen || !seqoff || !lossvector || !grad || !logz || !crf_workspace ||
        !logz_workspace || nblk == 0 || nbatch == 0 || nbase == 0 || !(sharpfact > 0.f))
        return TK_ERR_BAD_ARG;
    if (!tk::aligned16(scores) || !tk::aligned16(grad)) return TK_ERR_BAD_ARG;
    if ((modidx == nullptr) != (modfact == nullptr)) return TK_ERR_BAD_ARG;
    const size_t ncan = 2 * nbase * (nbase + 1);
    const size_t one = (nblk * nbatch * ncan * sizeof(float) + 255) / 256 * 256;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool catmod = modidx != nullptr;
    if (!catmod && ntrans != ncan) return TK_ERR_BAD_ARG;
    if (catmod && (ntrans <= ncan || ntrans > 62)) return TK_ERR_BAD_ARG;
    if (catmod && (aux == nullptr || aux_bytes < 2 * one)) return TK_ERR_WORKSPACE;
    // ctc.pyx:258-303: only the canonical columns are sharpened; cost / sharp
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
    c.labels = labels;
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
    c.mod_col_weights = catmod ? mod_col_weights : nullptr;

    if (!catmod && (aux == nullptr || aux_bytes < one || !loss_overlap_enabled(st))) {
        // (A) first: per-read costs into `lossvector`, its gradient into `grad`; (B) then ADDS
        // logZ / nblk and (d logZ / d scores) / nblk in place -- in its posterior kernel, whose stores
        // are whole coalesced row sets
        int rc = tk::crf_dispatch(c);
        if (rc != 0) return rc;
        return tk::logz_dispatch(scores, nblk, nbatch, nbase, logz, grad, logz_workspace, logz_workspace_bytes, status,
                                 st, lossvector, 1.0f / (float)nblk, grad_scale, grad_scale_per_read);
    }
    // (B) into a compact gradient of its own -- for cat-mod (bin/train_flipflop.py:165-176) on a compact
    // copy of the canonical columns, which are not contiguous in the (T, N, ntrans) tensor --, (A) folds
    // logZ / nblk into its costs and (d logZ) / nblk, times the gradient multiplier, into the canonical
    // columns of the rows it writes anyway: one gradient tensor, no elementwise pass outside these kernels.
    float *x40 = catmod ? static_cast<float *>(aux) : nullptr;
    float *g40 = reinterpret_cast<float *>(static_cast<char *>(aux) + (catmod ? one : 0));
    hipStream_t sb = st;
    hipEvent_t fork = nullptr, join = nullptr;
    const bool side = loss_overlap_enabled(st) && tk::logz_side_stream(&sb, &fork, &join);
    std::unique_lock<std::mutex> turn(loss_overlap_mu, std::defer_lock);
    if (side) turn.lock();
    if (side) {
        if (hipEventRecord(fork, st) != hipSuccess || hipStreamWaitEvent(sb, fork, 0) != hipSuccess) return TK_ERR_LAUNCH;
    } else {
        sb = st;
    }
    if (catmod) {
        const size_t n = nblk * nbatch * ncan;
        hipLaunchKernelGGL(slice_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sb, scores, x40,
                           nblk * nbatch, (int)ntrans, (int)ncan);
        if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    }
    int rc = tk::logz_dispatch(catmod ? x40 : scores, nblk, nbatch, nbase, logz, g40, logz_workspace, logz_workspace_bytes,
                               status, sb);
    if (side && hipEventRecord(join, sb) != hipSuccess) rc = rc != 0 ? rc : TK_ERR_LAUNCH;
    if (rc != 0) {
        if (side) (void)hipStreamWaitEvent(st, join, 0);        // (never leave the side queue dangling in a capture)
        return rc;
    }
    c.add_grad = g40;
    c.add_cost = logz;
    c.add_S = (int)ncan;
    c.add_scale = 1.0f / (float)nblk;
    c.add_ready = side ? join : nullptr;
    rc = tk::crf_dispatch(c);
    if (rc != 0 && side) (void)hipStreamWaitEvent(st, join, 0);
    return rc;
}

int tk_flipflop_loss_fused_dev(const float *scores, size_t nblk, size_t nbatch, size_t nbase, size_t ntrans,
                               const int32_t *stayidx, const int32_t *moveidx, const int32_t *modidx,
                               const float *modfact, const int32_t *seqlen,
                               const int64_t *seqoff, size_t max_seqlen, float sharpfact, float grad_scale,
                               const float *grad_scale_per_read, float *lossvector,
                               float *grad, float *logz, void *crf_workspace, size_t crf_workspace_bytes,
                               void *logz_workspace, size_t logz_workspace_bytes, void *aux, size_t aux_bytes,
                               uint32_t *status, void *stream, const float *mod_col_weights) {
    return loss_fused_impl(scores, nblk, nbatch, nbase, ntrans, stayidx, moveidx, modidx, modfact, seqlen, seqoff, max_seqlen,
                           sharpfact, grad_scale, grad_scale_per_read, lossvector, grad, logz, crf_workspace,
                           crf_workspace_bytes, logz_workspace, logz_workspace_bytes, aux, aux_bytes, status, stream,
                           mod_col_weights, nullptr);
}

int tk_flipflop_loss_fused_labels_dev(const float *scores, size_t nblk, size_t nbatch, size_t ntrans,
                                      const tk_seq_labels *labels, const int32_t *seqlen,
                                      int64_t *seqoff, int32_t *stayidx, int32_t *moveidx, int32_t *modidx, float *modfact,
                                      size_t max_seqlen, float sharpfact, float grad_scale,
                                      const float *grad_scale_per_read, float *lossvector,
                                      float *grad, float *logz, void *crf_workspace, size_t crf_workspace_bytes,
                                      void *logz_workspace, size_t logz_workspace_bytes, void *aux, size_t aux_bytes,
                                      uint32_t *status, void *stream) {
    tk::SeqLabels lab;
    if (!labels_ok(labels, modidx, &lab)) return TK_ERR_BAD_ARG;
    return loss_fused_impl(scores, nblk, nbatch, labels->nbase, ntrans, stayidx, moveidx, modidx, modfact, seqlen, seqoff,
                           max_seqlen, sharpfact, grad_scale, grad_scale_per_read, lossvector, grad, logz, crf_workspace,
                           crf_workspace_bytes, logz_workspace, logz_workspace_bytes, aux, aux_bytes, status, stream,
                           labels->mod_cat_weights, &lab);
}

typedef float tk_f4 __attribute__((ext_vector_type(4)));
// Measurement helper ("report the fraction against a measured device-copy ceiling"): a plain float4
// streaming copy, four independent 16-byte loads in flight per lane, one workgroup per 16 KiB -- the form the
// MI355X guide measured at 6.29 TB/s.  bench.py times it on the score tensor beside the logZ op.
__global__ __launch_bounds__(256) void devcopy_f4_kernel(const tk_f4 *__restrict__ src, tk_f4 *__restrict__ dst, size_t n4) {
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    tk_f4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (base + (size_t)k * 256 < n4) v[k] = __builtin_nontemporal_load(src + base + (size_t)k * 256);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (base + (size_t)k * 256 < n4) __builtin_nontemporal_store(v[k], dst + base + (size_t)k * 256);
}
int tk_devcopy_f32_dev(float *dst, const float *src, size_t n, void *stream) {
    if (dst == nullptr || src == nullptr || n % 4 != 0 || !tk::aligned16(dst) || !tk::aligned16(src)) return TK_ERR_BAD_ARG;
    if (n == 0) return TK_OK;
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(devcopy_f4_kernel, dim3((unsigned)((n4 + 1023) / 1024)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const tk_f4 *>(src), reinterpret_cast<tk_f4 *>(dst), n4);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

#ifdef TK_LAB
// the lab hooks (lab build only; declared in dispatch.h, not in the public header)
void tk_lab_crf_band_phase(int phase) { tk::crf_band_lab_phase(phase); }
void tk_lab_lstm_cols(int cols) { tk::lstm_lab_cols(cols); }
void tk_lab_lstm_units(int units) { tk::lstm_lab_units(units); }
int tk_lab_lstm_geometry(size_t nbatch, size_t size, int cu_count, size_t *out) {
    return tk::lstm_lab_geometry(nbatch, size, cu_count, out) ? 1 : 0;
}
void tk_lab_gru_cols(int cols) { tk::gru_lab_cols(cols); }
int tk_lab_logz_plan(size_t nblk, size_t nbatch, size_t nbase, size_t score_bytes, size_t *out) {
    tk::LogzPlan p;
    if (!tk::logz_lab_plan(nblk, nbatch, nbase, score_bytes, &p)) return 0;
    const size_t v[4] = {(size_t)p.ch, (size_t)p.transfer, (size_t)p.super, p.chain_tail ? (size_t)1 : (size_t)0};
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    return 1;
}
int tk_lab_viterbi_plan(size_t nbatch) { return tk::viterbi_lab_waves(nbatch); }
int tk_lab_crf_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, int form,
                    int want_grad, float sharp, size_t workspace_bytes, size_t *out) {
    return tk::crf_lab_plan(ntrans, nblk, nbatch, max_seqlen, bulk_seqlen, form, want_grad, sharp, workspace_bytes, out) ? 1 : 0;
}
#endif

size_t tk_lstm_workspace_bytes(size_t nbatch, size_t size, int cu_count) {
    return tk::lstm_workspace_bytes(nbatch, size, cu_count);
}

int tk_lstm_forward_dev(const float *gx, const float *w_hh, size_t nblk, size_t nbatch, size_t size, int reverse,
                        int cu_count, float *y, float *gates, float *cell, void *workspace, size_t workspace_bytes,
                        uint32_t *status, void *stream) {
    return tk::lstm_forward_dispatch(gx, w_hh, nblk, nbatch, size, reverse, cu_count, y, gates, cell, workspace,
                                     workspace_bytes, status, static_cast<hipStream_t>(stream));
}

int tk_lstm_backward_dev(const float *w_hh, const float *gates, const float *cell, const float *dy, size_t nblk,
                         size_t nbatch, size_t size, int reverse, int cu_count, float *dgates, void *workspace,
                         size_t workspace_bytes, uint32_t *status, void *stream) {
    return tk::lstm_backward_dispatch(w_hh, gates, cell, dy, nblk, nbatch, size, reverse, cu_count, dgates,
                                      workspace, workspace_bytes, status, static_cast<hipStream_t>(stream));
}

size_t tk_gru_workspace_bytes(size_t nbatch, size_t size, int cu_count) {
    return tk::gru_workspace_bytes(nbatch, size, cu_count);
}

int tk_gru_forward_dev(const float *gx, const float *w_hh, const float *b_hh, size_t nblk, size_t nbatch, size_t size,
                       int reverse, int cu_count, float *y, float *gates, float *q, void *workspace,
                       size_t workspace_bytes, uint32_t *status, void *stream) {
    return tk::gru_forward_dispatch(gx, w_hh, b_hh, nblk, nbatch, size, reverse, cu_count, y, gates, q, workspace,
                                    workspace_bytes, status, static_cast<hipStream_t>(stream));
}

int tk_gru_backward_dev(const float *w_hh, const float *y, const float *gates, const float *q, const float *dy,
                        size_t nblk, size_t nbatch, size_t size, int reverse, int cu_count, float *dgates, float *dq,
                        void *workspace, size_t workspace_bytes, uint32_t *status, void *stream) {
    return tk::gru_backward_dispatch(w_hh, y, gates, q, dy, nblk, nbatch, size, reverse, cu_count, dgates, dq,
                                     workspace, workspace_bytes, status, static_cast<hipStream_t>(stream));
}

int tk_conv1d_small_supported(size_t insize, size_t size, size_t winlen, size_t stride) {
    return tk::conv_small_supported(insize, size, winlen, stride) ? 1 : 0;
}

size_t tk_conv1d_small_workspace_bytes(size_t nblk, size_t nbatch, size_t insize, size_t size, size_t winlen,
                                       int cu_count) {
    return tk::conv_small_workspace_bytes(nblk, nbatch, insize, size, winlen, cu_count);
}

int tk_conv1d_small_forward_dev(const float *x, const float *weight, const float *bias, size_t nblk, size_t nbatch,
                                size_t insize, size_t size, size_t winlen, int cu_count, float *y, void *stream) {
    return tk::conv_small_forward_dispatch(x, weight, bias, nblk, nbatch, insize, size, winlen, cu_count, y,
                                           static_cast<hipStream_t>(stream));
}

int tk_conv1d_small_backward_dev(const float *dy, const float *x, const float *weight, const float *bias, size_t nblk,
                                 size_t nbatch, size_t insize, size_t size, size_t winlen, int cu_count, float *dx,
                                 float *dweight, float *dbias, void *workspace, size_t workspace_bytes, void *stream) {
    return tk::conv_small_backward_dispatch(dy, x, weight, bias, nblk, nbatch, insize, size, winlen, cu_count, dx,
                                            dweight, dbias, workspace, workspace_bytes,
                                            static_cast<hipStream_t>(stream));
}

int tk_flipflop_lattice_dev(const float *scores, size_t nblk, size_t nbatch, size_t nbase, int forward,
                            const float *init, float *out, float *total, void *stream) {
    if (scores == nullptr || out == nullptr || total == nullptr) return TK_ERR_BAD_ARG;
    return tk::lattice_dispatch(scores, nblk, nbatch, nbase, forward, init, out, total,
                                static_cast<hipStream_t>(stream));
}

size_t tk_flipflop_beamsearch_workspace_bytes(size_t nblk, size_t nbatch, size_t nbase) {
    return tk::beam_workspace_bytes(nblk, nbatch, nbase);
}

int tk_flipflop_beamsearch_dev(const float *scores, size_t nblk, size_t nbatch, size_t nbase, int beam_width,
                               float beam_cut, int guided, int8_t *seq, int32_t *seqlen, float *score,
                               void *workspace, size_t workspace_bytes, void *stream) {
    if (!scores || !seq || !seqlen || !score || !workspace || nblk == 0 || nbatch == 0) return TK_ERR_BAD_ARG;
    return tk::beam_dispatch(scores, nblk, nbatch, nbase, beam_width, beam_cut, guided,
                             reinterpret_cast<signed char *>(seq), seqlen, score, workspace, workspace_bytes,
                             static_cast<hipStream_t>(stream));
}

size_t tk_flipflop_logz_workspace_bytes(size_t nblk, size_t nbatch, size_t nbase) {
    return tk::logz_workspace_bytes(nblk, nbatch, nbase);
}

int tk_flipflop_logz_dev(const float *scores, size_t nblk, size_t nbatch, size_t nbase,
                         float *logz, float *grad, void *workspace, size_t workspace_bytes,
                         uint32_t *status, void *stream) {
    if (!scores || !logz || !workspace || nblk == 0 || nbatch == 0) return TK_ERR_BAD_ARG;
    if (!tk::aligned16(scores) || (grad && !tk::aligned16(grad))) return TK_ERR_BAD_ARG;
    return tk::logz_dispatch(scores, nblk, nbatch, nbase, logz, grad, workspace,
                             workspace_bytes, status, static_cast<hipStream_t>(stream));
}

size_t tk_flipflop_viterbi_workspace_bytes(size_t nblk, size_t nbatch, size_t nbase) {
    return tk::viterbi_workspace_bytes(nblk, nbatch, nbase);
}

int tk_flipflop_viterbi_dev(const float *scores, size_t nblk, size_t nbatch, size_t nbase,
                            float *fwd, int64_t *traceback, int64_t *path, void *workspace,
                            size_t workspace_bytes, void *stream) {
    if (!scores || !path || !workspace || nbatch == 0) return TK_ERR_BAD_ARG;
    if (!tk::aligned16(scores)) return TK_ERR_BAD_ARG;
    if ((fwd == nullptr) != (traceback == nullptr)) return TK_ERR_BAD_ARG;      // both or neither
    return tk::viterbi_dispatch(scores, nblk, nbatch, nbase, fwd, traceback, path, workspace,
                                workspace_bytes, static_cast<hipStream_t>(stream));
}

/* ------------------------------------------------------------------------- *
 * exact reference prototypes on HOST pointers
 * ------------------------------------------------------------------------- */
namespace {

struct DevBuf {
    void *p = nullptr;
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess; }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

bool host_seq_call(float const *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                   size_t const *moveidxs, size_t const *stayidxs, size_t const *modmoveidxs,
                   float const *modmovefacts, int32_t const *seqlen, float *score, float *grad) {
    // reference layout -> padded per-position layout (moves: seqidx[b] - b, c_crf_flipflop.c:479)
    std::vector<int64_t> off(nbatch + 1, 0);
    int32_t maxlen = 0;
    for (size_t b = 0; b < nbatch; ++b) {
        off[b + 1] = off[b] + seqlen[b];
        if (seqlen[b] > maxlen) maxlen = seqlen[b];
    }
    const size_t total = (size_t)off[nbatch];
    std::vector<int32_t> stay(total ? total : 1), move(total ? total : 1), mod;
    std::vector<float> fact;
    if (modmoveidxs) {
        mod.assign(total ? total : 1, 0);
        fact.assign(total ? total : 1, 0.f);
    }
    // Read b's moves start after the moves of the reads before it.  The caller (ctc.pyx:127-134)
    // concatenates max(L - 1, 0) move ids per read, i.e. the start is off[b] minus the number of
    // NON-EMPTY reads before b.  The reference C indexes off[b] - b (c_crf_flipflop.c:479-480),
    // which is the same number when no read is empty and otherwise reads its neighbours' slots
    // (before the array, even): this entry point follows the array the caller actually built.
    std::vector<size_t> mstart(nbatch + 1, 0);
    for (size_t b = 0; b < nbatch; ++b) mstart[b + 1] = mstart[b] + (seqlen[b] > 0 ? (size_t)seqlen[b] - 1 : 0);
    auto mbase = [&](size_t b) { return mstart[b]; };
    for (size_t b = 0; b < nbatch; ++b) {
        const size_t L = (size_t)seqlen[b];
        for (size_t p = 0; p < L; ++p) {
            stay[off[b] + p] = (int32_t)stayidxs[off[b] + p];
            if (p + 1 < L) {
                move[off[b] + p] = (int32_t)moveidxs[mbase(b) + p];
                if (modmoveidxs) {
                    mod[off[b] + p] = (int32_t)modmoveidxs[mbase(b) + p];
                    fact[off[b] + p] = modmovefacts[mbase(b) + p];
                }
            } else {
                move[off[b] + p] = 0;
            }
        }
    }
    const size_t nelt = nblk * nbatch * ntrans;
    const size_t wsb = tk::crf_workspace_bytes_sharp(ntrans, nblk, nbatch, (size_t)maxlen, grad != nullptr, 1.0f);
    DevBuf d_lp, d_stay, d_move, d_mod, d_fact, d_len, d_off, d_cost, d_grad, d_ws;
    if (!d_lp.alloc(nelt * 4) || !d_stay.alloc(stay.size() * 4) || !d_move.alloc(move.size() * 4) ||
        !d_len.alloc(nbatch * 4) || !d_off.alloc((nbatch + 1) * 8) || !d_cost.alloc(nbatch * 4) ||
        !d_ws.alloc(wsb))
        return false;
    if (grad && !d_grad.alloc(nelt * 4)) return false;
    if (modmoveidxs && (!d_mod.alloc(mod.size() * 4) || !d_fact.alloc(fact.size() * 4))) return false;
    bool ok = true;
    ok &= hipMemcpy(d_lp.p, logprob, nelt * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(d_stay.p, stay.data(), stay.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(d_move.p, move.data(), move.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(d_len.p, seqlen, nbatch * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(d_off.p, off.data(), (nbatch + 1) * 8, hipMemcpyHostToDevice) == hipSuccess;
    if (modmoveidxs) {
        ok &= hipMemcpy(d_mod.p, mod.data(), mod.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
        ok &= hipMemcpy(d_fact.p, fact.data(), fact.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) return false;
    // The C layer of the reference works on lp directly (no sharpening, no -1/nblk):
    // score = +path score, grad = +posterior (c_crf_flipflop.c:434-516).  The device
    // entry point returns cost = -score/nblk and d cost, so undo that here.
    // canonical columns = everything below the first mod column (ids of stay/move < ncan <= mod ids)
    size_t ncan = ntrans;
    if (modmoveidxs) {
        for (size_t b = 0; b < nbatch; ++b)
            for (size_t p = 0; p + 1 < (size_t)seqlen[b]; ++p)
                if (modmoveidxs[mbase(b) + p] < ncan) ncan = modmoveidxs[mbase(b) + p];
    }
    tk::CrfCall c;
    c.lp = static_cast<const float *>(d_lp.p);
    c.ntrans = ntrans;
    c.nblk = nblk;
    c.nbatch = nbatch;
    c.max_seqlen = (size_t)maxlen;
    c.ncan = ncan;
    c.stay = static_cast<const int32_t *>(d_stay.p);
    c.move = static_cast<const int32_t *>(d_move.p);
    c.mod = modmoveidxs ? static_cast<const int32_t *>(d_mod.p) : nullptr;
    c.modfact = modmoveidxs ? static_cast<const float *>(d_fact.p) : nullptr;
    c.seqlen = static_cast<const int32_t *>(d_len.p);
    c.seqoff = static_cast<const int64_t *>(d_off.p);
    c.cost = static_cast<float *>(d_cost.p);
    c.grad = grad ? static_cast<float *>(d_grad.p) : nullptr;
    c.workspace = d_ws.p;
    c.workspace_bytes = wsb;
    const int rc = tk::crf_dispatch(c);
    if (rc != 0 || hipDeviceSynchronize() != hipSuccess) return false;
    std::vector<float> cost(nbatch);
    if (hipMemcpy(cost.data(), d_cost.p, nbatch * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (size_t b = 0; b < nbatch; ++b) {
        if (grad != nullptr && seqlen[b] == 0) continue;     // score untouched (:458-464)
        score[b] = -cost[b] * (float)nblk;
    }
    if (grad) {
        if (hipMemcpy(grad, d_grad.p, nelt * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
        const float s = -(float)nblk;
        for (size_t i = 0; i < nelt; ++i) grad[i] *= s;
    }
    return true;
}

void fail_scores(float *score, size_t nbatch) {
    for (size_t b = 0; b < nbatch; ++b) score[b] = NAN;     // c_crf_flipflop.c:278-282
}

}  // namespace

void crf_flipflop_grad(float const *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                       size_t const *moveidxs, size_t const *stayidxs, int32_t const *seqlen,
                       float *score, float *grad) {
    if (!host_seq_call(logprob, ntrans, nblk, nbatch, moveidxs, stayidxs, nullptr, nullptr, seqlen,
                       score, grad))
        fail_scores(score, nbatch);
}

void crf_flipflop_cost(float const *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                       size_t const *moveidxs, size_t const *stayidxs, int32_t const *seqlen,
                       float *score) {
    if (!host_seq_call(logprob, ntrans, nblk, nbatch, moveidxs, stayidxs, nullptr, nullptr, seqlen,
                       score, nullptr))
        fail_scores(score, nbatch);
}

void cat_mod_flipflop_grad(float const *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                           size_t const *moveidxs, size_t const *stayidxs,
                           size_t const *modmoveidxs, float const *modmovefacts,
                           int32_t const *seqlen, float *score, float *grad) {
    if (!host_seq_call(logprob, ntrans, nblk, nbatch, moveidxs, stayidxs, modmoveidxs,
                       modmovefacts, seqlen, score, grad))
        fail_scores(score, nbatch);
}

void cat_mod_flipflop_cost(float const *logprob, size_t ntrans, size_t nblk, size_t nbatch,
                           size_t const *moveidxs, size_t const *stayidxs,
                           size_t const *modmoveidxs, float const *modmovefacts,
                           int32_t const *seqlen, float *score) {
    if (!host_seq_call(logprob, ntrans, nblk, nbatch, moveidxs, stayidxs, modmoveidxs,
                       modmovefacts, seqlen, score, nullptr))
        fail_scores(score, nbatch);
}

}  // extern "C"

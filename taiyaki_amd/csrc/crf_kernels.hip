// crf_kernels.hip -- sequence-constrained flip-flop CRF score + gradient (plain and
// cat-mod) for gfx950.
//
// Replaces taiyaki/ctc/c_crf_flipflop.c:43-516 and c_cat_mod_flipflop.c:37-582
// (forward, backward, posterior scatter) and the index algebra of
// taiyaki/flipflopfings.py:6-31 / ctc.pyx:127-134,282-292.
//
// Two forms (see DESIGN.md "Kernel A"):
//   * crf_band.hip (default): banded skewed sweep + row-parallel posterior pass, both lattices
//     of the band in HBM.  This file holds its launcher, the index construction and
//   * crf_kernel below, the single-launch CHECKPOINT form for batches whose lattices would not
//     fit the workspace cap: one workgroup of W wavefronts per read, position-parallel (thread
//     g owns R consecutive lattice positions in registers, one DPP / LDS neighbour exchange and
//     one s_barrier per time step, log2-space LSE, column max every 4th step tracked in fp64);
//     the forward sweep stores one checkpoint column every CK steps, the backward sweep
//     recomputes each CK-column tile into LDS, walks it backwards fused with the backward
//     recursion and writes every posterior to a slot PRE-SORTED by transition id; at tile flush
//     a wave turns a row into per-id sums with a DPP prefix scan and boundary differences (no
//     atomics), normalises the row (c_crf_flipflop.c:400-401) and streams it out once.
#include <stdio.h>
#include <stdlib.h>

#include "crf_log.h"
#include "dispatch.h"

namespace tk {

// Workgroup n does read n (TK_CRF_MODE=ckpt, batches the band path does not take).  Behind a band launch the disowned
// reads are redone by that path's own tail launch (crf_band.hip: crf_band_tail_kernel), which calls crf_read itself.
template <int R, int W, bool MOD, bool VL = false>
__global__ __launch_bounds__(W *WAVE) void crf_kernel(CrfArgs a) {
    crf_read<R, W, MOD, VL>(a, (int)blockIdx.x, (int)blockIdx.x);
}

// ---------------------------------------------------------------------------
// index construction (flipflopfings.py:6-31, ctc.pyx:127-134, 282-292)
// ---------------------------------------------------------------------------
__global__ void seqoff_kernel(const int32_t *__restrict__ seqlen, int nbatch,
                              int64_t *__restrict__ seqoff, long long total_len, uint32_t *status) {
    // single block; chunked serial prefix sum (nbatch is a few thousand at most)
    __shared__ long long part[256];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int per = (nbatch + nt - 1) / nt;
    const int lo = min(nbatch, tid * per), hi = min(nbatch, lo + per);
    long long s = 0;
    for (int i = lo; i < hi; ++i) s += seqlen[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long acc = 0;
        for (int i = 0; i < nt; ++i) {
            const long long v = part[i];
            part[i] = acc;
            acc += v;
        }
    }
    __syncthreads();
    long long acc = part[tid];
    // Offsets are CLAMPED to the label array: a batch that announces more labels than it hands over
    // is flagged, and its reads end where the array ends (the CRF kernels take
    // min(seqlen, seqoff[n+1] - seqoff[n]) for a read's length): no kernel indexes past `total_len`.
    for (int i = lo; i < hi; ++i) {
        seqoff[i] = min(acc, total_len);
        acc += seqlen[i];
    }
    if (hi == nbatch && lo <= nbatch) {
        seqoff[nbatch] = min(acc, total_len);       // identical value from every writer
        if (acc > total_len && status) atomicOr(status, 8u);    // more labels announced than handed over
    }
}

__global__ void build_indices_kernel(const int32_t *__restrict__ seqs,
                                     const int32_t *__restrict__ seqlen,
                                     int64_t *__restrict__ seqoff, int nbatch, int nbase,
                                     const int32_t *__restrict__ mod_cats,
                                     const int32_t *__restrict__ can_mods_offsets,
                                     const float *__restrict__ mod_cat_weights,
                                     int32_t *__restrict__ stay, int32_t *__restrict__ move,
                                     int32_t *__restrict__ mod, float *__restrict__ fact,
                                     long long total_len, uint32_t *__restrict__ status) {
    const int n = blockIdx.x;
    // this read's offset = the sum of the lengths before it, clamped to the label array (see
    // seqoff_kernel): every workgroup sums for itself -- a batch is a few hundred reads, and it saves
    // the separate prefix-sum launch (~5 us of a 170 us loss path)
    __shared__ long long off_sh;
    __shared__ long long wsum[2][2];    // [wave][mine | all]: the block is two wavefronts
    if (nbatch == 0) {                  // (offsets already there: seqoff_kernel ran)
        if (threadIdx.x == 0) off_sh = seqoff[n];
        __syncthreads();
    } else {
        long long mine = 0, all = 0;
        for (int i = threadIdx.x; i < nbatch; i += blockDim.x) {
            const long long v = seqlen[i];
            all += v;
            if (i < n) mine += v;
        }
        // wave sums by butterfly, one hand-over through LDS -- the tree of fourteen barriers this replaces was
        // most of the kernel
        auto wave_sum = [&](long long v) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
            return v;
        };
        const long long wm = wave_sum(mine), wa = wave_sum(all);
        if ((threadIdx.x & (WAVE - 1)) == 0) {
            wsum[threadIdx.x >> 6][0] = wm;
            wsum[threadIdx.x >> 6][1] = wa;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long m = 0, t = 0;
            for (unsigned w = 0; w < (blockDim.x + WAVE - 1) / WAVE && w < 2; ++w) {
                m += wsum[w][0];
                t += wsum[w][1];
            }
            off_sh = m;
            seqoff[n] = min(m, total_len);
            if (n == nbatch - 1) {
                seqoff[nbatch] = min(t, total_len);
                if (t > total_len && status) atomicOr(status, 8u);      // more labels announced than handed over
            }
        }
        __syncthreads();
    }
    const int64_t off = min(off_sh, total_len);
    // (a batch that announces more labels than were handed over is flagged by seqoff_kernel;
    // here its reads are cut at the end of the label array)
    const int L = (int)max(0ll, min((long long)seqlen[n], total_len - (long long)off));
    const int ns = 2 * nbase, ncan = ns * (nbase + 1);
    bool bad = false;
    // the reference asserts 0 <= move / stay index < ntrans (ctc.pyx:127-134); a bad label is
    // clamped here, so that no kernel downstream gathers out of range, and reported
    auto label = [&](int64_t i) {
        const int c = seqs[i];
        bad |= c < 0 || c >= ns;
        return min(max(c, 0), ns - 1);
    };
    for (int p = threadIdx.x; p < L; p += blockDim.x) {
        const int cp = label(off + p);
        stay[off + p] = cp + min(cp, nbase) * ns;                 // flipflopfings.py:20-31
        if (p + 1 < L) {
            const int cn = label(off + p + 1);
            move[off + p] = cp + min(cn, nbase) * ns;             // flipflopfings.py:6-17
            if (mod_cats != nullptr) {
                // ctc.pyx:288-292
                const int lo = can_mods_offsets[cn % nbase], hi = can_mods_offsets[cn % nbase + 1];
                int mseq = lo + mod_cats[off + p + 1];
                bad |= mseq < lo || mseq >= hi;
                mseq = min(max(mseq, lo), hi - 1);
                mod[off + p] = ncan + mseq;
                fact[off + p] = mod_cat_weights[mseq];
            }
        } else {
            move[off + p] = 0;
            if (mod_cats != nullptr) {
                mod[off + p] = ncan;
                fact[off + p] = 0.f;
            }
        }
    }
    if (bad && status) atomicOr(status, 8u);
}

int build_indices_dispatch(const int32_t *seqs, const int32_t *seqlen, size_t nbatch,
                           size_t nbase, const int32_t *mod_cats,
                           const int32_t *can_mods_offsets, const float *mod_cat_weights,
                           int64_t *seqoff, int32_t *stay, int32_t *move, int32_t *mod,
                           float *fact, size_t total_len, uint32_t *status, hipStream_t stream) {
    // (one launch: every workgroup computes its read's offset itself; seqoff_kernel is kept for
    // batches of more than 8192 reads, where the redundant sums would cost more than a launch)
    if (nbatch > 8192)
        hipLaunchKernelGGL(seqoff_kernel, dim3(1), dim3(256), 0, stream, seqlen, (int)nbatch, seqoff,
                           (long long)total_len, status);
    hipLaunchKernelGGL(build_indices_kernel, dim3((unsigned)nbatch), dim3(128), 0, stream, seqs,
                       seqlen, seqoff, (int)(nbatch > 8192 ? 0 : nbatch), (int)nbase, mod_cats, can_mods_offsets, mod_cat_weights,
                       stay, move, mod, fact, (long long)total_len, status);
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

// ---------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------
struct CrfShape {
    int R, W;
};

// (R, W) from the longest sequence: 2 cells per lane, up to 16 waves, then deeper strips
static CrfShape crf_pick_shape(size_t max_seqlen) {
    if (max_seqlen <= WAVE) return {1, 1};
    int W = 1;
    while ((size_t)2 * W * WAVE < max_seqlen && W < 16) W *= 2;
    int R = 2;
    while ((size_t)R * W * WAVE < max_seqlen) R *= 2;
    return {R, W};
}

// Which form of kernel A runs (TK_CRF_MODE overrides: band | ckpt):
//   band     crf_band.hip -- linear-domain banded skewed sweep + recomputing gradient pass, followed
//            by ONE tail launch (crf_band.hip: crf_band_tail_kernel) that retries the reads the band path disowned alone
//            and redoes in the log domain (crf_read, crf_log.h) what it disowns twice
//            (default whenever the sequences fit 16 waves x 256 cells and the checkpoint columns
//            fit the workspace cap)
//   ckpt     the single-launch log-domain checkpoint/recompute kernel of this file on every read:
//            three serial passes per read (workspace-bound batches, and the band path's safety net)
enum CrfMode { CRF_BAND, CRF_CKPT };
static size_t crf_lattice_cap_bytes() {
    // TK_CRF_LATTICE_MB, else a quarter of THIS device's memory (72 GB of an MI355X's 288; round 3's checkpoint
    // columns are 3.9 GB at T = 4000 / N = 256, so the cap is about smaller devices and partitions, and about
    // callers that do not know their longest sequence).  No device (the build container): 40 GiB.
    if (const char *e = TK_LAB_ENV("TK_CRF_LATTICE_MB")) return (size_t)atoll(e) * 1024 * 1024;
    static size_t cap[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return (size_t)40960 * 1024 * 1024;
    }
    if (cap[dev] == 0) {
        size_t total = 0;
        if (hipDeviceTotalMem(&total, dev) != hipSuccess || total == 0) {
            (void)hipGetLastError();
            total = (size_t)160 * 1024 * 1024 * 1024;
        }
        cap[dev] = total / 4;
    }
    return cap[dev];
}
// `bk`: the block length the linear path would use for this call (crf_band_pick_block; 0 = it does not take it).
// The band layout is checked against the cap for both forms: the plain CRF and cat-mod may pick different cells per
// lane (crf_band_pick_R), hence different padded read lengths -- the bound covers both.
static CrfMode crf_pick_mode(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, bool want_grad, int bk) {
    const char *e = TK_LAB_ENV("TK_CRF_MODE");
    if ((e && e[0] == 'c') || bk <= 0 || !crf_band_fits(max_seqlen)) return CRF_CKPT;
    const size_t a = crf_band_layout(ntrans, nblk, nbatch, max_seqlen, true, want_grad, bk).total;
    const size_t b = crf_band_layout(ntrans, nblk, nbatch, max_seqlen, false, want_grad, bk).total;
    return (a > b ? a : b) <= crf_lattice_cap_bytes() ? CRF_BAND : CRF_CKPT;
}

// THE WORKSPACE PLAN of one call: [band layout | the retry's band layout | checkpoint columns + offsets of the log-domain form].
// Band mode (`bk` > 0): the batch launch's layout; the retry's (`rbk` > 0, round 6: the band layout of 4-step blocks for
// crf_band_retry_slots(nbatch) reads, gradient form whatever the call -- a cost-only retry runs the same sweeps); and one set
// of checkpoint columns per workgroup of the TAIL launch (crf_band.hip: crf_band_tail_kernel -- 16 waves, cells per lane by
// the retry's): a sixteenth of the batch, at least 4 -- it redoes only what the linear path disowned twice, none on the inputs
// a network produces (round 3 sized them for the whole batch: 8.4 of 12.2 GB at T = 4000 / N = 256).  Checkpoint mode
// (`bk` = 0): crf_kernel's columns, one set per read.
struct CrfPlan {
    BandLayout band, retry;     // at 0 and at band.total (total 0: not in this plan)
    CrfShape sh;                // the log-domain form: its shape and workgroups
    size_t nslots;
    size_t ck, ckcols, total;   // its region: at ck, ckcols bytes of columns (the call's kinds), then the offsets, up to total
};
static CrfPlan crf_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, bool mod, bool want_grad, int bk, int rbk) {
    CrfPlan p{};
    p.sh = crf_pick_shape(max_seqlen);
    p.nslots = nbatch;
    if (bk > 0) {
        p.band = crf_band_layout(ntrans, nblk, nbatch, max_seqlen, mod, want_grad, bk);
        p.nslots = crf_band_retry_slots(nbatch);
        if (rbk > 0) p.retry = crf_band_layout(ntrans, nblk, p.nslots, max_seqlen, mod, true, rbk, crf_band_retry_R(max_seqlen));
        p.sh = {crf_tail_log_R(crf_band_retry_R(max_seqlen)), 16};
    }
    // one column of R W 64 cells every CK steps, NK per workgroup; then one offset per column
    auto NK = [&](int kinds) {
        const size_t CK = (size_t)crf_ck(p.sh.R, p.sh.W, kinds);
        return (nblk + CK - 1) / CK;
    };
    auto aligned = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t cells = p.nslots * (size_t)p.sh.R * p.sh.W * WAVE;
    // (a cost-only call keeps no checkpoint column: crf_kernel stores them under want_grad only)
    p.ck = p.band.total + p.retry.total;
    // (the region is sized for three kinds: the cat-mod tile is the smaller one, an upper bound for both)
    p.ckcols = want_grad ? aligned(cells * NK(mod ? 3 : 2) * sizeof(float)) : 0;
    p.total = p.ck + (want_grad ? aligned(cells * NK(3) * sizeof(float)) + aligned(p.nslots * NK(3) * sizeof(double)) + 256 : 256);
    return p;
}

// `sharp`: the call's sharpening factor -- it picks the linear path's block length, and short blocks keep
// more checkpoint columns.  The block lengths of the plain CRF and of cat-mod differ; the bound covers both.
size_t crf_workspace_bytes_sharp(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen,
                                 int want_grad, float sharp) {
    if (max_seqlen == 0) max_seqlen = nblk + 1;
    const bool g = want_grad != 0;
    // (every block length either form may take for this shape: with and without per-column factors; a batch with narrow
    // bands takes 8 steps where wider ones take 12)
    // (... and whatever the batch's bulk is: between "unknown" and "every read as long as the longest")
    auto shortest = [](int x, int y) { return (x > 0 && y > 0) ? (x < y ? x : y) : (x > 0 ? x : y); };
    int bk = 0;
    for (int bulk = 0; bulk < 2; ++bulk)
        for (int form = 0; form < 3; ++form)
            bk = shortest(bk, crf_band_pick_block(sharp, form > 0, max_seqlen, form == 2, nblk, bulk ? max_seqlen : 0).bk);
    // (a call whose own block choice differs from the one assumed here -- another sharpening factor than the
    // query's -- needs what ITS factor's query returns; with less, crf_dispatch falls back to the log-domain
    // kernel on every read if the workspace holds that kernel's whole-batch columns, and returns 3 otherwise:
    // sizing every workspace for that case would be 8.0 instead of 4.7 GB at T = 4000 / N = 256)
    if (crf_pick_mode(ntrans, nblk, nbatch, max_seqlen, g, bk) != CRF_BAND)
        return crf_plan(ntrans, nblk, nbatch, max_seqlen, false, g, 0, 0).total;
    // (each band region the larger of the plain CRF's and cat-mod's: see crf_pick_mode)
    const CrfPlan p = crf_plan(ntrans, nblk, nbatch, max_seqlen, false, g, bk, 4);
    const CrfPlan q = crf_plan(ntrans, nblk, nbatch, max_seqlen, true, g, bk, 4);
    auto larger = [](size_t x, size_t y) { return x > y ? x : y; };
    return larger(p.band.total, q.band.total) + larger(p.retry.total, q.retry.total) + (p.total - p.ck);
}

template <int R, int W, bool MOD>
static int crf_launch_one(const CrfArgs &a, hipStream_t stream, size_t nwg) {
    const size_t lds = crf_lds_bytes(R, W, a.S, MOD ? 3 : 2);
    if (lds > 160 * 1024) return 2;
    if (raise_dynamic_lds(reinterpret_cast<const void *>(&crf_kernel<R, W, MOD, CRF_VL>))) return 4;
    hipLaunchKernelGGL((crf_kernel<R, W, MOD, CRF_VL>), dim3((unsigned)nwg), dim3(W * WAVE), lds, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

template <bool MOD>
static int crf_launch_mod(CrfShape sh, const CrfArgs &a, hipStream_t stream, size_t nwg) {
    const int key = sh.R * 100 + sh.W;
#define TK_CRF_CASE(R_, W_)                                                           \
    case R_ * 100 + W_:                                                               \
        return crf_launch_one<R_, W_, MOD>(a, stream, nwg);
    switch (key) {
        TK_CRF_CASE(1, 1)
        TK_CRF_CASE(2, 1)
        TK_CRF_CASE(2, 2)
        TK_CRF_CASE(2, 4)
        TK_CRF_CASE(2, 8)
        TK_CRF_CASE(2, 16)
        TK_CRF_CASE(4, 16)
        default: return 2;
    }
#undef TK_CRF_CASE
}

// The fields CrfArgs and BandArgs share, from the call (the two structs keep their own layouts: the kernels read them).
// `ids_from` non-null: this launch forms its ids from those labels and writes no index array (crf_band.h: BandArgs::codes).
template <class Args>
static void crf_fill_args(Args &x, const CrfCall &c, const SeqLabels *ids_from) {
    x.lp = c.lp;
    x.T = (int)c.nblk;
    x.N = (int)c.nbatch;
    x.S = (int)c.ntrans;
    x.ncan = (int)c.ncan;
    x.stay = c.stay;
    x.move = c.move;
    x.mod = c.mod;
    x.modfact = c.modfact;
    x.seqlen = c.seqlen;
    x.seqoff = c.seqoff;
    x.c_can = c.sharp_can * LOG2E;
    x.c_mod = c.sharp_mod * LOG2E;
    x.out_scale = c.out_scale;
    x.grad_scale = c.grad_scale;
    x.grad_scale_vec = c.grad_scale_vec;
    x.add_grad = c.add_grad;
    x.add_cost = c.add_cost;
    x.add_S = c.add_S;
    x.add_scale = c.add_scale;
    x.cost = c.cost;
    x.grad = c.grad;
    x.status = c.status;
    // (a batch of empty reads has no label array: any non-null pointer says "build here", nothing reads it)
    x.codes = ids_from != nullptr ? (ids_from->seqs != nullptr ? ids_from->seqs : c.stay) : nullptr;
    x.mod_cats = ids_from != nullptr ? ids_from->mod_cats : nullptr;
    x.cmo = ids_from != nullptr ? ids_from->can_mods_offsets : nullptr;
    x.mcw = ids_from != nullptr ? ids_from->mod_cat_weights : nullptr;
    x.nbase = ids_from != nullptr ? (int)ids_from->nbase : 0;
#ifdef TK_LOSS_VARLEN
    x.lengths = c.lengths;
#endif
}

// a band layout placed at `base` -> the sweep and gradient-pass arrays of a launch (a cost-only launch has only the scores)
static void crf_bind_layout(BandArgs &b, const BandLayout &l, char *base, bool g) {
    b.W = l.W;
    b.LP = (int)l.LP;
    b.Wp = (int)(l.LP / WAVE);
    b.ckFm = g ? reinterpret_cast<float *>(base + l.ckFm) : nullptr;
    b.ckBm = g ? reinterpret_cast<float *>(base + l.ckBm) : nullptr;
    b.ckFf = g ? reinterpret_cast<int16_t *>(base + l.ckFf) : nullptr;
    b.ckBf = g ? reinterpret_cast<int16_t *>(base + l.ckBf) : nullptr;
    b.ckFb = g ? reinterpret_cast<int *>(base + l.ckFb) : nullptr;
    b.ckBb = g ? reinterpret_cast<int *>(base + l.ckBb) : nullptr;
    b.bndF = g ? reinterpret_cast<float *>(base + l.bndF) : nullptr;
    b.bndB = g ? reinterpret_cast<float *>(base + l.bndB) : nullptr;
    b.scoreF = reinterpret_cast<double *>(base + l.scoreF);
    b.scoreB = reinterpret_cast<double *>(base + l.scoreB);
    b.rec = g ? reinterpret_cast<uint32_t *>(base + l.rec) : nullptr;
    b.segend = g ? reinterpret_cast<int *>(base + l.segend) : nullptr;
}

// lab (TK_CRF_GATE_DUMP; tests/helpers/gate_dump.py reads it): the reads the batch's launch disowned; with `rblk`, the tail's verdicts
static void crf_gate_dump(const BandArgs &b, const BandBlock *rblk, size_t nbatch, hipStream_t stream) {
    if (!TK_LAB_ENV("TK_CRF_GATE_DUMP")) return;
    (void)hipStreamSynchronize(stream);
    static int h1[1 << 16], h2[1 << 16];
    const size_t ng = nbatch < (1u << 16) ? nbatch : (1u << 16);
    (void)hipMemcpy(h1, b.gate, ng * sizeof(int), hipMemcpyDeviceToHost);
    if (rblk != nullptr) (void)hipMemcpy(h2, b.gate2, ng * sizeof(int), hipMemcpyDeviceToHost);
    size_t cnt = 0, why[8] = {0}, tried = 0, kept = 0;
    for (size_t i = 0; i < ng; ++i) {
        cnt += h1[i] != 0;
        ++why[h1[i] & 7];
        tried += h2[i] != -1;
        kept += h2[i] == 0;
    }
    if (rblk == nullptr)
        fprintf(stderr, "crf band: %zu of %zu reads gated (non-finite score %zu, sweeps disagree %zu, row lost mass %zu)\n",
                cnt, ng, why[1], why[4], why[2]);
    else
        fprintf(stderr, "crf band tail (retry: bk %d, bias %.1f, slope %d): %zu reads taken, %zu kept on the linear path\n",
                rblk->bk, rblk->wbias, rblk->klip, tried, kept);
    for (size_t i = 0, shown = 0; i < ng && shown < 16; ++i) {
        if (rblk == nullptr && h1[i]) fprintf(stderr, "crf band:   read %zu (reason %d)\n", i, h1[i]), ++shown;
        if (rblk != nullptr && h2[i] > 0) fprintf(stderr, "crf band tail:   read %zu first %d retry %d\n", i, h1[i], h2[i]), ++shown;
    }
}

// WHAT crf_dispatch MAKES OF A CALL, before it touches a pointer: the form (linear path or log domain on every read), the
// linear path's block configuration and its retry's, and the workspace plan.  rc != 0: the call is refused (2: no
// instantiation for the shape, 3: the workspace holds neither form).  The lab build's plan query reports the same choice.
struct CrfChoice {
    int rc;
    bool band;
    BandBlock blk, rblk;
    CrfPlan p;
};
static CrfChoice crf_choose(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, bool mod, bool colw,
                            bool g, float sharp, size_t workspace_bytes) {
    CrfChoice ch{};
    const CrfShape sh = crf_pick_shape(max_seqlen);
    if ((size_t)sh.R * sh.W * WAVE < max_seqlen || sh.R > 4) {
        ch.rc = 2;
        return ch;
    }
    // the linear path's block length for this sharpening factor; when the workspace the caller brought is
    // too small for it (sized without the factor: tk_crf_flipflop_workspace_bytes) but large enough for the
    // log-domain kernel on every read, that kernel does the call
    ch.blk = crf_band_pick_block(sharp, mod, max_seqlen, mod && colw, nblk, bulk_seqlen);
    ch.band = crf_pick_mode(ntrans, nblk, nbatch, max_seqlen, g, ch.blk.bk) == CRF_BAND;
    // the second chance for what the batch's launch disowns (round 6); left out when the workspace the caller brought has no
    // room for it (sized by an older query): such reads go straight to the log-domain kernel, as in round 5
    ch.rblk = ch.band ? crf_band_pick_retry(sharp, ch.blk) : BandBlock{0, 0.f, 0};
    auto plan = [&](int bk, int rbk) { return crf_plan(ntrans, nblk, nbatch, max_seqlen, mod, g, bk, rbk); };
    ch.p = plan(ch.band ? ch.blk.bk : 0, ch.rblk.bk);
    if (ch.band && ch.p.total > workspace_bytes) {
        ch.rblk.bk = 0;
        ch.p = plan(ch.blk.bk, 0);
    }
    if (ch.band && ch.p.total > workspace_bytes) {
        ch.band = false;
        ch.p = plan(0, 0);
    }
    if (!ch.band && ch.p.total > workspace_bytes) ch.rc = 3;
    return ch;
}

#if defined(TK_LAB) || defined(TK_LOSS_VARLEN)
// tk_lab_crf_plan (dispatch.h) and, in the -DTK_LOSS_VARLEN build, tk_crf_varlen_plan: the choice above and what the launchers
// behind it make of it, as numbers
bool crf_lab_plan(size_t ntrans, size_t nblk, size_t nbatch, size_t max_seqlen, size_t bulk_seqlen, int form, int want_grad,
                  float sharp, size_t workspace_bytes, size_t *out) {
    for (int i = 0; i < 20; ++i) out[i] = 0;
    if (ntrans > 62 || ntrans == 0 || form < 0 || form > 2) return false;
    if (max_seqlen == 0) max_seqlen = nblk + 1;
    const bool mod = form > 0, colw = form == 1;
    const CrfChoice ch = crf_choose(ntrans, nblk, nbatch, max_seqlen, bulk_seqlen, mod, colw, want_grad != 0, sharp, workspace_bytes);
    if (ch.rc != 0) return false;
    const int kinds = mod ? 3 : 2;
    if (!ch.band && crf_lds_bytes(ch.p.sh.R, ch.p.sh.W, (int)ntrans, kinds) > 160 * 1024) return false;     // (crf_launch_one)
    auto halves = [](float bias) { return (size_t)(bias * 2.f + 0.5f); };
    out[0] = ch.band ? 0 : 1;
    out[1] = (size_t)ch.p.sh.R;
    out[2] = (size_t)ch.p.sh.W;
    out[3] = (size_t)crf_ck(ch.p.sh.R, ch.p.sh.W, kinds);
    out[18] = ch.p.nslots;
    if (!ch.band) return true;
    const BandLayout &l = ch.p.band;
    const bool rows = crf_band_use_rows(l.W, (int)ntrans, mod, colw, ch.blk.bk);
    out[4] = (size_t)l.R;
    out[5] = (size_t)l.W;
    out[6] = (size_t)ch.blk.bk;
    out[7] = halves(ch.blk.wbias);
    out[8] = (size_t)ch.blk.klip;
    out[9] = rows ? 1 : 0;
    out[10] = (size_t)crf_band_wave_class(l.R, ch.blk.bk, l.W + (rows ? 1 : 0));
    const int rR = crf_band_retry_R(max_seqlen);
    if (ch.rblk.bk > 0) {
        out[11] = (size_t)ch.rblk.bk;
        out[12] = halves(ch.rblk.wbias);
        out[13] = (size_t)ch.rblk.klip;
        out[14] = (size_t)ch.p.retry.R;
        out[15] = (size_t)ch.p.retry.W;
        out[16] = crf_band_tail_side_by_side(ch.p.retry.W) ? 1 : 0;
    }
    out[17] = (size_t)crf_tail_log_R(rR);
    out[19] = (size_t)rR;       // the tail launch's instantiation (crf_band_tail_dispatch), with or without a retry
    return true;
}
#endif

int crf_dispatch(const CrfCall &c) {
    const SeqLabels *labels = c.labels;
    if (c.ntrans > 62 || c.ncan > c.ntrans || c.ncan == 0) return 2;
    if (labels != nullptr && ((labels->seqs == nullptr && labels->total_len != 0) || labels->nbase == 0 ||
                              2 * labels->nbase * (labels->nbase + 1) != c.ncan ||
                              ((c.mod != nullptr) != (labels->mod_cats != nullptr)) ||
                              (labels->mod_cats != nullptr && (labels->can_mods_offsets == nullptr || labels->mod_cat_weights == nullptr))))
        return 1;
    const size_t max_seqlen = c.max_seqlen != 0 ? c.max_seqlen : c.nblk + 1;
    const bool mod = c.mod != nullptr, g = c.grad != nullptr;
    const CrfChoice ch = crf_choose(c.ntrans, c.nblk, c.nbatch, max_seqlen, labels != nullptr ? labels->bulk_seqlen : 0, mod,
                                    c.mod_col_weights != nullptr, g, c.sharp_can, c.workspace_bytes);
    if (ch.rc != 0) return ch.rc;
    const bool band = ch.band;
    const BandBlock &blk = ch.blk, &rblk = ch.rblk;
    const CrfPlan &p = ch.p;
    if (labels != nullptr && !band) {
        // the index arrays are OUTPUTS of this call; the band launch builds them itself, this path takes the
        // stand-alone kernel (tk_flipflop_build_indices_dev's)
        const int rc = build_indices_dispatch(labels->seqs, c.seqlen, c.nbatch, labels->nbase, labels->mod_cats,
                                              labels->can_mods_offsets, labels->mod_cat_weights, const_cast<int64_t *>(c.seqoff),
                                              const_cast<int32_t *>(c.stay), const_cast<int32_t *>(c.move),
                                              const_cast<int32_t *>(c.mod), const_cast<float *>(c.modfact), labels->total_len,
                                              c.status, c.stream);
        if (rc != 0) return rc;
    }
    char *wb = static_cast<char *>(c.workspace);
    // (ids from the labels wherever the band launch took them: it wrote no index array)
    CrfArgs a;
    crf_fill_args(a, c, band ? labels : nullptr);
    a.ckpt = reinterpret_cast<float *>(wb + p.ck);
    a.ckoff = reinterpret_cast<double *>(wb + p.ck + p.ckcols);
    // (what add_grad / add_cost hold may come from another stream: the band path waits between its sweeps
    // and its gradient pass, the single-launch form before it starts)
    if (c.add_ready != nullptr && !(band && g) && hipStreamWaitEvent(c.stream, c.add_ready, 0) != hipSuccess) return 4;
    if (!band) return mod ? crf_launch_mod<true>(p.sh, a, c.stream, c.nbatch) : crf_launch_mod<false>(p.sh, a, c.stream, c.nbatch);

    BandArgs b;
    crf_fill_args(b, c, labels);
    b.total_len = labels != nullptr ? (long long)labels->total_len : 0;
    crf_bind_layout(b, p.band, wb, g);
    b.gate = reinterpret_cast<int *>(wb + p.band.gate);
    b.gate2 = reinterpret_cast<int *>(wb + p.band.gate2);
    b.anygate = g ? reinterpret_cast<int *>(wb + p.band.anygate) : nullptr;
    b.zeros = reinterpret_cast<const float *>(wb + p.band.zeros);
    b.dbg = nullptr;
    b.before_gradient = c.add_ready;
    b.colw = mod ? c.mod_col_weights : nullptr;
    b.wbias = blk.wbias;
    b.klip = blk.klip;
    const int rc = crf_band_dispatch(b, p.band.R, mod, blk.bk, c.stream);
    if (rc != 0) return rc;
    crf_gate_dump(b, nullptr, c.nbatch, c.stream);
    // THE TAIL LAUNCH (round 6; crf_band.hip: crf_band_tail_kernel): the reads the batch's launch disowned, once more on
    // the linear path -- alone, 4-step blocks, steep frames -- and what that disowns too, redone in the log domain by the
    // same workgroup.  One launch; it finds nothing to do on the inputs a network produces.
    BandArgs t = b;
    t.gate = nullptr;
    t.gate2 = nullptr;
    t.anygate = nullptr;
    if (rblk.bk > 0) {
        crf_bind_layout(t, p.retry, wb + p.band.total, true);
        t.wbias = rblk.wbias;
        t.klip = rblk.klip;
    }
    // (the offsets and -- a call that brought index arrays -- the ids are the batch launch's; a launch that built its
    // ids from the labels left seqoff behind, and the tail forms its ids from the codes as well)
    BandRetry r;
    r.gate = b.gate;
    r.gate2 = b.gate2;
    r.firstF = g ? nullptr : b.scoreF;
    r.firstB = g ? nullptr : b.scoreB;
    r.first_wbias = blk.wbias;
    r.anygate = b.anygate;
    r.retry = rblk.bk > 0 ? 1 : 0;
    r.log_domain = 1;
    if (const char *e = TK_LAB_ENV("TK_CRF_NO_FALLBACK"))       // lab: time / test the linear path alone
        if (e[0] == '1') r.log_domain = 0;
    // (the tail launch has its own cells per lane: the retry's sweeps run side by side when 2 W waves fit its 16)
    const int rr = crf_band_tail_dispatch(t, r, a, crf_band_retry_R(max_seqlen), mod, p.nslots, c.stream);
    if (rr != 0) return rr;
    crf_gate_dump(b, &rblk, c.nbatch, c.stream);
    return 0;
}

}  // namespace tk

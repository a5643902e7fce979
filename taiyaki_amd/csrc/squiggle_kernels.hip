// squiggle_kernels.hip -- squiggle-match cost, gradient and alignment path (gfx950).
//
// Replaces taiyaki/squiggle_match (c_squiggle_match.c + squiggle_match.pyx): the dynamic programme
// that scores an observed signal against a predicted squiggle (per position: level, log-scale and
// move logit), used by bin/train_squiggle.py (squiggle_match_loss) and bin/map_to_squiggle.py
// (squiggle_match_path).  The reference runs it on the host, one OpenMP thread per read.
//
// States: npos positions plus one "back" state per position.  Per signal sample a position may
// stay, move on by one, or step into the back state of the position before it; a back state may
// stay or move out into the position after it.  Emission is a Laplace density shared by a position
// and its back state.
//
// One wave (one 64-thread workgroup) per read; lane l owns the R consecutive positions
// [l R, (l+1) R) and their back states in registers.  A sample step needs the left neighbour's
// last position and back state and the right neighbour's first position: three DPP wave shifts,
// no LDS and no barrier.  R is a template parameter (npos <= 64 R; up to 1024 positions).
//
//   sq_forward_kernel   forward sweep (c_squiggle_match.c:108-186); writes the negated score and,
//                       when asked, every column of the lattice for the gradient
//   sq_backward_kernel  backward sweep (:189-267) over the stored forward columns, accumulating the
//                       three gradients of a position in the registers of the lane that owns it
//                       (:591-694, as written there), written once at the end
//   sq_viterbi_kernel   Viterbi with start / end states (:270-454), a byte of traceback per
//                       (sample, position) and an int32 per sample for the end state; the wave walks
//                       the traceback back in chunks staged through LDS and writes the flat path.
//
// Precision.  The forward / backward sweeps use hardware exp / log in logsumexp (their outputs are
// compared against tolerances).  The Viterbi reproduces the reference bit for bit: the same float
// operations in the same order, the reference's emission rounding (float, then minus the double
// M_LN2, rounded back to float), strict '>' in the reference's candidate order, and no FP
// contraction in this file.
#include "ff_common.h"
#include "../../include/taiyaki_amd_flipflop.h"
#include "squiggle_match.h"

#pragma clang fp contract(off)

namespace tk {

constexpr float SQ_LARGE = 1e30f;           // c_squiggle_match.c:7 LARGE_VAL
constexpr int SQ_TB_ROWS = 32;              // traceback rows staged in LDS per walk chunk


// c_squiggle_match.c:10-12: float arithmetic, then the double M_LN2, rounded back to float
__device__ __forceinline__ float sq_loglaplace(float x, float loc, float sc, float logsc) {
    const float t = -fabsf(x - loc) / sc - logsc;
    return (float)((double)t - 0.69314718055994530942);
}

__device__ __forceinline__ float sq_plogistic(float x) { return 0.5f * (1.0f + tanhf(x / 2.0f)); }

// natural-log logsumexp on the hardware exp2 / log2 (c_squiggle_match.c:62-64 up to an ulp)
__device__ __forceinline__ float sq_lse(float a, float b) {
    const float mx = fmaxf(a, b);
    return mx + fast_log2(1.0f + fast_exp2(-fabsf(a - b) * LOG2E)) * LN2;
}

// The read a workgroup sweeps, or false (and the status flag) when its length is not usable:
// siglen <= 0 or a read that runs past the end of `signal`.  The test is the same in every lane.
__device__ __forceinline__ bool sq_read(const SqArgs &a, int b, int64_t &off, int &n) {
    n = a.siglen[b];
    off = a.sig_off[b];
    const bool ok = n > 0 && off >= 0 && off + n <= a.nsignal && a.sig_off[b + 1] == off + n;
    if (!ok && threadIdx.x == 0 && a.status) atomicOr(a.status, TK_STATUS_BAD_SIGLEN);
    return ok;
}

// Per-position tables of one read (c_squiggle_match.c:124-130, 474-477): loc, logsc, sc = exp(logsc),
// move_pen = log((1 - pb) plogistic(m)), stay_pen = log1p(-mp - pb).  Padding positions get zeros.
template <int R>
struct SqTables {
    float loc[R], logsc[R], sc[R], mpen[R], spen[R], mlogit[R];

    __device__ __forceinline__ void load(const SqArgs &a, int b, int lane) {
        const size_t ldp = (size_t)a.nbatch * 3;
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int p = lane * R + i;
            float l = 0.0f, ls = 0.0f, m = 0.0f;
            if (p < a.npos) {
                const float *q = a.params + (size_t)p * ldp + (size_t)b * 3;
                l = q[0];
                ls = q[1];
                m = q[2];
            }
            loc[i] = l;
            logsc[i] = ls;
            sc[i] = expf(ls);
            mlogit[i] = m;
            const float mp = (1.0f - a.prob_back) * sq_plogistic(m);
            mpen[i] = logf(mp);
            spen[i] = log1pf(-mp - a.prob_back);
        }
    }
};

// The sample of step s: one coalesced load per 64 samples, then a lane read with a uniform index.
struct SqSignal {
    const float *base;
    int n;
    float cache;
    int chunk;
    __device__ __forceinline__ void init(const float *p, int len) {
        base = p;
        n = len;
        chunk = -1;
        cache = 0.0f;
    }
    __device__ __forceinline__ float at(int s, int lane) {
        const int c = s >> 6;
        if (c != chunk) {       // (uniform)
            chunk = c;
            const int k = (c << 6) + lane;
            cache = k < n ? base[k] : 0.0f;
        }
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cache), s & 63));
    }
};

// ---------------------------------------------------------------------------------------------------
// forward sweep (c_squiggle_match.c:108-186)
// ---------------------------------------------------------------------------------------------------
template <int R, bool STORE>
__global__ __launch_bounds__(64) void sq_forward_kernel(SqArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int64_t off;
    int n;
    if (!sq_read(a, b, off, n)) {
        if (lane == 0 && a.cost) a.cost[b] = __int_as_float(0x7fc00000);
        return;
    }
    const int npos = a.npos;
    SqTables<R> t;
    t.load(a, b, lane);
    const float lnhalf = logf(0.5f), lnpb = logf(a.prob_back);
    SqSignal sig;
    sig.init(a.signal + off, n);

    float fp[R], fb[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        fp[i] = (lane * R + i == 0) ? 0.0f : -SQ_LARGE;     // point prior at position 0
        fb[i] = -SQ_LARGE;
    }
    constexpr int RS = 2 * 64 * R;          // floats per stored column
    float *col = STORE ? a.lattice + (size_t)(off + b) * RS : nullptr;
    if (STORE) {
#pragma unroll
        for (int i = 0; i < R; i++) {
            col[lane * R + i] = fp[i];
            col[64 * R + lane * R + i] = fb[i];
        }
    }
    for (int s = 0; s < n; s++) {
        const float x = sig.at(s, lane);
        const float pl = wave_shift_up1(fp[R - 1], -SQ_LARGE);
        const float bl = wave_shift_up1(fb[R - 1], -SQ_LARGE);
        const float pr = wave_shift_down1(fp[0], -SQ_LARGE);
        float np[R], nb[R];
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int p = lane * R + i;
            const float prevp = i == 0 ? pl : fp[i - 1];
            const float prevb = i == 0 ? bl : fb[i - 1];
            const float nextp = i == R - 1 ? pr : fp[i + 1];
            float v = fp[i] + t.spen[i];                                    // stay
            float w = fb[i] + lnhalf;                                       // stay in back
            if (p >= 1) v = sq_lse(v, prevp + t.mpen[i]);                   // move on
            if (p + 1 < npos) w = sq_lse(w, nextp + lnpb);                  // move into back
            if (p >= 1) v = sq_lse(v, prevb + lnhalf);                      // move out of back
            const float em = sq_loglaplace(x, t.loc[i], t.sc[i], t.logsc[i]);
            np[i] = p < npos ? v + em : -SQ_LARGE;
            nb[i] = p < npos ? w + em : -SQ_LARGE;
        }
#pragma unroll
        for (int i = 0; i < R; i++) {
            fp[i] = np[i];
            fb[i] = nb[i];
        }
        if (STORE) {
            col += RS;
#pragma unroll
            for (int i = 0; i < R; i++) {
                col[lane * R + i] = fp[i];
                col[64 * R + lane * R + i] = fb[i];
            }
        }
    }
    // must finish in the final position
    const int last = npos - 1;
    if (lane == last / R && a.cost) {
        float v = fp[0];
#pragma unroll
        for (int i = 1; i < R; i++)
            if (i == last % R) v = fp[i];
        a.cost[b] = -v;
    }
}

// ---------------------------------------------------------------------------------------------------
// backward sweep and gradient (c_squiggle_match.c:189-267, 591-694)
// ---------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64) void sq_backward_kernel(SqArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int npos = a.npos;
    const size_t ldp = (size_t)a.nbatch * 3;
    int64_t off;
    int n;
    if (!sq_read(a, b, off, n)) {
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int p = lane * R + i;
            if (p < npos)
                for (int k = 0; k < 3; k++) a.grad[(size_t)p * ldp + (size_t)b * 3 + k] = __int_as_float(0x7fc00000);
        }
        return;
    }
    SqTables<R> t;
    t.load(a, b, lane);
    const float lnhalf = logf(0.5f), lnpb = logf(a.prob_back);
    SqSignal sig;
    sig.init(a.signal + off, n);

    // move_pen of the position to the right (the move into it), and d move_pen / d logit as :664-667 has it
    float mpn[R], dl[R];
    const float mpr = wave_shift_down1(t.mpen[0], 0.0f);
#pragma unroll
    for (int i = 0; i < R; i++) {
        mpn[i] = i == R - 1 ? mpr : t.mpen[i + 1];
        const float m = sq_plogistic(t.mlogit[i]);
        dl[i] = (1.0f - a.prob_back) * m * (1.0f - m);
    }

    constexpr int RS = 2 * 64 * R;
    const float *lat = a.lattice + (size_t)(off + b) * RS;
    float bp[R], bb[R], g0[R], g1[R], g2[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        bp[i] = (lane * R + i == npos - 1) ? 0.0f : -SQ_LARGE;     // must end in the final position
        bb[i] = -SQ_LARGE;
        g0[i] = g1[i] = g2[i] = 0.0f;
    }
    // forward columns in flight: step s reads pos + back of column s and pos of column s - 1;
    // the loads for the next two steps are issued ahead
    float fps[R], fbs[R], fpp[R], fb1[R], fp1[R], fb2[R], fp2[R];
    auto ld = [&](float (&d)[R], int s, int half) {
        const float *q = lat + (size_t)(s < 0 ? 0 : s) * RS + half * 64 * R + lane * R;
#pragma unroll
        for (int i = 0; i < R; i++) d[i] = q[i];
    };
    ld(fps, n, 0);
    ld(fbs, n, 1);
    ld(fpp, n - 1, 0);
    ld(fb1, n - 1, 1);
    ld(fp1, n - 2, 0);
    ld(fb2, n - 2, 1);
    ld(fp2, n - 3, 0);

    for (int s = n; s >= 1; s--) {
        const float x = sig.at(s - 1, lane);
        float em[R];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < R; i++) {
            em[i] = sq_loglaplace(x, t.loc[i], t.sc[i], t.logsc[i]);
            mx = fmaxf(mx, fmaxf(fps[i] + bp[i], fbs[i] + bb[i]));
        }
        // fact: logsumexp over every state of f[s] + b[s] (:632-637)
        mx = wave_allmax_dpp(mx);
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < R; i++)
            sum += fast_exp2((fps[i] + bp[i] - mx) * LOG2E) + fast_exp2((fbs[i] + bb[i] - mx) * LOG2E);
        sum = wave_allsum(sum);
        const float fact = mx + fast_log2(sum) * LN2;

        const float fpl = wave_shift_up1(fpp[R - 1], -SQ_LARGE);
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int p = lane * R + i;
            // level and log-scale: posterior of the position and its back state (:639-655)
            const float w = fast_exp2((fps[i] + bp[i] - fact) * LOG2E) + fast_exp2((fbs[i] + bb[i] - fact) * LOG2E);
            const float sgn = (float)((x > t.loc[i]) - (x < t.loc[i]));
            g0[i] += w * (sgn / t.sc[i]);
            g1[i] += w * (fabsf(x - t.loc[i]) / t.sc[i] - 1.0f);
            // move logit, as :657-686 write it: f[s-1] + b[s] + emission, no transition penalty in the exponent
            const float prevp = i == 0 ? fpl : fpp[i - 1];
            const float stay = fast_exp2((fpp[i] + bp[i] + em[i] - fact) * LOG2E);
            const float move = p >= 1 ? fast_exp2((prevp + bp[i] + em[i] - fact) * LOG2E) : 0.0f;
            g2[i] += (move - stay) * dl[i];
        }

        // b[s-1] from b[s] (:222-257)
        float tp[R], tq[R];
#pragma unroll
        for (int i = 0; i < R; i++) {
            tp[i] = bp[i] + em[i];
            tq[i] = bb[i] + em[i];
        }
        const float tpr = wave_shift_down1(tp[0], -SQ_LARGE);
        const float tql = wave_shift_up1(tq[R - 1], -SQ_LARGE);
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int p = lane * R + i;
            const float nextp = i == R - 1 ? tpr : tp[i + 1];
            const float prevq = i == 0 ? tql : tq[i - 1];
            float v = tp[i] + t.spen[i];                                    // stay
            if (p + 1 < npos) v = sq_lse(v, nextp + mpn[i]);                // move on
            float w = tq[i] + lnhalf;                                       // stay in back
            if (p + 1 < npos) w = sq_lse(w, nextp + lnhalf);                // move out of back
            if (p >= 1) v = sq_lse(v, prevq + lnpb);                        // move into back
            bp[i] = p < npos ? v : -SQ_LARGE;
            bb[i] = p < npos ? w : -SQ_LARGE;
        }
        // rotate the forward columns and issue the loads for step s - 3
#pragma unroll
        for (int i = 0; i < R; i++) {
            fps[i] = fpp[i];
            fbs[i] = fb1[i];
            fpp[i] = fp1[i];
            fb1[i] = fb2[i];
            fp1[i] = fp2[i];
        }
        ld(fb2, s - 3, 1);
        ld(fp2, s - 4, 0);
    }
#pragma unroll
    for (int i = 0; i < R; i++) {
        const int p = lane * R + i;
        if (p < npos) {
            float *g = a.grad + (size_t)p * ldp + (size_t)b * 3;
            g[0] = -g0[i];
            g[1] = -g1[i];
            g[2] = -g2[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Viterbi path (c_squiggle_match.c:270-454)
// ---------------------------------------------------------------------------------------------------
// Order key of an end-state candidate: larger score first, then the earlier candidate (strict '>' in
// the reference's order: stay, move from the last position, then from position o = 0 .. npos-2).
__device__ __forceinline__ uint64_t sq_key(float v, uint32_t order) {
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (0xffffffffu - order);
}

__device__ __forceinline__ uint64_t sq_key_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <int CTRL>
__device__ __forceinline__ uint64_t sq_dpp_u64(uint64_t x) {
    const int lo = __builtin_amdgcn_update_dpp((int)(uint32_t)x, (int)(uint32_t)x, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(uint32_t)(x >> 32), (int)(uint32_t)(x >> 32), CTRL, 0xF, 0xF, false);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

__device__ __forceinline__ uint64_t sq_readlane_u64(uint64_t x, int l) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)x, l);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// max over the wave, uniform result (butterflies inside each 16-lane row, then the four rows)
__device__ __forceinline__ uint64_t sq_wave_max_u64(uint64_t x) {
    x = sq_key_max(x, sq_dpp_u64<0xB1>(x));
    x = sq_key_max(x, sq_dpp_u64<0x4E>(x));
    x = sq_key_max(x, sq_dpp_u64<0x141>(x));
    x = sq_key_max(x, sq_dpp_u64<0x140>(x));
    return sq_key_max(sq_key_max(sq_readlane_u64(x, 0), sq_readlane_u64(x, 16)),
                      sq_key_max(sq_readlane_u64(x, 32), sq_readlane_u64(x, 48)));
}

// traceback byte of a position k: bits 0-1 how its position state was entered (0 stay, 1 move from
// k - 1 (the start state for k = 0), 2 jump from the start, 3 out of the back state of k - 1);
// bit 2 how its back state was entered (0 stay, 1 from position k + 1).
// end-state traceback: -1 stay, otherwise the position it came from.
// States of the walk: k in [0, npos) positions, npos + k back states, -1 start, -2 end.
template <int R>
__global__ __launch_bounds__(64) void sq_viterbi_kernel(SqArgs a) {
    __shared__ uint32_t rows[SQ_TB_ROWS * 16 * R];
    __shared__ int32_t endrows[SQ_TB_ROWS];
    __shared__ int32_t outrows[SQ_TB_ROWS];
    const int b = blockIdx.x, lane = threadIdx.x;
    int64_t off;
    int n;
    if (!sq_read(a, b, off, n)) {
        if (lane == 0) a.cost[b] = __int_as_float(0x7fc00000);
        return;
    }
    const int npos = a.npos;
    SqTables<R> t;
    t.load(a, b, lane);
    const float lnhalf = logf(0.5f), lnpb = logf(a.prob_back);
    const float localpen = a.localpen, minscore = a.minscore;
    SqSignal sig;
    sig.init(a.signal + off, n);

    // mean move / stay penalties of the start and end states (:291-309): sequential float sums
    float mean_move, mean_stay;
    {
        float *pen = reinterpret_cast<float *>(rows);       // (rows is free until the walk)
#pragma unroll
        for (int i = 0; i < R; i++) {
            pen[lane * R + i] = t.mpen[i];
            pen[64 * R + lane * R + i] = t.spen[i];
        }
        __syncthreads();
        float sm = 0.0f, ss = 0.0f;
        for (int p = 0; p < npos; p++) {
            sm += pen[p];
            ss += pen[64 * R + p];
        }
        mean_move = sm / (float)npos;
        mean_stay = ss / (float)npos;
        __syncthreads();
    }
    // move penalty of the state to the left (the move out of it into this position)
    float mpl[R];
    {
        const float l = wave_shift_up1(t.mpen[R - 1], mean_move);
#pragma unroll
        for (int i = 0; i < R; i++) mpl[i] = i == 0 ? l : t.mpen[i - 1];
    }

    float vp[R], vb[R];
#pragma unroll
    for (int i = 0; i < R; i++) vp[i] = vb[i] = -SQ_LARGE;
    float vs = 0.0f, ve = -SQ_LARGE;        // must begin in the start state
    constexpr int TBW = 64 * R;             // traceback bytes per sample
    uint8_t *tb = a.tb + (size_t)off * TBW;
    int32_t *endtb = a.endtb + off;

    for (int s = 0; s < n; s++) {
        const float x = sig.at(s, lane);
        const float pl = wave_shift_up1(vp[R - 1], vs);
        const float bl = wave_shift_up1(vb[R - 1], -SQ_LARGE);
        const float pr = wave_shift_down1(vp[0], -SQ_LARGE);
        const float from_start = vs + mean_move;
        // end state (:337-368): stay, move from the last position, then from each position o < npos-1
        uint64_t ekey = 0;
        float np[R], nb[R];
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int p = lane * R + i;
            const float prevp = i == 0 ? pl : vp[i - 1];
            const float prevb = i == 0 ? bl : vb[i - 1];
            const float nextp = i == R - 1 ? pr : vp[i + 1];
            float v = vp[i] + t.spen[i];
            uint32_t code = 0;
            const float mv = prevp + mpl[i];
            if (mv > v) { v = mv; code = 1; }
            if (p >= 1) {
                const float js = from_start - localpen * (float)p;
                if (js > v) { v = js; code = 2; }
            }
            float w = vb[i] + lnhalf;
            if (p + 1 < npos) {
                const float bk = nextp + lnpb;
                if (bk > w) { w = bk; code |= 4; }
            }
            if (p >= 1) {
                const float ob = prevb + lnhalf;
                if (ob > v) { v = ob; code = (code & 4) | 3; }
            }
            if (p < npos) {
                const float em = fmaxf(-minscore, sq_loglaplace(x, t.loc[i], t.sc[i], t.logsc[i]));
                // into the end state from here
                const float es = vp[i] + t.mpen[i];
                if (p == npos - 1) {
                    ekey = sq_key_max(ekey, sq_key(es, 1u));
                } else {
                    ekey = sq_key_max(ekey, sq_key(es - localpen * (float)(npos - 1 - p), 2u + (uint32_t)p));
                }
                np[i] = v + em;
                nb[i] = w + em;
                tb[(size_t)s * TBW + p] = (uint8_t)code;
            } else {
                np[i] = nb[i] = -SQ_LARGE;
            }
        }
        ekey = sq_wave_max_u64(ekey);
        const float estay = ve + mean_stay;
        const float ebest = __uint_as_float((uint32_t)(ekey >> 32) & 0x80000000u ? (uint32_t)(ekey >> 32) & 0x7fffffffu
                                                                                  : ~(uint32_t)(ekey >> 32));
        const uint32_t eorder = 0xffffffffu - (uint32_t)ekey;
        int32_t etb = -1;
        float enew = estay;
        if (ebest > estay) {
            enew = ebest;
            etb = eorder == 1u ? npos - 1 : (int32_t)(eorder - 2u);
        }
        if (lane == 0) endtb[s] = etb;
        ve = enew - localpen;
        vs = (vs + mean_stay) - localpen;
#pragma unroll
        for (int i = 0; i < R; i++) {
            vp[i] = np[i];
            vb[i] = nb[i];
        }
    }

    // best final state: the last position or the end state (:407-415)
    const int last = npos - 1;
    float vlast = vp[0];
#pragma unroll
    for (int i = 1; i < R; i++)
        if (i == last % R) vlast = vp[i];
    vlast = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vlast), last / R));
    if (lane == 0) a.cost[b] = -fmaxf(vlast, ve);
    int cur = vlast > ve ? last : -2;

    // walk the traceback back, SQ_TB_ROWS samples at a time staged in LDS (:417-448)
    __syncthreads();        // (the traceback rows of this wave are visible to all its lanes)
    int32_t *path = a.path + off;
    for (int hi = n - 1; hi >= 0; hi -= SQ_TB_ROWS) {
        const int lo = hi - SQ_TB_ROWS + 1 < 0 ? 0 : hi - SQ_TB_ROWS + 1;
        const int nrow = hi - lo + 1;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(tb + (size_t)lo * TBW);
        for (int k = lane; k < nrow * 16 * R; k += 64) rows[k] = src[k];
        if (lane < nrow) endrows[lane] = endtb[lo + lane];
        __syncthreads();
        if (lane == 0) {
            const uint8_t *r8 = reinterpret_cast<const uint8_t *>(rows);
            for (int s = hi; s >= lo; s--) {
                outrows[s - lo] = cur < 0 ? -1 : (cur >= npos ? cur - npos : cur);
                if (s == 0) break;
                // the state at sample s - 1: how `cur` was entered at sample s
                if (cur == -2) {
                    const int e = endrows[s - lo];
                    cur = e < 0 ? -2 : e;
                } else if (cur >= npos) {
                    const int k = cur - npos;
                    if (r8[(s - lo) * TBW + k] & 4) cur = k + 1;
                } else if (cur >= 0) {
                    const int c = r8[(s - lo) * TBW + cur] & 3;
                    if (c == 1) cur = cur - 1;          // (-1 = start for position 0)
                    else if (c == 2) cur = -1;
                    else if (c == 3) cur = npos + cur - 1;
                }
            }
        }
        __syncthreads();
        if (lane < nrow) path[lo + lane] = outrows[lane];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int sq_positions_per_lane(size_t npos) {
    static const int rs[] = {1, 2, 4, 5, 8, 12, 16};
    for (int r : rs)
        if (npos <= (size_t)64 * r) return r;
    return 0;
}

size_t sq_lattice_bytes(size_t npos, size_t nbatch, size_t nsignal) {
    const int R = sq_positions_per_lane(npos);
    return R ? (nsignal + nbatch) * 2 * 64 * (size_t)R * sizeof(float) : 0;
}

size_t sq_path_bytes(size_t npos, size_t nsignal) {
    const int R = sq_positions_per_lane(npos);
    return R ? nsignal * (64 * (size_t)R + sizeof(int32_t)) + 16 : 0;
}

template <int R>
static int sq_launch(int which, const SqArgs &a, hipStream_t stream) {
    const dim3 grid(a.nbatch), block(64);
    if (which == 0) hipLaunchKernelGGL((sq_forward_kernel<R, false>), grid, block, 0, stream, a);
    else if (which == 1) hipLaunchKernelGGL((sq_forward_kernel<R, true>), grid, block, 0, stream, a);
    else if (which == 2) hipLaunchKernelGGL(sq_backward_kernel<R>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(sq_viterbi_kernel<R>, grid, block, 0, stream, a);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

// which: 0 cost, 1 cost + stored lattice, 2 backward over a stored lattice, 3 Viterbi
int squiggle_dispatch(int which, const SqArgs &a, hipStream_t stream) {
    switch (sq_positions_per_lane((size_t)a.npos)) {
    case 1: return sq_launch<1>(which, a, stream);
    case 2: return sq_launch<2>(which, a, stream);
    case 4: return sq_launch<4>(which, a, stream);
    case 5: return sq_launch<5>(which, a, stream);
    case 8: return sq_launch<8>(which, a, stream);
    case 12: return sq_launch<12>(which, a, stream);
    case 16: return sq_launch<16>(which, a, stream);
    default: return TK_ERR_UNSUPPORTED;
    }
}

}  // namespace tk

// beam_search.h -- the hash beam search's device code (the method: beam_kernels.hip's opening comment): hashes, the
// table-driven log-sum-exp, the restatement of the reference's sort procedure and the ONE kernel body, which two
// entry points instantiate:
//   tk_flipflop_beamsearch_dev   (beam_kernels.hip)   BeamArgs:       a dense (T, N, S) tensor, one T for every read
//   tk_basecall_beamsearch_dev   (basecall_beam.hip)  BeamPackedArgs: reads of different lengths, packed row after row
// The per-read geometry -- score base and row stride, T, workspace and output offsets -- is the only difference; it is
// resolved once at the top of the kernel (`Args::read`).  The tables (BEAM_TAB and its constants) are defined by
// beam_kernels.hip, where tests/test_host_logic.py holds them against their generator: a file that includes this header
// includes that one first (basecall_beam.hip does so with TK_BEAM_TABLES_ONLY).
#pragma once
#include "ff_common.h"

#ifndef TK_BEAM_TABLES_DEFINED
#error "beam_search.h: include beam_kernels.hip first (with TK_BEAM_TABLES_ONLY outside that file): it defines BEAM_TAB and its constants"
#endif

namespace tk {

constexpr int BEAM_MAXW = 12;

__device__ __forceinline__ unsigned long long beam_mix(unsigned long long h) {
    h ^= h >> 23;
    h *= 0x2127599bf4325c37ULL;
    h ^= h >> 47;
    return h;
}
// fasthash.c:95-103
__device__ __forceinline__ unsigned long long beam_chain(unsigned long long h, unsigned long long v) {
    h ^= beam_mix(v);
    h *= 0x880355f21e6d1965ULL;
    return beam_mix(h);
}

// tables into LDS (per-lane look-ups; a wave's own DS instructions execute in order)
__device__ __forceinline__ void beam_load_tables(double *tab, int lane) {
    for (int i = lane; i < TAB_N; i += WAVE) tab[i] = BEAM_TAB[i];
    wave_lds_fence();
}
__device__ __forceinline__ float beam_expf_neg(float a, const double *tab) {
    const double x = -(double)a;
    const double nf = __builtin_rint(x * INV_LN2_32);
    double r = __builtin_fma(nf, -LN2_32_HI, x);
    r = __builtin_fma(nf, -LN2_32_LO, r);
    const int n = (int)nf;
    const double scale = tab[TAB_EXP2 + (n & 31)];
    double p = 1.0 / 720.0;
    p = __builtin_fma(p, r, 1.0 / 120.0);
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return (float)__builtin_ldexp(scale * p, n >> 5);
}
__device__ __forceinline__ float beam_log1pf_unit(float e, const double *tab) {
    const double t = 1.0 + (double)e;
    const int i = (int)__builtin_rint((t - 1.0) * 64.0);
    const double r = __builtin_fma(t, tab[TAB_INVC + i], -1.0);
    double q = 1.0 / 7.0;
    q = __builtin_fma(q, -r, 1.0 / 6.0);
    q = __builtin_fma(q, -r, 1.0 / 5.0);
    q = __builtin_fma(q, -r, 1.0 / 4.0);
    q = __builtin_fma(q, -r, 1.0 / 3.0);
    q = __builtin_fma(q, -r, 0.5);
    q = __builtin_fma(q, -r, 1.0);
    return (float)__builtin_fma(q, r, tab[TAB_LOGC + i]);
}
// c_hashdecode.c:50-54
__device__ __forceinline__ float beam_lse(float x, float y, const double *tab) {
    const float absdif = fabsf(x - y);
    // (clamped argument: both functions run unconditionally, a lane outside the range drops the result)
    const float tail = beam_log1pf_unit(beam_expf_neg(fminf(absdif, 17.0f), tab), tab);
    return fmaxf(x, y) + ((absdif < 17.0f) ? tail : 0.0f);
}
__device__ __forceinline__ float rdl(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float bpf(float v, int l) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(l * 4, __float_as_int(v)));
}
__device__ __forceinline__ int bpi(int v, int l) { return __builtin_amdgcn_ds_bpermute(l * 4, v); }

// The sort procedure of taiyaki/decodeutil/qsort.h:39-186 with LESS(i, j) = key[i] > key[j]
// (c_hashdecode.c:156-158), on n <= 64 records: median of (second, middle, last), Sedgewick
// partition, insertion sort below 16 records, the smaller subfile first -- the same comparisons
// and exchanges in the same order, so equal keys end where the reference leaves them.
// The records live ACROSS THE LANES of two registers (lane p = position p) and the whole wave runs
// the procedure with uniform control flow: an element access is a v_readlane / v_writelane (a few
// cycles, the indices are scalars), not a 100-cycle LDS round trip from one lane -- the first version
// ran this on lane 0 over LDS arrays and a block with a tie (1-3 % of them) cost ~100 us, more than
// all the other blocks together.  The subfile stack sits in the lanes of a third / fourth register.
__device__ __forceinline__ void beam_qsort_lanes(float &keyv, int &idv, int n, int lane) {
    // (v_writelane has no builtin in this hipcc: a compare + select on the lane id does the same)
    auto wrl = [&](int val, int at, int old) { return lane == at ? val : old; };
    auto K = [&](int i) { return rdl(keyv, i); };
    auto less = [&](int i, int j) { return K(i) > K(j); };
    auto swap = [&](int i, int j) {
        const int ki = __builtin_amdgcn_readlane(__float_as_int(keyv), i);
        const int kj = __builtin_amdgcn_readlane(__float_as_int(keyv), j);
        const int ti = __builtin_amdgcn_readlane(idv, i), tj = __builtin_amdgcn_readlane(idv, j);
        int kv = __float_as_int(keyv);
        kv = wrl(kj, i, kv);
        kv = wrl(ki, j, kv);
        keyv = __int_as_float(kv);
        idv = wrl(tj, i, idv);
        idv = wrl(ti, j, idv);
    };
    if (n <= 1) return;
    int lo = 0, hi = n - 1, sp = 0;
    int st_lo = 0, st_hi = 0;                       // lane s = stack slot s
    while (true) {
        if (hi - lo + 1 >= 16) {
            const int m = lo + ((hi - lo) >> 1);
            const int a1 = lo + 1, a2 = m, a3 = hi;
            if (less(a2, a1)) {
                if (less(a3, a2)) swap(a1, a3);
                else {
                    swap(a1, a2);
                    if (less(a3, a2)) swap(a2, a3);
                }
            } else if (less(a3, a2)) {
                swap(a2, a3);
                if (less(a2, a1)) swap(a1, a2);
            }
            swap(lo, m);
            int i = lo + 1, j = hi;
            while (true) {
                do ++i; while (less(i, lo));
                do --j; while (less(lo, j));
                if (i >= j) break;
                swap(i, j);
            }
            i = j + 1;
            swap(lo, j);
            --j;
            int bl, bh, sl, sh;
            if (j - lo >= hi - i) { bl = lo; bh = j; sl = i; sh = hi; }
            else { bl = i; bh = hi; sl = lo; sh = j; }
            if (sl == sh) { lo = bl; hi = bh; }
            else {
                st_lo = wrl(bl, sp, st_lo);
                st_hi = wrl(bh, sp, st_hi);
                ++sp;
                lo = sl;
                hi = sh;
            }
        } else {
            for (int q = lo + 1; q <= hi; ++q)
                for (int k = q; k > lo && less(k, k - 1); --k) swap(k, k - 1);
            if (sp == 0) break;
            --sp;
            lo = __builtin_amdgcn_readlane(st_lo, sp);
            hi = __builtin_amdgcn_readlane(st_hi, sp);
        }
    }
}

// one read's geometry: all that differs between the dense and the packed form of the search
struct BeamRead {
    const float *sc;            // its first score row
    size_t rowstride;           // floats between two of its rows
    int T;
    float *bwd;                 // workspace [T + 1][2 nbase]
    unsigned char *bp;          // workspace [T][16]
    signed char *seq;           // out: its states
};

struct BeamArgs {
    const float *scores;        // (T, N, S)
    int T, N, nbase;
    int width;                  // max_beam_width
    float logcut;               // log(beam_cut); -inf = no cutting
    int guided;
    float *bwd;                 // workspace [N][T + 1][2 nbase]
    unsigned char *bp;          // workspace [N][T][16]: (parent slot << 4) | (appended state + 1)
    signed char *seq;           // out (N, T): flip-flop states, -1 padded
    int *seqlen;                // out (N)
    float *score;               // out (N)
    int lds_rows;               // rows of the back-pointer table kept in LDS (0: walk global memory)

    static constexpr bool PACKED = false;
    __device__ __forceinline__ BeamRead read(int n, int ns, int S) const {
        return {scores + (size_t)n * S, (size_t)N * S, T, bwd + (size_t)n * (T + 1) * ns, bp + (size_t)n * T * 16,
                seq + (size_t)n * T};
    }
};

// Reads of different lengths in one launch: the scores packed row after row (row stride S), read n's rows from
// row_off[n], nrows[n] of them (a device-side count: the stitch kernel writes it), in a room of row_off[n + 1] -
// row_off[n].  `T`, `N` of the base are not read.  Workspace and outputs sit at the same prefix offsets: bwd rows from
// row_off[n] + n (a read has T + 1 of them), back-pointer rows, states and call characters from row_off[n].
struct BeamPackedArgs : BeamArgs {
    const int64_t *row_off;     // (nread + 1)
    const int32_t *nrows;       // (nread)
    int64_t total_rows;         // rows of `scores`: bounds every read
    unsigned char *call;        // out: alphabet[state % nbase] of every state after the first that differs from its predecessor
    int *calllen;               // out (nread)
    uint32_t alphabet;          // the character of base b in bits [8 b, 8 b + 8) (nbase <= 4)
    uint32_t *status;           // nullable; `status_bit` is OR-ed in where row_off does not fit total_rows
    uint32_t status_bit;

    static constexpr bool PACKED = true;
    __device__ __forceinline__ BeamRead read(int n, int ns, int S) const {
        const int64_t lo = row_off[n], room = row_off[n + 1] - lo;
        const bool fits = lo >= 0 && room >= 0 && room <= 0x7fffffff && lo + room <= total_rows;
        if (!fits && status && threadIdx.x == 0) atomicOr(status, status_bit);
        const int64_t first = fits ? lo : 0;
        const int T = fits ? (int)min((int64_t)max(nrows[n], 0), room) : 0;
        return {scores + (size_t)first * S, (size_t)S, T, bwd + (size_t)(first + n) * ns, bp + (size_t)first * 16,
                seq + (size_t)first};
    }
};

// what both dispatchers admit (decodeutil.beamsearch's rule: one candidate record per lane), as their result code
inline int beam_admit(size_t nbase, int width, float beam_cut) {
    if (nbase < 1 || nbase > 4 || width < 1 || width > BEAM_MAXW || (size_t)width * (nbase + 1) > WAVE) return 2;
    if (!(beam_cut >= 0.f) || beam_cut > 1.f) return 1;
    return 0;
}
inline float beam_logcut(float beam_cut) { return beam_cut > 0.f ? logf(beam_cut) : -__builtin_huge_valf(); }
constexpr size_t BEAM_LDS_ROWS = 3584;      // back-pointer rows kept in LDS: 56 KiB of dynamic LDS at most

// NBT: the alphabet size as a compile-time constant (4: DNA / RNA, everything the reference ships) so that
// the loops over bases unroll and their gathers leave the serial chains; 0: read it from the arguments.
// Args: BeamArgs or BeamPackedArgs (above).
template <int NBT, class Args>
__global__ __launch_bounds__(WAVE) void beam_kernel(Args a) {
    extern __shared__ unsigned char lds_bp[];           // [lds_rows][16]
    __shared__ unsigned long long nh[16];
    __shared__ float nsc[16];
    __shared__ int nlast[16], nbp[16];
    __shared__ float qkey[WAVE];
    __shared__ int qid[WAVE], qrank[WAVE];
    __shared__ double tab[TAB_N];
    const int n = blockIdx.x, lane = threadIdx.x;
    beam_load_tables(tab, lane);
    const int nb = NBT ? NBT : a.nbase, ns = 2 * nb, S = ns * (nb + 1);
    const BeamRead g = a.read(n, ns, S);
    const int T = g.T;
    const size_t rowstride = g.rowstride;
    const float *sc = g.sc;
    float *bwd = g.bwd;
    unsigned char *bpn = g.bp;
    const int col = min(lane, S - 1);
    if constexpr (Args::PACKED) {
        if (T <= 0) {                                   // a read without rows: no states, no call, score 0
            if (lane == 0) {
                a.seqlen[n] = 0;
                a.calllen[n] = 0;
                a.score[n] = 0.f;
            }
            return;
        }
    }

    // ---- guiding backward pass (c_flipflopfwdbwd.c:55-91): lane = from-state ----------------
    if (lane < ns) bwd[(size_t)T * ns + lane] = 0.f;
    // (score rows are requested PF blocks ahead of their use: a block is a serial chain of nbase + 1
    // log-sum-exps, and a load issued where it is needed adds a memory round trip to every one)
    constexpr int PF = 4;
    auto load_row = [&](int blk) { return sc[(size_t)min(max(blk, 0), T - 1) * rowstride + col]; };
    if (a.guided) {
        float p = 0.f;                                  // pbwd[lane]
        float cur[PF], nxt[PF];
#pragma unroll
        for (int q = 0; q < PF; ++q) cur[q] = load_row(T - 1 - q);
        for (int b0 = T; b0 > 0; b0 -= PF) {
#pragma unroll
            for (int q = 0; q < PF; ++q) nxt[q] = load_row(b0 - 1 - PF - q);
#pragma unroll
            for (int q = 0; q < PF; ++q) {
                const int blk = b0 - q;
                if (blk <= 0) break;
                const float row = cur[q];
                const int fr = min(lane, ns - 1);
                // to the flop of this state's base
                float c = bpf(row, ns * nb + fr) + bpf(p, nb + fr % nb);
                float term[NBT ? NBT : 1];
                if constexpr (NBT != 0) {
#pragma unroll
                    for (int to = 0; to < NBT; ++to) term[to] = bpf(row, to * ns + fr) + rdl(p, to);
#pragma unroll
                    for (int to = 0; to < NBT; ++to) c = beam_lse(c, term[to], tab);
                } else {
                    for (int to = 0; to < nb; ++to) c = beam_lse(c, bpf(row, to * ns + fr) + rdl(p, to), tab);
                }
                p = c;
                if (lane < ns) bwd[(size_t)(blk - 1) * ns + lane] = c;
            }
#pragma unroll
            for (int q = 0; q < PF; ++q) cur[q] = nxt[q];
        }
    } else {
        for (int i = lane; i < T * ns; i += WAVE) bwd[i] = 0.f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();

    // ---- beam search --------------------------------------------------------------------
    // beam element i in lane i.  (The workgroup is ONE wavefront: its LDS instructions execute in order, so
    // the hand-offs through LDS below need no s_barrier -- and must not have __syncthreads(), whose
    // s_waitcnt vmcnt(0) would wait for the block's back-pointer store and the prefetched rows every time.)
    unsigned long long eh = beam_chain(0x880355f21e6d1965ULL, (unsigned long long)min(lane, nb - 1));
    float es = 0.f;
    int el = min(lane, nb - 1);
    int W = nb;
    auto load_bwd = [&](int blk) { return bwd[(size_t)min(blk + 1, T) * ns + min(lane, ns - 1)]; };
    float rowc[PF], bsvc[PF], rown[PF], bsvn[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) {
        rowc[q] = load_row(q);
        bsvc[q] = load_bwd(q);
    }
    for (int b0 = 0; b0 < T; b0 += PF) {
      // (this group's rows and backward scores were requested a group ago)
#pragma unroll
      for (int q = 0; q < PF; ++q) {
          rown[q] = load_row(b0 + PF + q);
          bsvn[q] = load_bwd(b0 + PF + q);
      }
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int blk = b0 + q;
        if (blk >= T) break;
        const float row = rowc[q];
        const float bsv = (lane < ns) ? bsvc[q] : 0.f;                                  // bwdscore[lane]
        const int next = W * nb, ncand = next + W;
        // candidate of this lane
        const bool is_ext = lane < next, is_cand = lane < ncand;
        const int i = is_ext ? lane / nb : min(max(lane - next, 0), W - 1);
        const int base = lane % nb;
        const unsigned pl = (unsigned)i;
        const float pscore = bpf(es, pl);
        const int plast = bpi(el, pl);
        const unsigned hlo = (unsigned)bpi((int)(unsigned)eh, pl), hhi = (unsigned)bpi((int)(unsigned)(eh >> 32), pl);
        const unsigned long long phash = ((unsigned long long)hhi << 32) | hlo;
        const int newstate = is_ext ? ((base != plast) ? base : plast + nb) : plast;
        const int tidx = plast + ns * min(newstate, nb);       // MOVE_IDX / STAY_IDX
        const float bnew = bpf(bsv, newstate);              // bwdscore[new last state]
        float cscore = (pscore + bpf(row, tidx)) + bnew;
        const unsigned long long chash = is_ext ? beam_chain(phash, (unsigned long long)newstate) : phash;
        bool valid = is_cand;
        if (a.logcut > -1e30f) {
            // lower bound from the best element (c_hashdecode.c:385-396), then the running maximum
            // over the records BEFORE this one in candidate order
            const int pb = __builtin_amdgcn_readlane(el, 0);
            float mx = rdl(row, nb * ns + pb) + rdl(bsv, pb < nb ? pb + nb : pb);
            for (int k = 0; k < nb; ++k) mx = fmaxf(mx, rdl(row, k * ns + pb) + rdl(bsv, k));
            mx += rdl(es, 0);
            float run = is_cand ? cscore : -__builtin_huge_valf();
            // inclusive prefix max over lanes, then shift by one lane
            for (int d = 1; d < WAVE; d <<= 1) {
                const float o = bpf(run, max(lane - d, 0));
                if (lane >= d) run = fmaxf(run, o);
            }
            float before = bpf(run, max(lane - 1, 0));
            if (lane == 0) before = -__builtin_huge_valf();
            valid = valid && !(cscore < fmaxf(mx, before) + a.logcut);
        }
        // ---- merge records with the same hash (= the same sequence).  The only pairs there can be
        //      are (extension of s[:-1] by its last base, stay of s): two extensions with the same
        //      sequence would have the same parent, two stays are two beam elements.  So the W stay
        //      records are broadcast one by one and the extension lanes compare -- W steps, not W (nbase + 1).
        int partner = -1;
        for (int j = next; j < ncand; ++j) {
            const unsigned jlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)chash, j);
            const unsigned jhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(chash >> 32), j);
            const bool jvalid = __builtin_amdgcn_readlane((int)valid, j) != 0;
            const bool hit = jvalid && valid && is_ext && jlo == (unsigned)chash && jhi == (unsigned)(chash >> 32);
            const unsigned long long hits = __builtin_amdgcn_ballot_w64(hit);
            if (hit) partner = j;                                   // the extension: keeps the record
            if (lane == j && hits != 0ull) partner = __builtin_ctzll(hits);     // the stay: folds into it
        }
        const float pscore2 = bpf(cscore, max(partner, 0));
        bool uniq = valid;
        if (valid && partner >= 0) {
            if (partner > lane) cscore = beam_lse(pscore2, cscore, tab);     // keep the earlier record
            else uniq = false;
        }
        // ---- rank among the unique records by score: every lane counts the records that beat its own
        //      and those that equal it (itself included).  Records that are not in the running -- merged
        //      away, cut, lanes past the candidates -- carry -inf and beat nobody, so the sweep needs no
        //      validity test and may run past the last candidate (four records per trip).
        const float rs = uniq ? cscore : -__builtin_huge_valf();
        const int nuniq = __builtin_popcountll(__builtin_amdgcn_ballot_w64(uniq));
        int rank = 0, same = 0;
        for (int j0 = 0; j0 < ncand; j0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float js = rdl(rs, j0 + u);                   // (ncand <= 60: lanes 60 .. 63 hold -inf)
                rank += (js > rs) ? 1 : 0;
                same += (js == rs) ? 1 : 0;
            }
        }
        const bool tie = uniq && same > 1;
        if (__builtin_amdgcn_ballot_w64(tie) != 0ull) {
            // equal scores: the reference's order.  Its score sort starts from the records in
            // descending hash order (c_hashdecode.c:440), a merged pair as (sum, -inf).
            int hpos = (valid && !uniq) ? 1 : 0;
            for (int j = 0; j < ncand; ++j) {
                const unsigned jlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)chash, j);
                const unsigned jhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(chash >> 32), j);
                const bool jvalid = __builtin_amdgcn_readlane((int)valid, j) != 0;
                hpos += (jvalid && (((unsigned long long)jhi << 32) | jlo) > chash) ? 1 : 0;
            }
            const int nrec = __builtin_popcountll(__builtin_amdgcn_ballot_w64(valid));
            if (valid) {
                qkey[hpos] = uniq ? cscore : -__builtin_huge_valf();
                qid[hpos] = lane;
            }
            wave_lds_fence();
            float keyv = qkey[min(lane, max(nrec - 1, 0))];
            int idv = qid[min(lane, max(nrec - 1, 0))];
            beam_qsort_lanes(keyv, idv, nrec, lane);
            if (lane < nrec) qrank[idv] = lane;
            wave_lds_fence();
            if (valid) rank = qrank[lane];
        }
        const int newW = min(a.width, nuniq);              // c_hashdecode.c:474
        if (uniq && rank < newW) {
            nh[rank] = chash;
            nsc[rank] = cscore - bnew;                      // remove the backward contribution (:485)
            nlast[rank] = newstate;
            nbp[rank] = (i << 4) | (is_ext ? newstate + 1 : 0);
        }
        wave_lds_fence();
        if (lane < newW) {
            eh = nh[lane];
            es = nsc[lane];
            el = nlast[lane];
            const unsigned char b = (unsigned char)nbp[lane];
            if (blk < a.lds_rows) lds_bp[blk * 16 + lane] = b;
            bpn[(size_t)blk * 16 + lane] = b;
        }
        W = newW;
        wave_lds_fence();
      }
#pragma unroll
      for (int q = 0; q < PF; ++q) {
          rowc[q] = rown[q];
          bsvc[q] = bsvn[q];
      }
    }
    // ---- walk the best element's sequence back -----------------------------------------------
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // (the back-pointer stores of every lane, once)
    __syncthreads();
    if (lane == 0) {
        a.score[n] = es;
        int slot = 0, len = 1;
        for (int blk = T - 1; blk >= 0; --blk) {
            const unsigned char b = (blk < a.lds_rows) ? lds_bp[blk * 16 + slot] : bpn[(size_t)blk * 16 + slot];
            len += (b & 15) ? 1 : 0;
            slot = b >> 4;
        }
        const int first = slot;                             // the initial one-state sequence
        signed char *out = g.seq;
        const int keep = min(len, T);                       // (the reference's buffer holds nblock states)
        a.seqlen[n] = keep;
        slot = 0;
        int pos = len - 1;
        for (int blk = T - 1; blk >= 0; --blk) {
            const unsigned char b = (blk < a.lds_rows) ? lds_bp[blk * 16 + slot] : bpn[(size_t)blk * 16 + slot];
            if (b & 15) {
                if (pos < T) out[pos] = (signed char)((b & 15) - 1);
                --pos;
            }
            slot = b >> 4;
        }
        if (T > 0) out[0] = (signed char)first;
        if constexpr (Args::PACKED) nbp[0] = keep;          // (for the other lanes, below)
        else
            for (int k = keep; k < T; ++k) out[k] = -1;     // the dense (N, T) output is -1 padded
    }
    if constexpr (Args::PACKED) {
        // ---- the call (flipflopfings.py:94-97, include_first_source=False): the whole wave over the states
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (lane 0's states, for the other lanes)
        __syncthreads();
        const int keep = nbp[0];
        unsigned char *call = a.call + (g.seq - a.seq);
        int count = 0;
        for (int k0 = 1; k0 < keep; k0 += WAVE) {
            const int k = min(k0 + lane, keep - 1);
            const int s = g.seq[k], p = g.seq[k - 1];
            const bool move = k0 + lane < keep && s != p;
            const unsigned long long moves = __builtin_amdgcn_ballot_w64(move);
            if (move) call[count + __builtin_popcountll(moves & ((1ull << lane) - 1ull))] = (unsigned char)(a.alphabet >> (8 * (s % nb)));
            count += __builtin_popcountll(moves);
        }
        if (lane == 0) a.calllen[n] = count;
    }
}

}  // namespace tk

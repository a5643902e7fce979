// include/taiyaki_amd_align.h: unit-cost global alignment of a batch of (query, reference) pairs, one wavefront per pair.
//
// A cell is ONE 32-bit key, D in the upper half and 65535 - M in the lower, so the lexicographic minimum of (D, -M) is
// v_min_u32: a non-match column adds INC = 1 << 16, a match column subtracts 1.  Sums saturate (v_add_u32 clamp), so the
// all-ones key is an absorbing "no cell" and nothing wraps below TK_ALIGN_MAX_LEN.
//
// A row of the band is laid out by DIAGONAL: cell k of row i is column j = i + first + k, so a cell's diagonal
// predecessor is cell k of the row before and its upper one cell k + 1; the band's edges stay where they are and only
// the reference slides, one code per row.  Lane l owns the C consecutive cells l C .. l C + C - 1:
//   1. a[k] = min(prev[k] + (match ? -1 : INC), prev[k + 1] + INC)                    independent per cell
//   2. the left neighbour, cur[k] = min(a[k], cur[k - 1] + INC), is a prefix minimum once k INC is taken out: a serial
//      chain over the lane's own C cells, then a six-step DPP scan of the lanes' last cells in which every step adds
//      the INC of the cells it jumps (no subtraction, so the saturation holds), then one min per cell with the carry.
// C = 1, 2, 4, 8, 16: prev, a and the lane's C reference codes are registers (the codes shift down a cell per row, the
// next lane's first comes in by DPP, lane 63's from a 64-row block that all lanes fetched together one block ahead; the
// row's query code is read from such a block too).  Wider bands: the row is in LDS, C odd (bank-conflict free), the
// codes come from memory (L1: consecutive rows read the same lines).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/taiyaki_amd_align.h"

namespace tk {

constexpr uint32_t KEY_NONE = 0xFFFFFFFFu, INC = 0x10000u;
constexpr int LDS_TILE = 8;
constexpr int NO_QUERY = 0x200, NO_REF = 0x100;     // codes outside a sequence: equal to nothing

__host__ __device__ inline int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t imax64(int64_t a, int64_t b) { return a > b ? a : b; }

// the band of (m, n, t), clipped to the diagonals that cross the matrix; false: t in 0 .. |n - m| - 1, no diagonal
__host__ __device__ inline bool band_of(int64_t m, int64_t n, int64_t t, int64_t *first, int64_t *last) {
    if (t < 0) {
        *first = -m, *last = n;
        return true;
    }
    const int64_t diff = n > m ? n - m : m - n;
    if (t < diff) return false;
    const int64_t p = (t - diff) / 2;
    *first = imax64(-m, imin64(0, n - m) - p);
    *last = imin64(n, imax64(0, n - m) + p);
    return true;
}

__host__ __device__ inline int cells_per_lane(int64_t width) {
    const int64_t c = (width + 63) / 64;
    return c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : c <= 8 ? 8 : c <= 16 ? 16 : (int)(c | 1);
}

__device__ __forceinline__ uint32_t sat(uint32_t x, uint32_t inc) { return __builtin_elementwise_add_sat(x, inc); }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// lanes without a source (and rows outside ROWMASK) read "no cell"
template <int CTRL, int ROWMASK = 0xF>
__device__ __forceinline__ uint32_t dpp_or_none(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)KEY_NONE, (int)x, CTRL, ROWMASK, 0xF, false);
}

// last: the lane's last cell with nothing coming in from the left.  Returns the finished cell to the left of the
// lane's first one (lane 0: none): min over the lanes l' below of last[l'] + (distance in cells) INC.  ci = C INC.
__device__ __forceinline__ uint32_t carry_scan(uint32_t last, uint32_t ci, int lane) {
    uint32_t y = last;
    y = umin(y, sat(dpp_or_none<0x111>(y), ci));            // row_shr:1
    y = umin(y, sat(dpp_or_none<0x112>(y), 2 * ci));        // row_shr:2
    y = umin(y, sat(dpp_or_none<0x114>(y), 4 * ci));        // row_shr:4
    y = umin(y, sat(dpp_or_none<0x118>(y), 8 * ci));        // row_shr:8
    y = umin(y, sat(dpp_or_none<0x142, 0xA>(y), (uint32_t)((lane & 15) + 1) * ci));     // row_bcast:15 -> rows 1, 3
    y = umin(y, sat(dpp_or_none<0x143, 0xC>(y), (uint32_t)(lane - 31) * ci));           // row_bcast:31 -> rows 2, 3
    return dpp_or_none<0x138>(y);                           // wave_shr:1
}

struct ByteCodes {
    const uint8_t *p;
    __device__ __forceinline__ int at(int64_t i, int len, int none) const { return i >= 0 && i < len ? (int)p[i] : none; }
};
struct LabelCodes {     // the loss's labels: flip-flop codes, the base is code % nbase
    const int32_t *p;
    uint32_t nbase;
    __device__ __forceinline__ int at(int64_t i, int len, int none) const {
        return i >= 0 && i < len ? (int)((uint32_t)p[i] % nbase) : none;
    }
};

// The query's code of row i (q[i - 1]) and, for the register sweep, the reference code that enters lane 63 after row i:
// 64 rows per block, lane t holds row 64 b + 1 + t's, the next block is fetched while this one is used.
template <class Q, class R>
struct Feed {
    int q_now, q_next, r_now, r_next;
    int64_t r_at;       // reference index of lane 0's code in block 0
    __device__ __forceinline__ void start(const Q &q, const R &r, int m, int n, int64_t r0, int lane) {
        r_at = r0;
        q_now = q.at(lane, m, NO_QUERY), q_next = q.at(64 + lane, m, NO_QUERY);
        r_now = r.at(r_at + lane, n, NO_REF), r_next = r.at(r_at + 64 + lane, n, NO_REF);
    }
    __device__ __forceinline__ void turn(const Q &q, const R &r, int m, int n, int i, int lane) {     // at i = 64 b + 1, b > 0
        q_now = q_next, r_now = r_next;
        q_next = q.at((int64_t)i - 1 + 64 + lane, m, NO_QUERY);
        r_next = r.at(r_at + i - 1 + 64 + lane, n, NO_REF);
    }
};

__device__ __forceinline__ uint32_t row0_key(int64_t j) { return ((uint32_t)j << 16) | 0xFFFFu; }

// The register sweep: returns the key of cell (m, n).  first: the band's first diagonal, width: its diagonals (<= 64 C).
template <int C, class Q, class R>
__device__ uint32_t sweep_registers(const Q &q, const R &r, int m, int n, int first, int width, int lane) {
    uint32_t prev[C], a[C];
    int code[C];
    const int k0 = lane * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int k = k0 + c, j = first + k;
        prev[c] = k < width && j >= 0 ? row0_key(j) : KEY_NONE;
        code[c] = r.at(j, n, NO_REF);           // row 1: cell k is column 1 + first + k, code r[first + k]
    }
    Feed<Q, R> feed;
    feed.start(q, r, m, n, (int64_t)first + 64 * C, lane);      // after row i lane 63 takes r[i + first + 64 C - 1]
    for (int i = 1; i <= m; ++i) {
        const int t = (i - 1) & 63;
        if (t == 0 && i > 1) feed.turn(q, r, m, n, i, lane);
        const int qi = __builtin_amdgcn_readlane(feed.q_now, t);
        const uint32_t up_next = dpp_or_none<0x130>(prev[0]);   // wave_shl:1: the next lane's first cell
        uint32_t x = KEY_NONE;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int k = k0 + c, j = i + first + k;
            const uint32_t up = c + 1 < C ? prev[c + 1] : up_next;
            const uint32_t dg = code[c] == qi ? prev[c] - 1u : sat(prev[c], INC);
            uint32_t v = umin(dg, sat(up, INC));
            v = j < 0 || k >= width ? KEY_NONE : v;
            v = j == 0 ? row0_key(i) : v;
            x = umin(v, sat(x, INC));
            a[c] = x;
        }
        const uint32_t carry = carry_scan(x, (uint32_t)C * INC, lane);
#pragma unroll
        for (int c = 0; c < C; ++c) prev[c] = k0 + c < width ? umin(a[c], sat(carry, (uint32_t)(c + 1) * INC)) : KEY_NONE;
        const int code_next = (int)dpp_or_none<0x130>((uint32_t)code[0]);
        const int code_in = __builtin_amdgcn_readlane(feed.r_now, t);
#pragma unroll
        for (int c = 0; c + 1 < C; ++c) code[c] = code[c + 1];
        code[C - 1] = lane == 63 ? code_in : code_next;
    }
    const int kf = n - m - first;
    uint32_t v = prev[0];
#pragma unroll
    for (int c = 1; c < C; ++c) v = c == kf % C ? prev[c] : v;
    return (uint32_t)__shfl((int)v, kf / C);
}

// The LDS sweep: row (64 C cells, C odd) holds the band's row, updated in place.
template <class Q, class R>
__device__ uint32_t sweep_lds(const Q &q, const R &r, int m, int n, int first, int width, int C, uint32_t *row, int lane) {
    const int k0 = lane * C;
    for (int c = 0; c < C; ++c) {
        const int k = k0 + c, j = first + k;
        row[k] = k < width && j >= 0 ? row0_key(j) : KEY_NONE;
    }
    Feed<Q, R> feed;
    feed.start(q, r, m, n, 0, lane);
    __syncthreads();
    for (int i = 1; i <= m; ++i) {
        const int t = (i - 1) & 63;
        if (t == 0 && i > 1) feed.turn(q, r, m, n, i, lane);
        const int qi = __builtin_amdgcn_readlane(feed.q_now, t);
        const uint32_t up_next = lane < 63 ? row[k0 + C] : KEY_NONE;    // read before its owner replaces it
        __syncthreads();
        uint32_t x = KEY_NONE, dgp = row[k0];
        const int64_t r0 = (int64_t)i + first + k0 - 1;
        // tiles of LDS_TILE cells: a tile's codes and upper cells are fetched together, then its chain runs
        for (int c0 = 0; c0 < C; c0 += LDS_TILE) {
            int code[LDS_TILE];
            uint32_t up[LDS_TILE];
#pragma unroll
            for (int u = 0; u < LDS_TILE; ++u) {
                const int c = c0 + u;
                code[u] = c < C ? r.at(r0 + c, n, NO_REF) : NO_REF;
                up[u] = c + 1 < C ? row[k0 + c + 1] : up_next;
            }
#pragma unroll
            for (int u = 0; u < LDS_TILE; ++u) {
                const int c = c0 + u, k = k0 + c, j = i + first + k;
                if (c < C) {
                    const uint32_t dg = code[u] == qi ? dgp - 1u : sat(dgp, INC);
                    uint32_t v = umin(dg, sat(up[u], INC));
                    v = j < 0 || k >= width ? KEY_NONE : v;
                    v = j == 0 ? row0_key(i) : v;
                    x = umin(v, sat(x, INC));
                    row[k] = k < width ? x : KEY_NONE;
                    dgp = up[u];
                }
            }
        }
        const uint32_t carry = carry_scan(x, (uint32_t)C * INC, lane);
        if (carry != KEY_NONE) {
            for (int c0 = 0; c0 < C; c0 += LDS_TILE) {
                uint32_t cell[LDS_TILE];
#pragma unroll
                for (int u = 0; u < LDS_TILE; ++u) cell[u] = c0 + u < C ? row[k0 + c0 + u] : KEY_NONE;
#pragma unroll
                for (int u = 0; u < LDS_TILE; ++u) {
                    const int c = c0 + u;
                    if (c < C && k0 + c < width) row[k0 + c] = umin(cell[u], sat(carry, (uint32_t)(c + 1) * INC));
                }
            }
        }
        __syncthreads();
    }
    return row[n - m - first];
}

// One pair, whole wave.  cap: the cells of `row` (0: none).  Writes the three words from lane 0; returns `exact`, the
// same in every lane.
template <class Q, class R>
__device__ bool align_one(const Q &q, const R &r, int64_t m64, int64_t n64, int t, uint32_t *row, int cap,
                          int32_t *distance, int32_t *matches, int32_t *exact) {
    const int lane = threadIdx.x;
    const int64_t longest = imax64(m64, n64);
    int64_t first = 0, last = 0;
    const bool swept = longest <= TK_ALIGN_MAX_LEN && band_of(m64, n64, t, &first, &last) &&
                       last - first + 1 <= imax64(cap, TK_ALIGN_REG_BAND);
    if (!swept) {       // (uniform: reported, not swept)
        if (lane == 0) *distance = (int32_t)imin64(longest, INT32_MAX), *matches = 0, *exact = 0;
        return false;
    }
    const int m = (int)m64, n = (int)n64, f = (int)first, width = (int)(last - first + 1);
    uint32_t key;
    switch (cells_per_lane(width)) {
    case 1: key = sweep_registers<1>(q, r, m, n, f, width, lane); break;
    case 2: key = sweep_registers<2>(q, r, m, n, f, width, lane); break;
    case 4: key = sweep_registers<4>(q, r, m, n, f, width, lane); break;
    case 8: key = sweep_registers<8>(q, r, m, n, f, width, lane); break;
    case 16: key = sweep_registers<16>(q, r, m, n, f, width, lane); break;
    default: key = sweep_lds(q, r, m, n, f, width, cells_per_lane(width), row, lane);
    }
    const int32_t d = (int32_t)(key >> 16);
    const bool holds = t < 0 || d <= t;
    if (lane == 0) *distance = d, *matches = (int32_t)(0xFFFFu - (key & 0xFFFFu)), *exact = holds;
    return holds;
}

__global__ __launch_bounds__(64) void align_pairs_kernel(const uint8_t *query, const int64_t *q_off, const uint8_t *ref,
                                                         const int64_t *r_off, const int32_t *pairs,
                                                         const int32_t *max_distance, int shared,
                                                         int cap, int32_t *distance, int32_t *matches, int32_t *exact) {
    extern __shared__ uint32_t lds[];
    const size_t pair = pairs ? (size_t)pairs[blockIdx.x] : (size_t)blockIdx.x;
    const int64_t qb = q_off[pair], rb = r_off[pair];
    const int64_t m = imax64(q_off[pair + 1] - qb, 0), n = imax64(r_off[pair + 1] - rb, 0);
    align_one(ByteCodes{query + qb}, ByteCodes{ref + rb}, m, n, max_distance ? max_distance[pair] : shared, lds, cap,
              distance + pair, matches + pair, exact + pair);
}

// Column `blockIdx.x`: collapse its path into LDS (a ballot per 64 states, as the basecaller's call kernel) and align it
// against the column's labels.  The answer is that of every diagonal, but a call that is close to its labels does not pay
// for them: the wave sweeps the band of max_distance |n - m| + max(16, min(m, n) / 16) and doubles it until the band
// holds the answer (its D <= max_distance), at the last with every diagonal.  A good call costs a band of a hundred
// diagonals, a call that has nothing to do with its labels less than twice the whole table.
__global__ __launch_bounds__(64) void align_calls_kernel(const int64_t *path, const int32_t *lengths, int nblk,
                                                         int64_t nbatch, uint32_t nbase, const int32_t *seqs,
                                                         const int64_t *seq_off, const int32_t *seqlens, int cap,
                                                         int32_t *distance, int32_t *matches, int32_t *exact) {
    extern __shared__ uint32_t lds[];
    uint8_t *call = reinterpret_cast<uint8_t *>(lds);
    uint32_t *row = lds + TK_ALIGN_MAX_CALL / 4;
    const int64_t col = blockIdx.x;
    const int lane = threadIdx.x;
    int len = lengths ? lengths[col] : nblk;
    len = len < 0 ? 0 : len > nblk ? nblk : len;
    int ncall = 0;
    for (int base = 0; base <= len; base += 64) {
        const int s = base + lane;
        bool move = false;
        int64_t state = 0;
        if (s <= len) {
            state = path[(int64_t)s * nbatch + col];
            move = s == 0 || state != path[(int64_t)(s - 1) * nbatch + col];
        }
        const unsigned long long moved = __ballot(move);
        if (move) call[ncall + __popcll(moved & ((1ull << lane) - 1ull))] = (uint8_t)((uint64_t)state % nbase);
        ncall += __popcll(moved);
    }
    __syncthreads();
    const int64_t n = imax64(seqlens[col], 0), longest = imax64(n, ncall);
    for (int64_t t = longest - imin64(n, ncall) + imax64(16, imin64(n, ncall) / 16);; t *= 2) {
        const int td = t >= longest ? -1 : (int)t;          // max(m, n) holds every alignment: all diagonals
        if (align_one(ByteCodes{call}, LabelCodes{seqs + seq_off[col], nbase}, ncall, n, td, row, cap, distance + col,
                      matches + col, exact + col) || td < 0)
            break;
    }
}

// the LDS row of a launch whose widest band is `cells`: none for the register sweeps
static size_t row_bytes(size_t cells) {
    return cells <= TK_ALIGN_REG_BAND ? 0 : (size_t)64 * cells_per_lane((int64_t)cells) * sizeof(uint32_t);
}

}  // namespace tk

static int launched() { return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH; }

extern "C" {

int tk_align_band(size_t m, size_t n, int max_distance, int *first, int *last, int *cells) {
    if (!first || !last || !cells) return TK_ERR_BAD_ARG;
    if (m > TK_ALIGN_MAX_LEN || n > TK_ALIGN_MAX_LEN) return TK_ERR_UNSUPPORTED;
    int64_t lo = 1, hi = 0;
    if (!tk::band_of((int64_t)m, (int64_t)n, max_distance, &lo, &hi)) {
        *first = 1, *last = 0, *cells = 0;
        return TK_OK;
    }
    if (hi - lo + 1 > TK_ALIGN_MAX_BAND) return TK_ERR_UNSUPPORTED;
    *first = (int)lo, *last = (int)hi, *cells = tk::cells_per_lane(hi - lo + 1);
    return TK_OK;
}

int tk_align_pairs_dev(const uint8_t *query, const int64_t *q_off, const uint8_t *ref, const int64_t *r_off,
                       size_t npair, const int32_t *pairs, const int32_t *max_distance, int shared_max_distance,
                       size_t band_cells, int32_t *distance, int32_t *matches, int32_t *exact, void *stream) {
    if (npair == 0) return TK_OK;
    if (!query || !q_off || !ref || !r_off || !distance || !matches || !exact) return TK_ERR_BAD_ARG;
    if (npair > (size_t)INT32_MAX || band_cells > TK_ALIGN_MAX_BAND) return TK_ERR_UNSUPPORTED;
    const size_t cap = band_cells ? band_cells : TK_ALIGN_MAX_BAND;
    hipLaunchKernelGGL(tk::align_pairs_kernel, dim3((unsigned)npair), dim3(64), tk::row_bytes(cap),
                       static_cast<hipStream_t>(stream), query, q_off, ref, r_off, pairs, max_distance, shared_max_distance,
                       (int)cap, distance, matches, exact);
    return launched();
}

int tk_align_calls_dev(const int64_t *path, const int32_t *lengths, size_t nblk, size_t nbatch, size_t nbase,
                       const int32_t *seqs, const int64_t *seq_off, const int32_t *seqlens, size_t band_cells,
                       int32_t *distance, int32_t *matches, int32_t *exact, void *stream) {
    if (nbatch == 0) return TK_OK;
    if (!path || !seq_off || !seqlens || !distance || !matches || !exact) return TK_ERR_BAD_ARG;
    if (nbatch > (size_t)INT32_MAX || nblk + 1 > TK_ALIGN_MAX_CALL || nbase == 0 || nbase > 127 ||
        band_cells > TK_ALIGN_MAX_CALL_BAND)
        return TK_ERR_UNSUPPORTED;
    const size_t cap = band_cells ? band_cells : TK_ALIGN_MAX_CALL_BAND;
    hipLaunchKernelGGL(tk::align_calls_kernel, dim3((unsigned)nbatch), dim3(64), TK_ALIGN_MAX_CALL + tk::row_bytes(cap),
                       static_cast<hipStream_t>(stream), path, lengths, (int)nblk, (int64_t)nbatch, (uint32_t)nbase,
                       seqs, seq_off, seqlens, (int)cap, distance, matches, exact);
    return launched();
}

}  // extern "C"

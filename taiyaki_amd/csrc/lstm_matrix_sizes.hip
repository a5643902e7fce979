// lstm_matrix_sizes.hip -- the forward recurrence of layers.Lstm that saves nothing (gate order i, f, g, o; h0 = c0 = 0)
// at H = 384 and 192, the sizes of the 48-unit family of the main library, on the gfx950 matrix cores
// (include/taiyaki_amd_lstm_matrix_sizes.h; libtaiyaki_amd_lstm_matrix_sizes.so).  384 is the reference trainer's default
// --size.  The operator, the row order, the order of the sums, the granule and the contract of lengths and direction are
// those of lstm_matrix_group.hip (H = 256), which keeps its bits in its own library; this is a kernel of its own, a
// template over the size and the column sets, that shares rnn_common.h and wgrad_common.h with it and nothing else.
//
// Geometry.  A group is G = H / 32 workgroups (12 at 384, 6 at 192) of 256 lanes (4 waves, one per SIMD) and shares
// C = 16 M batch columns, M sets of the instruction's 16.  Member g owns the units 32 g ... 32 g + 31 with all four
// gates: 128 rows of W_hh as 8 row tiles of 16, 2 per wave.  Row 4 q + i of tile j of wave w is gate i of unit
// 32 g + 8 w + 4 j + q.  Lane l of A holds row l % 16 at k = 8 (l / 16) ... + 7 of a 32-wide k-block, lane l of B column
// l % 16 at the same k, accumulator register r of lane l is row 4 (l / 16) + r of column l % 16.  So a lane's four
// accumulator registers of (set, tile j) are the four gates of ONE (unit, column) pair: the cell update runs in the lane
// and c stays in registers for the launch (2 M cells per lane).  A member's 32 units are exactly one k-block: k-block kb
// of the h image is what member kb published.
//
// Weights.  Loaded once, split with split2 and kept: 2 tiles x (H / 32) k-blocks x 3 parts x 4 = 288 VGPRs per lane at
// 384, 144 at 192.  __launch_bounds__(256) is one wave per SIMD and the whole budget of 512 registers; no instantiation
// uses scratch (profiles/r55_lstm_matrix_sizes_resource_usage.txt).  To stay there at 384 the lane keeps no table of its
// granule pairs: their places are recomputed from the lane's number and the member's every step (pair_at).
//
// Products.  An accumulator starts as gx and takes, k-block by k-block, W1 h1, W1 h2, W2 h1, W1 h3, W3 h1, W2 h2.  Every
// column of the instruction and every set is treated alike: a column's y is a function of its gx, its length and W_hh
// alone, not of N, the other columns, its place in the group, M, the slab or the CU count.
//
// h between members: an all-to-all per step.  The producer splits its new h once.  A granule is 8 bytes, one (unit,
// column): the three bf16 parts in bits 0-47 and the tag 1 + s % 65535 in bits 48-63, written by ONE agent-scope relaxed
// store and polled by agent-scope relaxed loads until the tag matches (rnn_common.h: the data is the flag).  Two slots by
// step parity, zeroed in front of every launch.  Layout [slot][group][member][column][unit of 32]: a consumer lane reads
// the two granules of an adjacent pair of units (16 bytes) of each of the G - 1 other members, (G - 1) M pairs per lane
// and step (11 at 384), and writes three 4-byte words, one per part, into the LDS image hb[parity][part][column][k].  A
// member's own units go straight from the cell lanes to the image.  A column of the image is H + 8 bf16: 49 chunks of
// 16 bytes at 384 and 25 at 192, both odd, so a B fragment is one conflict-free 16-byte read.
// The tag is never 0, what a zeroed slot holds.  A slot of parity p holds only what the steps of that parity wrote, in
// order, and no member publishes step s + 2 before every member has read step s (it needs step s + 1 of every member,
// which each published behind its own read of step s).  So a poll for step s finds 0, the granule of step s - 2 or that
// of step s; tag(s) = tag(s - 2) would need 2 = 0 mod 65535.  The tag may wrap: nblk has no bound of its own.
// Every spin is bounded by the clock budget (kSpinTicks); on expiry TK_STATUS_RNN_TIMEOUT is OR-ed into *status and the
// whole grid leaves.
//
// Schedule of step s (nothing bound for HBM is issued in front of a poll in the same step).
//   poll: the other members' h of step s - 1 into hb[s & 1];
//   right behind it the gx rows of step s + 1 are asked for, whole 128-byte pieces with 16 bytes per lane, 2 M per lane;
//   barrier (the only one of the step);
//   the y rows of step s - 1 leave from ys[(s - 1) & 1] as whole 128-byte pieces;
//   accumulators from gs[s & 1], 18 H / 48 MFMAs per wave and set (144 at 384, 72 at 192), cell update, h to ys[s & 1],
//   its parts to hb[(s + 1) & 1] and to the granules of slot s & 1; the gx rows that arrived go to gs[(s + 1) & 1].
// A column of the gx block is 132 floats (4 mod 64 banks: the 16 columns x 4 units of a wave's 4-byte read are 64
// banks), of the y block 36 (the same argument).  gx is not __restrict__ (DESIGN.md "LSTM inference at size 96 on the
// matrix cores").
//
// Column sets and LDS.  (12 (H + 8) + 1344) x 16 M bytes: 94.5 KB at 384 with M = 1, where M = 2 (189 KB) is past the
// 160 KB of a workgroup and is NOT built; 58.5 KB and 117 KB at 192, both built.
//
// Lengths and tails.  At t >= lengths[n] the lane writes y = 0 and hands on h = c = 0 through a select behind the cell
// update: a NaN in gx there stays in that step's accumulators.  A column of the last group at or beyond N has length
// 0, loads column N - 1 and stores nothing; it still publishes, because the members wait for each other.
//
// Admission and slabs.  All members of all groups must be resident: groups x G <= cu_count, one workgroup per CU.  A
// wider batch runs inside the entry as slabs of (cu_count / G) C columns, launch behind launch on the caller's stream, in
// place on windows of columns (LD, the tensors' columns per time step, is a kernel argument), the granules zeroed in
// front of each.  place() keeps a group inside one XCD only where the grid is a multiple of 8 G workgroups: at 384 on 256
// CUs a full slab is 21 groups, which is not.  Whether 16 groups per slab would be ahead there is not measured.
#include "ff_common.h"          // TK_LAB_ENV
#include "wgrad_common.h"       // split2, bf16x8; dispatch.h
#include "rnn_common.h"         // the granule protocol's parts, place, sigmoidf, row_chunk, zero_ws

#include "../../include/taiyaki_amd_lstm_matrix_sizes.h"

namespace tk {
namespace {

constexpr int MS_U = 32;                // units of a member: one k-block
constexpr int MS_THREADS = 256;
constexpr int MS_TILES = 2;             // 16-row tiles of a wave: 8 units x 4 gates
constexpr int MS_GPITCH = 4 * MS_U + 4; // floats per column of the gx block
constexpr int MS_YPITCH = MS_U + 4;     // floats per column of the y block
constexpr int MS_LDS = 160 * 1024;      // what a workgroup can have

constexpr bool size_built(size_t H) { return H == 192 || H == 384; }
constexpr int members(size_t H) { return (int)(H / MS_U); }
constexpr size_t lds_bytes(size_t H, int m) { return (12 * (H + 8) + 8 * MS_GPITCH + 8 * MS_YPITCH) * 16 * (size_t)m; }
// the sets built at a size: what fits the LDS, M = 1 at 384 and M = 1, 2 at 192
constexpr int max_m(size_t H) { return lds_bytes(H, 2) + 64 <= MS_LDS ? 2 : 1; }
static_assert(max_m(384) == 1 && max_m(192) == 2, "M = 2 does not fit the LDS at 384");
// ... and the one the release build launches at 192: M = 2 was ahead of M = 1 in every turn at every width the route
// takes, 1024 ... 8192 (7.2 against 8.9 us per step of a layer at 1024, 60 against 68 at 8192); behind it at 256 and 512,
// which stay with the main library (profiles/r55_lstm_matrix_sizes.txt)
constexpr int MS_RELEASE_M_192 = 2;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

__host__ __device__ constexpr unsigned step_tag(int s) { return 1u + (unsigned)s % 65535u; }

// Pair i of a lane, i < (G - 1) M: units 2 p, 2 p + 1 (p = tid % 16) of column tid / 16 + 16 (i % M) of the member
// i / M + 1 places behind the lane's own.  `granule`: its first granule in a slot of the group; `word`: its 4-byte word
// in a part of an h image.
template <int H, int M>
__device__ __forceinline__ void pair_at(int i, int tid, int member, int &granule, int &word) {
    constexpr int G = H / MS_U, C = 16 * M, HP = H + 8;
    const int p = tid % 16, c = tid / 16 + 16 * (i % M);
    int mm = member + 1 + i / M;
    mm = mm >= G ? mm - G : mm;
    granule = (mm * C + c) * MS_U + 2 * p;
    word = (c * HP + MS_U * mm) / 2 + p;
}

// This lane's NP pairs of granules until every lane of the wave sees `tag` in all of its own; false when the clock
// budget runs out or another workgroup has already given up (rnn_common.h: sweep, with the tag in the granule's top 16
// bits).  Every pass issues all loads before it waits.
template <int H, int M, int NP>
__device__ __forceinline__ bool gather(const u64 *g, int tid, int member, unsigned tag, u64 (&a)[NP], u64 (&b)[NP],
                                       uint32_t *status) {
    const uint64_t start = __builtin_amdgcn_s_memrealtime();
    for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            int off, word;
            pair_at<H, M>(i, tid, member, off, word);
            a[i] = __hip_atomic_load((gu64 *)(g + off), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b[i] = __hip_atomic_load((gu64 *)(g + off + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) ok &= (unsigned)(a[i] >> 48) == tag && (unsigned)(b[i] >> 48) == tag;
        if (__all(ok)) return true;
        if ((spins & 31) == 31) {
            const uint32_t st = __hip_atomic_load((gu32 *)status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((st & TK_STATUS_RNN_TIMEOUT) || __builtin_amdgcn_s_memrealtime() - start > kSpinTicks) {
                __hip_atomic_fetch_or((gu32 *)status, TK_STATUS_RNN_TIMEOUT, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// N columns of this launch in tensors of LD columns per time step; the pointers stand at the launch's first column.
// hbuf: [2 slots][ngroups][G members][C columns][32 units] granules.
// (gx is not __restrict__: loads the compiler knows to be invariant are sunk through the step, each to its LDS write)
template <int H, int M>
__global__ __launch_bounds__(MS_THREADS) void lstm_matrix_sizes_kernel(const float *gx, const float *__restrict__ whh,
                                                                       int T, int N, int LD, int reverse,
                                                                       float *__restrict__ y,
                                                                       const int32_t *__restrict__ lengths, u64 *hbuf,
                                                                       int ngroups, uint32_t *status) {
    constexpr int H4 = 4 * H, C = 16 * M, G = H / MS_U, KB = H / 32, HP = H + 8;
    constexpr int GQ = C * MS_U / MS_THREADS;           // 16-byte chunks of gx per lane and step: 2 M
    constexpr int NP = (G - 1) * M;                     // pairs of granules per lane and step
    constexpr int SLOT = G * C * MS_U;                  // granules of a group's slot
    static_assert(H % 32 == 0 && (HP / 8) % 2 == 1, "a column of the image is an odd count of 16-byte chunks");
    static_assert(NP * MS_THREADS == (G - 1) * C * (MS_U / 2), "the lanes' pairs are the other members' units");
    __shared__ __attribute__((aligned(16))) unsigned short hb[2][3][C * HP];
    __shared__ __attribute__((aligned(16))) float gs[2][C * MS_GPITCH];
    __shared__ __attribute__((aligned(16))) float ys[2][C * MS_YPITCH];
    __shared__ int give_up;
    static_assert(sizeof(hb) + sizeof(gs) + sizeof(ys) == lds_bytes(H, M) && lds_bytes(H, M) + 64 <= MS_LDS, "LDS");

    int group, member;
    place(G, group, member);
    const int tid = threadIdx.x;
    const int wave = tid / 64, lane = tid % 64;
    const int col = lane % 16, quad = lane / 16;
    const int n0 = group * C;
    const int u0 = 8 * wave + quad;                     // the lane's cell of (set, tile j): unit u0 + 4 j of the member
    if (tid == 0) give_up = 0;

    // A: row lane % 16 of tile j is gate col % 4 of unit 32 member + 8 wave + 4 j + col / 4; k = 32 kb + 8 quad ... + 7
    bf16x8 wf[MS_TILES][KB][3];
#pragma unroll
    for (int j = 0; j < MS_TILES; ++j) {
        const float *row = whh + (size_t)((col % 4) * H + MS_U * member + 8 * wave + 4 * j + col / 4) * H + 8 * quad;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            // (w_hh needs no more than a float's alignment)
            const row_chunk a = *reinterpret_cast<const row_chunk *>(row + 32 * kb);
            const row_chunk b = *reinterpret_cast<const row_chunk *>(row + 32 * kb + 4);
            uint4 p1, p2, p3;
            split2(a.x, a.y, p1.x, p2.x, p3.x);
            split2(a.z, a.w, p1.y, p2.y, p3.y);
            split2(b.x, b.y, p1.z, p2.z, p3.z);
            split2(b.z, b.w, p1.w, p2.w, p3.w);
            wf[j][kb][0] = as_frag(p1);
            wf[j][kb][1] = as_frag(p2);
            wf[j][kb][2] = as_frag(p3);
        }
    }

    int len[M];
    float cst[M][MS_TILES];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int n = n0 + 16 * m + col;
        len[m] = n >= N ? 0 : lengths ? lengths[n] : T;
#pragma unroll
        for (int j = 0; j < MS_TILES; ++j) cst[m][j] = 0.f;
    }

    // the lane's chunks of a step's gx: chunk q is floats [4 (q % 8), + 4) of gate (q / 8) % 4 of column q / 32
    size_t goff[GQ];
    int gdst[GQ];
#pragma unroll
    for (int i = 0; i < GQ; ++i) {
        const int q = tid + i * MS_THREADS, c = q / 32, gate = (q / 8) % 4, ch = q % 8;
        const int nn = n0 + c < N ? n0 + c : N - 1;
        goff[i] = (size_t)nn * H4 + gate * H + MS_U * member + 4 * ch;
        gdst[i] = c * MS_GPITCH + gate * MS_U + 4 * ch;
    }
    // ... and its chunk of a step's y: floats [4 (tid % 8), + 4) of column tid / 8 (C 8 chunks: the lanes below that)
    const int yc = tid / 8;
    float *const ydst = yc < C && n0 + yc < N ? y + (size_t)(n0 + yc) * H + MS_U * member + 4 * (tid % 8) : nullptr;
    const int ysrc = (yc < C ? yc : 0) * MS_YPITCH + 4 * (tid % 8);
    const size_t gstep = (size_t)LD * H4, ystep = (size_t)LD * H;
    u64 *const slots = hbuf + (size_t)group * SLOT;         // slot p: + p * ngroups * SLOT
    const size_t slot_stride = (size_t)ngroups * SLOT;

    for (int i = tid; i < 3 * C * HP / 2; i += MS_THREADS) reinterpret_cast<uint32_t *>(hb[0][0])[i] = 0u;
    {
        const float *g = gx + (size_t)(reverse ? T - 1 : 0) * gstep;
#pragma unroll
        for (int i = 0; i < GQ; ++i)
            *reinterpret_cast<float4 *>(gs[0] + gdst[i]) = *reinterpret_cast<const float4 *>(g + goff[i]);
    }

    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        const int par = s & 1;
        if (s > 0) {
            u64 ga[NP], gb[NP];
            if (!gather<H, M, NP>(slots + (size_t)(par ^ 1) * slot_stride, tid, member, step_tag(s - 1), ga, gb, status))
                give_up = 1;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                int off, word;
                pair_at<H, M>(i, tid, member, off, word);
                const uint32_t alo = (uint32_t)ga[i], blo = (uint32_t)gb[i];
                const uint32_t ahi = (uint32_t)(ga[i] >> 32), bhi = (uint32_t)(gb[i] >> 32);
                reinterpret_cast<uint32_t *>(hb[par][0])[word] = (alo & 0xffffu) | (blo << 16);
                reinterpret_cast<uint32_t *>(hb[par][1])[word] = (alo >> 16) | (blo & 0xffff0000u);
                reinterpret_cast<uint32_t *>(hb[par][2])[word] = (ahi & 0xffffu) | (bhi << 16);
            }
        }
        // right behind the poll the rows of the next step are asked for (no branch: the last step asks for its own rows
        // again, and nothing reads them)
        f32x4 gn[GQ];
        const float *gnext = gx + (size_t)(s + 1 == T ? t : reverse ? t - 1 : t + 1) * gstep;
#pragma unroll
        for (int i = 0; i < GQ; ++i) gn[i] = *reinterpret_cast<const f32x4 *>(gnext + goff[i]);
        asm volatile("" ::: "memory");                   // the prefetch stays here
        __syncthreads();
        if (give_up) return;
        // behind the barrier the rows of the step before leave
        if (s > 0 && ydst) {
            const float4 v = *reinterpret_cast<const float4 *>(ys[par ^ 1] + ysrc);
            *reinterpret_cast<row_chunk *>(ydst + (size_t)(reverse ? t + 1 : t - 1) * ystep) = row_chunk{v.x, v.y, v.z, v.w};
        }

        f32x4 acc[M][MS_TILES];
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int j = 0; j < MS_TILES; ++j) {
                const float *g = gs[par] + (16 * m + col) * MS_GPITCH + u0 + 4 * j;
                acc[m][j] = f32x4{g[0], g[MS_U], g[2 * MS_U], g[3 * MS_U]};
            }
        // W1 h1, W1 h2, W2 h1, W1 h3, W3 h1, W2 h2, k-block by k-block; the sets and tiles innermost: 2 M independent
        // accumulators between two instructions on the same one
        constexpr int PW[6] = {0, 0, 1, 0, 2, 1}, PH[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            bf16x8 hf[M][3];
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    hf[m][p] = as_frag(*reinterpret_cast<const uint4 *>(hb[par][p] + (16 * m + col) * HP + 32 * kb + 8 * quad));
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int j = 0; j < MS_TILES; ++j)
                        acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][kb][PW[x]], hf[m][PH[x]], acc[m][j], 0, 0, 0);
        }

        u64 *const out = slots + (size_t)par * slot_stride;
        const u64 tag = (u64)step_tag(s) << 48;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float h[MS_TILES];
#pragma unroll
            for (int j = 0; j < MS_TILES; ++j) {
                const f32x4 a = acc[m][j];
                const float ig = sigmoidf(a[0]), fg = sigmoidf(a[1]), gg = tanhf(a[2]), og = sigmoidf(a[3]);
                cst[m][j] = fmaf(ig, gg, fg * cst[m][j]);
                h[j] = og * tanhf(cst[m][j]);
                if (t >= len[m]) cst[m][j] = h[j] = 0.f;
                ys[par][(16 * m + col) * MS_YPITCH + u0 + 4 * j] = h[j];
            }
            uint32_t p[3];
            split2(h[0], h[1], p[0], p[1], p[2]);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                unsigned short *at = hb[par ^ 1][q] + (16 * m + col) * HP + MS_U * member + u0;
                at[0] = (unsigned short)(p[q] & 0xffffu);
                at[4] = (unsigned short)(p[q] >> 16);
            }
            if (s + 1 < T) {                              // (nobody reads the last step's h)
                u64 *g = out + (member * C + 16 * m + col) * MS_U + u0;
                const u64 lo = (u64)((p[0] & 0xffffu) | (p[1] << 16)) | ((u64)(p[2] & 0xffffu) << 32) | tag;
                const u64 hi = (u64)((p[0] >> 16) | (p[1] & 0xffff0000u)) | ((u64)(p[2] >> 16) << 32) | tag;
                __hip_atomic_store((gu64 *)g, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store((gu64 *)(g + 4), hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int i = 0; i < GQ; ++i) *reinterpret_cast<f32x4 *>(gs[par ^ 1] + gdst[i]) = gn[i];
    }
    if (T > 0) {
        __syncthreads();
        if (ydst) {
            const float4 v = *reinterpret_cast<const float4 *>(ys[(T - 1) & 1] + ysrc);
            *reinterpret_cast<row_chunk *>(ydst + (size_t)(reverse ? 0 : T - 1) * ystep) = row_chunk{v.x, v.y, v.z, v.w};
        }
    }
}

// Column sets per group at a size.  The release build: 1 at 384 (all that fits), MS_RELEASE_M_192 at 192.  The lab
// build: TK_LAB_LSTM_MATRIX_SIZES_M = 1 or 2 in the environment, read at every call (tools/lstmmatrixsizesbench.py times
// every built M from one process), where the size has that M; else the same.
int release_m(size_t H) {
    const char *e = TK_LAB_ENV("TK_LAB_LSTM_MATRIX_SIZES_M");
    if (e && e[0] >= '1' && e[0] <= '0' + max_m(H) && !e[1]) return e[0] - '0';
    return H == 192 ? MS_RELEASE_M_192 : 1;
}

// both slots of one group
size_t group_bytes(size_t H, int m) { return (size_t)2 * members(H) * 16 * m * MS_U * sizeof(u64); }

size_t slab_columns(size_t H, int cu_count) {
    return size_built(H) && cu_count >= members(H) ? (size_t)(cu_count / members(H)) * 16 * release_m(H) : 0;
}

template <int H, int M>
void launch(int groups, hipStream_t st, const float *gx, const float *w_hh, int T, int n, int LD, int reverse, float *y,
            const int32_t *lengths, void *ws, uint32_t *status) {
    hipLaunchKernelGGL((lstm_matrix_sizes_kernel<H, M>), dim3((unsigned)(groups * (H / MS_U))), dim3(MS_THREADS), 0, st, gx,
                       w_hh, T, n, LD, reverse, y, lengths, static_cast<u64 *>(ws), groups, status);
}

}  // namespace
}  // namespace tk

extern "C" {

int tk_lstm_matrix_sizes_supported(size_t size) { return tk::size_built(size) ? 1 : 0; }

int tk_lstm_matrix_sizes_columns(size_t size) { return tk::size_built(size) ? 16 * tk::release_m(size) : 0; }

size_t tk_lstm_matrix_sizes_slab(size_t size, int cu_count) { return tk::slab_columns(size, cu_count); }

size_t tk_lstm_matrix_sizes_workspace_bytes(size_t nbatch, size_t size, int cu_count) {
    using namespace tk;
    const size_t S = slab_columns(size, cu_count);
    if (S == 0 || nbatch == 0) return 0;
    const size_t C = 16 * release_m(size), n = nbatch < S ? nbatch : S;
    return (n + C - 1) / C * group_bytes(size, release_m(size));
}

int tk_lstm_matrix_sizes_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk,
                                     size_t nbatch, size_t size, int reverse, int cu_count, float *y, void *workspace,
                                     size_t workspace_bytes, uint32_t *status, void *stream) {
    using namespace tk;
    if (!gx || !w_hh || !y || !aligned16(gx) || !aligned16(y) || nblk > (size_t)INT32_MAX || nbatch > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
    if (!workspace || !status || !aligned16(workspace)) return TK_ERR_BAD_ARG;
    if (!size_built(size) || nbatch == 0) return TK_ERR_UNSUPPORTED;
    const size_t S = slab_columns(size, cu_count);
    if (S == 0) return TK_ERR_UNSUPPORTED;
    if (workspace_bytes < tk_lstm_matrix_sizes_workspace_bytes(nbatch, size, cu_count)) return TK_ERR_WORKSPACE;
    if (nblk == 0) return TK_OK;
    const int m = release_m(size);
    const size_t C = 16 * m;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (size_t first = 0; first < nbatch; first += S) {
        const size_t n = nbatch - first < S ? nbatch - first : S;
        const int groups = (int)((n + C - 1) / C);
        const int rc = zero_ws(workspace, groups * group_bytes(size, m), st);
        if (rc != TK_OK) return rc;
        const float *g = gx + first * 4 * size;
        float *yy = y + first * size;
        const int32_t *ln = at_column(lengths, first, 1);
        if (size == 384)
            launch<384, 1>(groups, st, g, w_hh, (int)nblk, (int)n, (int)nbatch, reverse, yy, ln, workspace, status);
        else if (m == 2)
            launch<192, 2>(groups, st, g, w_hh, (int)nblk, (int)n, (int)nbatch, reverse, yy, ln, workspace, status);
        else
            launch<192, 1>(groups, st, g, w_hh, (int)nblk, (int)n, (int)nbatch, reverse, yy, ln, workspace, status);
        if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    }
    return TK_OK;
}

}  // extern "C"

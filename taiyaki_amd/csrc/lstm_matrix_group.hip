// lstm_matrix_group.hip -- the forward recurrence of layers.Lstm that saves nothing (gate order i, f, g, o; h0 = c0 = 0)
// at H = 256 on the gfx950 matrix cores, for batches of hundreds to thousands of columns
// (include/taiyaki_amd_lstm_matrix_group.h; libtaiyaki_amd_lstm_matrix_group.so).  The operator, the row order, the
// order of the sums and the contract of lengths and direction are those of lstm_matrix.hip (H = 96).  There one
// workgroup holds the whole split W_hh; at 256 that is 1.5 MB, so here a GROUP of workgroups holds it and hands h on
// through the tagged granules of rnn_common.h.
//
// Geometry as built.  A group is MG_G = 8 workgroups of 256 lanes (4 waves, one per SIMD) and shares C = 16 M batch
// columns, M = 1 or 2 sets of the instruction's 16 (a template parameter; MG_RELEASE_M is what the release build
// launches, the lab build takes M from the environment, see release_m).  Member g owns the units 32 g ... 32 g + 31 with
// all four gates: 128 rows of W_hh as 8 row tiles of 16, 2 per wave.  Row 4 q + i of tile j of wave w is gate i of unit
// 32 g + 8 w + 4 j + q.  Operands as in lstm_matrix.hip: lane l of A holds row l % 16 at k = 8 (l / 16) ... + 7 of a
// 32-wide k-block, lane l of B column l % 16 at the same k, accumulator register r of lane l is row 4 (l / 16) + r of
// column l % 16.  So a lane's four accumulator registers of (set, tile j) are the four gates of ONE (unit, column) pair:
// the cell update runs in the lane and c stays in registers for the launch (2 M cells per lane).
//
// Weights.  Loaded once, split with split2 and kept: 2 tiles x 8 k-blocks x 3 parts x 4 = 192 VGPRs per lane.
//
// Products.  An accumulator starts as gx and takes, k-block by k-block, W1 h1, W1 h2, W2 h1, W1 h3, W3 h1, W2 h2.  Every
// column of the instruction and every set is treated alike: a column's y is a function of its gx, its length and W_hh
// alone, not of N, the other columns, its place in the group, M or the CU count.
//
// h between members: an all-to-all per step.  The producer splits its new h once.  A granule is 8 bytes, one (unit,
// column): the three bf16 parts in bits 0-47 and a 16-bit tag in bits 48-63, written by ONE sc1 store and polled by sc1
// loads until the tag matches (rnn_common.h: the data is the flag).  Two slots by step parity, zeroed in front of every
// launch.  Layout [slot][group][member][column][unit of 32]: a consumer lane reads the two granules of an adjacent pair
// of units (16 bytes; a wave's 64 pairs are 1 KB in a row) and writes three 4-byte words, one per part, into the LDS
// image hb[parity][part][column][k].  No consumer splits anything, and the traffic is that of a float32 granule.  A
// member's own 32 units go straight from the cell lanes to the image.  A column of the image is MG_HPITCH = 264 bf16 =
// 33 chunks of 16 bytes, an odd number: a B fragment is one conflict-free 16-byte read.
// The tag of step s is 1 + s % 65535: never 0, what a zeroed slot holds.  A slot of parity p holds only what the steps
// of that parity wrote, in order, and no member publishes step s + 2 before every member has read step s (it needs
// step s + 1 of every member, which each published behind its own read of step s).  So a poll for step s finds 0, the
// granule of step s - 2 or that of step s; tag(s) = tag(s - 2) would need 2 = 0 mod 65535.  The tag may wrap: nblk
// has no bound of its own.
// Every spin is bounded by the clock budget (kSpinTicks); on expiry TK_STATUS_RNN_TIMEOUT is OR-ed into *status and the
// whole grid leaves.
//
// Schedule of step s (lstm_kernels.hip's rule: nothing bound for HBM is issued in front of a poll in the same step).
//   poll: the other members' h of step s - 1 into hb[s & 1];
//   right behind it the gx rows of step s + 1 are asked for, whole 128-byte pieces with 16 bytes per lane, 2 M per lane;
//   barrier (the only one of the step);
//   the y rows of step s - 1 leave from ys[(s - 1) & 1] as whole 128-byte pieces;
//   accumulators from gs[s & 1], 96 MFMAs per wave and set, cell update, h to ys[s & 1], its parts to hb[(s + 1) & 1]
//   and to the granules of slot s & 1; the gx rows that arrived go to gs[(s + 1) & 1].
// A column of the gx block is MG_GPITCH = 132 floats (4 mod 64 banks: the 16 columns x 4 units of a wave's 4-byte read
// are 64 banks), of the y block MG_YPITCH = 36 (36 mod 64, the same argument).  gx is not __restrict__ (DESIGN.md "LSTM
// inference at size 96 on the matrix cores").  With M = 2 both sets are gathered by one poll and run behind one barrier:
// the MFMAs of a set do NOT run under the gather of the next in this build.
//
// Lengths and tails.  At t >= lengths[n] the lane writes y = 0 and hands on h = c = 0 through a select behind the cell
// update: a NaN in gx there stays in that step's accumulators.  A column of the last group at or beyond N has length
// 0, loads column N - 1 and stores nothing; it still publishes, because the members wait for each other.
//
// Admission and slabs.  All members of all groups must be resident: groups x 8 <= cu_count, one workgroup per CU (LDS
// 70.5 KB at M = 1, 141 KB at M = 2).  A wider batch runs inside the entry as slabs of (cu_count / 8) C columns, launch
// behind launch on the caller's stream, in place on windows of columns (LD, the tensors' columns per time step, is a
// kernel argument), the granules zeroed in front of each.
#include "ff_common.h"          // TK_LAB_ENV
#include "wgrad_common.h"       // split2, bf16x8; dispatch.h
#include "rnn_common.h"         // the granule protocol's parts, place, sigmoidf, row_chunk, zero_ws

#include "../../include/taiyaki_amd_lstm_matrix_group.h"

namespace tk {
namespace {

constexpr int MG_H = 256;               // the size
constexpr int MG_G = 8;                 // workgroups of a group
constexpr int MG_U = MG_H / MG_G;       // units of a member
constexpr int MG_THREADS = 256;
constexpr int MG_TILES = 2;             // 16-row tiles of a wave: 8 units x 4 gates
constexpr int MG_KB = MG_H / 32;        // k-blocks
constexpr int MG_HPITCH = MG_H + 8;     // bf16 per column of an h image
constexpr int MG_GPITCH = 4 * MG_U + 4; // floats per column of the gx block
constexpr int MG_YPITCH = MG_U + 4;     // floats per column of the y block
constexpr int MG_RELEASE_M = 2;         // column sets per group of the release build: ahead of M = 1 at 4 of the 5
                                        // widths measured, behind at 512 (profiles/r52_lstm_matrix_group.txt)
constexpr int MG_MAX_M = 2;               // the sets built: M = 1, 2 (LDS: M = 4 would need 282 KB)
static_assert(MG_RELEASE_M >= 1 && MG_RELEASE_M <= MG_MAX_M, "the release build launches a built M");

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

__host__ __device__ constexpr unsigned step_tag(int s) { return 1u + (unsigned)s % 65535u; }

// This lane's NP pairs of granules g[off[i]], g[off[i] + 1] until every lane of the wave sees `tag` in all of its own;
// false when the clock budget runs out or another workgroup has already given up (rnn_common.h: sweep, with the tag in
// the granule's top 16 bits).  Every pass issues all loads before it waits.
template <int NP>
__device__ __forceinline__ bool gather(const u64 *g, const int (&off)[NP], unsigned tag, u64 (&a)[NP], u64 (&b)[NP],
                                       uint32_t *status) {
    const uint64_t start = __builtin_amdgcn_s_memrealtime();
    for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            a[i] = __hip_atomic_load((gu64 *)(g + off[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b[i] = __hip_atomic_load((gu64 *)(g + off[i] + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
// hbuf: [2 slots][ngroups][MG_G members][C columns][MG_U units] granules.
// (gx is not __restrict__: loads the compiler knows to be invariant are sunk through the step, each to its LDS write)
template <int M>
__global__ __launch_bounds__(MG_THREADS) void lstm_matrix_group_kernel(const float *gx, const float *__restrict__ whh,
                                                                       int T, int N, int LD, int reverse,
                                                                       float *__restrict__ y,
                                                                       const int32_t *__restrict__ lengths, u64 *hbuf,
                                                                       int ngroups, uint32_t *status) {
    constexpr int H = MG_H, H4 = 4 * MG_H, C = 16 * M;
    constexpr int GQ = C * MG_U / MG_THREADS;           // 16-byte chunks of gx per lane and step: 2 M
    constexpr int NP = (MG_G - 1) * C * (MG_U / 2) / MG_THREADS;        // pairs of granules per lane and step: 7 M
    constexpr int SLOT = MG_G * C * MG_U;               // granules of a group's slot
    __shared__ __attribute__((aligned(16))) unsigned short hb[2][3][C * MG_HPITCH];
    __shared__ __attribute__((aligned(16))) float gs[2][C * MG_GPITCH];
    __shared__ __attribute__((aligned(16))) float ys[2][C * MG_YPITCH];
    __shared__ int give_up;

    int group, member;
    place(MG_G, group, member);
    const int tid = threadIdx.x;
    const int wave = tid / 64, lane = tid % 64;
    const int col = lane % 16, quad = lane / 16;
    const int n0 = group * C;
    const int u0 = 8 * wave + quad;                     // the lane's cell of (set, tile j): unit u0 + 4 j of the member
    if (tid == 0) give_up = 0;

    // A: row lane % 16 of tile j is gate col % 4 of unit 32 member + 8 wave + 4 j + col / 4; k = 32 kb + 8 quad ... + 7
    bf16x8 wf[MG_TILES][MG_KB][3];
#pragma unroll
    for (int j = 0; j < MG_TILES; ++j) {
        const float *row = whh + (size_t)((col % 4) * H + MG_U * member + 8 * wave + 4 * j + col / 4) * H + 8 * quad;
#pragma unroll
        for (int kb = 0; kb < MG_KB; ++kb) {
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
    float cst[M][MG_TILES];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int n = n0 + 16 * m + col;
        len[m] = n >= N ? 0 : lengths ? lengths[n] : T;
#pragma unroll
        for (int j = 0; j < MG_TILES; ++j) cst[m][j] = 0.f;
    }

    // the lane's chunks of a step's gx: chunk q is floats [4 (q % 8), + 4) of gate (q / 8) % 4 of column q / 32
    size_t goff[GQ];
    int gdst[GQ];
#pragma unroll
    for (int i = 0; i < GQ; ++i) {
        const int q = tid + i * MG_THREADS, c = q / 32, gate = (q / 8) % 4, ch = q % 8;
        const int nn = n0 + c < N ? n0 + c : N - 1;
        goff[i] = (size_t)nn * H4 + gate * H + MG_U * member + 4 * ch;
        gdst[i] = c * MG_GPITCH + gate * MG_U + 4 * ch;
    }
    // ... its chunk of a step's y: floats [4 (tid % 8), + 4) of column tid / 8 (C 8 chunks: the lanes below that)
    const int yc = tid / 8;
    float *const ydst = yc < C && n0 + yc < N ? y + (size_t)(n0 + yc) * H + MG_U * member + 4 * (tid % 8) : nullptr;
    const int ysrc = (yc < C ? yc : 0) * MG_YPITCH + 4 * (tid % 8);
    // ... and its pairs of granules: pair q % 16 of column (q / 16) % C of member (member + 1 + q / (16 C)) % 8
    int poff[NP], pdst[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int q = tid + i * MG_THREADS, p = q % 16, c = (q / 16) % C, mm = (member + 1 + q / (16 * C)) % MG_G;
        poff[i] = (mm * C + c) * MG_U + 2 * p;
        pdst[i] = (c * MG_HPITCH + MG_U * mm) / 2 + p;      // in 4-byte words of an image
    }
    const size_t gstep = (size_t)LD * H4, ystep = (size_t)LD * H;
    u64 *const slots = hbuf + (size_t)group * SLOT;         // slot p: + p * ngroups * SLOT
    const size_t slot_stride = (size_t)ngroups * SLOT;

    for (int i = tid; i < 3 * C * MG_HPITCH / 2; i += MG_THREADS) reinterpret_cast<uint32_t *>(hb[0][0])[i] = 0u;
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
            if (!gather<NP>(slots + (size_t)(par ^ 1) * slot_stride, poff, step_tag(s - 1), ga, gb, status)) give_up = 1;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const uint32_t alo = (uint32_t)ga[i], blo = (uint32_t)gb[i];
                const uint32_t ahi = (uint32_t)(ga[i] >> 32), bhi = (uint32_t)(gb[i] >> 32);
                reinterpret_cast<uint32_t *>(hb[par][0])[pdst[i]] = (alo & 0xffffu) | (blo << 16);
                reinterpret_cast<uint32_t *>(hb[par][1])[pdst[i]] = (alo >> 16) | (blo & 0xffff0000u);
                reinterpret_cast<uint32_t *>(hb[par][2])[pdst[i]] = (ahi & 0xffffu) | (bhi << 16);
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

        f32x4 acc[M][MG_TILES];
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int j = 0; j < MG_TILES; ++j) {
                const float *g = gs[par] + (16 * m + col) * MG_GPITCH + u0 + 4 * j;
                acc[m][j] = f32x4{g[0], g[MG_U], g[2 * MG_U], g[3 * MG_U]};
            }
        // W1 h1, W1 h2, W2 h1, W1 h3, W3 h1, W2 h2, k-block by k-block; the sets and tiles innermost: 2 M independent
        // accumulators between two instructions on the same one
        constexpr int PW[6] = {0, 0, 1, 0, 2, 1}, PH[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
        for (int kb = 0; kb < MG_KB; ++kb) {
            bf16x8 hf[M][3];
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    hf[m][p] = as_frag(*reinterpret_cast<const uint4 *>(hb[par][p] + (16 * m + col) * MG_HPITCH + 32 * kb +
                                                                        8 * quad));
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int j = 0; j < MG_TILES; ++j)
                        acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][kb][PW[x]], hf[m][PH[x]], acc[m][j], 0, 0, 0);
        }

        u64 *const out = slots + (size_t)par * slot_stride;
        const u64 tag = (u64)step_tag(s) << 48;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float h[MG_TILES];
#pragma unroll
            for (int j = 0; j < MG_TILES; ++j) {
                const f32x4 a = acc[m][j];
                const float ig = sigmoidf(a[0]), fg = sigmoidf(a[1]), gg = tanhf(a[2]), og = sigmoidf(a[3]);
                cst[m][j] = fmaf(ig, gg, fg * cst[m][j]);
                h[j] = og * tanhf(cst[m][j]);
                if (t >= len[m]) cst[m][j] = h[j] = 0.f;
                ys[par][(16 * m + col) * MG_YPITCH + u0 + 4 * j] = h[j];
            }
            uint32_t p[3];
            split2(h[0], h[1], p[0], p[1], p[2]);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                unsigned short *at = hb[par ^ 1][q] + (16 * m + col) * MG_HPITCH + MG_U * member + u0;
                at[0] = (unsigned short)(p[q] & 0xffffu);
                at[4] = (unsigned short)(p[q] >> 16);
            }
            if (s + 1 < T) {                              // (nobody reads the last step's h)
                u64 *g = out + (member * C + 16 * m + col) * MG_U + u0;
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

constexpr bool size_built(size_t H) { return H == MG_H; }

// Column sets per group.  The release build: MG_RELEASE_M.  The lab build: TK_LAB_LSTM_MATRIX_GROUP_M = 1 or 2 in the
// environment, read at every call (tools/lstmmatrixgroupbench.py times every built M from one process), else the same.
int release_m() {
    const char *e = TK_LAB_ENV("TK_LAB_LSTM_MATRIX_GROUP_M");
    if (e && e[0] >= '1' && e[0] <= '0' + MG_MAX_M && !e[1]) return e[0] - '0';
    return MG_RELEASE_M;
}

size_t group_bytes(int m) { return (size_t)2 * MG_G * 16 * m * MG_U * sizeof(u64); }      // both slots of one group

size_t slab_columns(size_t H, int cu_count) {
    return size_built(H) && cu_count >= MG_G ? (size_t)(cu_count / MG_G) * 16 * release_m() : 0;
}

}  // namespace
}  // namespace tk

extern "C" {

int tk_lstm_matrix_group_supported(size_t size) { return tk::size_built(size) ? 1 : 0; }

int tk_lstm_matrix_group_columns(size_t size) { return tk::size_built(size) ? 16 * tk::release_m() : 0; }

size_t tk_lstm_matrix_group_slab(size_t size, int cu_count) { return tk::slab_columns(size, cu_count); }

size_t tk_lstm_matrix_group_workspace_bytes(size_t nbatch, size_t size, int cu_count) {
    using namespace tk;
    const size_t S = slab_columns(size, cu_count);
    if (S == 0 || nbatch == 0) return 0;
    const size_t C = 16 * release_m(), n = nbatch < S ? nbatch : S;
    return (n + C - 1) / C * group_bytes(release_m());
}

int tk_lstm_matrix_group_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk,
                                     size_t nbatch, size_t size, int reverse, int cu_count, float *y, void *workspace,
                                     size_t workspace_bytes, uint32_t *status, void *stream) {
    using namespace tk;
    if (!gx || !w_hh || !y || !aligned16(gx) || !aligned16(y) || nblk > (size_t)INT32_MAX || nbatch > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
    if (!workspace || !status || !aligned16(workspace)) return TK_ERR_BAD_ARG;
    if (!size_built(size) || nbatch == 0) return TK_ERR_UNSUPPORTED;
    const size_t S = slab_columns(size, cu_count);
    if (S == 0) return TK_ERR_UNSUPPORTED;
    if (workspace_bytes < tk_lstm_matrix_group_workspace_bytes(nbatch, size, cu_count)) return TK_ERR_WORKSPACE;
    if (nblk == 0) return TK_OK;
    const int m = release_m();
    const size_t C = 16 * m;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (size_t first = 0; first < nbatch; first += S) {
        const size_t n = nbatch - first < S ? nbatch - first : S;
        const int groups = (int)((n + C - 1) / C);
        const int rc = zero_ws(workspace, groups * group_bytes(m), st);
        if (rc != TK_OK) return rc;
        const float *g = gx + first * 4 * MG_H;
        float *yy = y + first * MG_H;
        const int32_t *ln = at_column(lengths, first, 1);
        const dim3 grid((unsigned)(groups * MG_G)), block(MG_THREADS);
        if (m == 2)
            hipLaunchKernelGGL(lstm_matrix_group_kernel<2>, grid, block, 0, st, g, w_hh, (int)nblk, (int)n, (int)nbatch,
                               reverse, yy, ln, static_cast<u64 *>(workspace), groups, status);
        else
            hipLaunchKernelGGL(lstm_matrix_group_kernel<1>, grid, block, 0, st, g, w_hh, (int)nblk, (int)n, (int)nbatch,
                               reverse, yy, ln, static_cast<u64 *>(workspace), groups, status);
        if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    }
    return TK_OK;
}

}  // extern "C"

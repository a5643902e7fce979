// gru_matrix_group.hip -- the forward recurrence of layers.GruMod that saves nothing (gate order r, z, n; h0 = 0) at
// H = 256 on the gfx950 matrix cores, for batches of hundreds to thousands of columns
// (include/taiyaki_amd_gru_matrix_group.h; libtaiyaki_amd_gru_matrix_group.so).  The cell, the row order, the order of
// the sums and the contract of lengths and direction are those of gru_matrix.hip (H = 96).  There one workgroup holds the
// whole split W_hh; at 256 that is 1.1 MB, so here a GROUP of workgroups holds it and hands h on through the tagged
// granules of rnn_common.h, as lstm_matrix_group.hip does for the LSTM.  The geometry is neither's.
//
// Geometry as built.  A group is GG_G = 4 workgroups of 256 lanes (4 waves, one per SIMD) and shares C = 16 M batch
// columns, M sets of the instruction's 16 (a template parameter; GG_RELEASE_M is what the entry launches).  Member g owns
// the units 64 g ... 64 g + 63 with all three gates; wave w of it the 16 units 64 g + 16 w ... + 15 as three row tiles of
// W_hh, rows gate 256 + 64 g + 16 w + i in the rows' own order: no permutation and no padded gate, every MFMA is used.
// Operands as in gru_matrix.hip: lane l of A holds row l % 16 at k = 8 (l / 16) ... + 7 of a 32-wide k-block, lane l of B
// column l % 16 at the same k, accumulator register j of lane l is row 4 (l / 16) + j of column l % 16.  So register j of
// a lane's three accumulators of a set holds r, z and q of ONE (unit, column) pair: the cell update runs in the lane, 4 M
// cells per lane, and h_prev for z h_prev stays in a float32 register for the launch.
//
// Weights.  Loaded once, split with split2 and kept: 3 tiles x 8 k-blocks x 3 parts x 4 = 288 VGPRs per lane, and b_hh
// in 12 more (one wave per SIMD has 512; profiles/r54_gru_matrix_group_resource_usage.txt: no scratch).
//
// Products.  The r and z accumulators start as gx + b_hh, the n accumulator as b_hh alone (q = W_hn h + b_hn is
// multiplied by r before gx_n joins), and each takes, k-block by k-block, W1 h1, W1 h2, W2 h1, W1 h3, W3 h1, W2 h2.
// Every column of the instruction and every set is treated alike: a column's y is a function of its gx, its length, W_hh
// and b_hh alone, not of N, the other columns, its place in the group, M or the CU count.
//
// h between members: an all-to-all per step, 3 partners.  The producer splits its new h once.  A granule is 8 bytes, one
// (unit, column): the three bf16 parts in bits 0-47 and a 16-bit tag in bits 48-63, written by ONE sc1 store and polled
// by sc1 loads until the tag matches (rnn_common.h: the data is the flag).  Two slots by step parity, zeroed in front of
// every launch.  Layout [slot][group][member][column][unit of 64]: a cell lane's 4 units are 4 granules in a row, 32
// bytes; a consumer lane reads the two granules of an adjacent pair of units (16 bytes; a wave's 64 pairs are 1 KB in a
// row), 6 M pairs per lane and step, and writes three 4-byte words, one per part, into the LDS image
// hb[parity][part][column][k].  No consumer splits anything.  A
// member's own 64 units go straight from the cell lanes to the image, 8 bytes per part.  A column of the image is
// GG_HPITCH = 264 bf16 = 33 chunks of 16 bytes, an odd number: a B fragment is one conflict-free 16-byte read.
// The tag of step s is 1 + s % 65535: never 0, what a zeroed slot holds.  A slot of parity p holds only what the steps
// of that parity wrote, in order, and no member publishes step s + 2 before every member has read step s (it needs
// step s + 1 of every member, which each published behind its own read of step s).  So a poll for step s finds 0, the
// granule of step s - 2 or that of step s; tag(s) = tag(s - 2) would need 2 = 0 mod 65535.  The tag may wrap: nblk has
// no bound of its own.
// Every spin is bounded by the clock budget (kSpinTicks); on expiry TK_STATUS_RNN_TIMEOUT is OR-ed into *status and the
// whole grid leaves.
//
// Schedule of step s (gru_kernels.hip's rule: nothing bound for HBM is issued in front of a poll in the same step).
//   poll: the other members' h of step s - 1 into hb[s & 1];
//   right behind it the gx rows of step s + 1 are asked for, whole 128-byte pieces with 16 bytes per lane, 3 M per lane;
//   barrier (the only one of the step);
//   the y rows of step s - 1 leave from ys[(s - 1) & 1] as whole 128-byte pieces, M chunks per lane;
//   accumulators from gs[s & 1], 144 MFMAs per wave and set, cell update, h to ys[s & 1], its parts to hb[(s + 1) & 1]
//   and to the granules of slot s & 1; the gx rows that arrived go to gs[(s + 1) & 1].
// A column of the gx block is GG_GPITCH = 196 floats (4 mod 64 banks: the 16 columns of a quarter wave's 16-byte read, 4
// consecutive units of one gate, start 4 banks apart, 64 different banks), of the y block GG_YPITCH = 68 (the same
// argument).  gx is not __restrict__ (DESIGN.md "LSTM inference at size 96 on the matrix cores").
//
// Lengths and tails.  At t >= lengths[n] the lane writes y = 0 and hands on h = 0 through a select behind the cell
// update: a NaN in gx there stays in that step's accumulators.  A column of the last group at or beyond N has length 0,
// loads column N - 1 and stores nothing; it still publishes, because the members wait for each other.
//
// Admission and slabs.  All members of all groups must be resident: groups x 4 <= cu_count, one workgroup per CU (LDS
// 82.5 KB at M = 1; M = 2 would need 165 KB as laid out and is not built).  A wider batch runs inside the entry as slabs
// of (cu_count / 4) C columns, launch behind launch on the caller's stream, in place on windows of columns (LD, the
// tensors' columns per time step, is a kernel argument), the granules zeroed in front of each.
#include "wgrad_common.h"       // split2, bf16x8; dispatch.h
#include "rnn_common.h"         // the granule protocol's parts, place, sigmoidf, row_chunk, zero_ws

#include "../../include/taiyaki_amd_gru_matrix_group.h"

namespace tk {
namespace {

constexpr int GG_H = 256;               // the size
constexpr int GG_G = 4;                 // workgroups of a group
constexpr int GG_U = GG_H / GG_G;       // units of a member: 16 per wave
constexpr int GG_THREADS = 256;
constexpr int GG_KB = GG_H / 32;        // k-blocks
constexpr int GG_HPITCH = GG_H + 8;     // bf16 per column of an h image
constexpr int GG_GPITCH = 3 * GG_U + 4; // floats per column of the gx block
constexpr int GG_YPITCH = GG_U + 4;     // floats per column of the y block
constexpr int GG_RELEASE_M = 1;         // column sets per group: the one built (M = 2 does not fit the LDS of a workgroup);
                                        // ahead of the main library at all 5 widths measured
                                        // (profiles/r54_gru_matrix_group.txt)
static_assert(GG_U == 16 * (GG_THREADS / 64), "a wave owns one unit tile of 16");

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

__host__ __device__ constexpr unsigned step_tag(int s) { return 1u + (unsigned)s % 65535u; }

// the granule of one (unit, column): part k of the unit in the low (hi = 0) or high half of p[k]
__device__ __forceinline__ u64 granule(uint32_t p1, uint32_t p2, uint32_t p3, int hi, u64 tag) {
    return hi ? (u64)((p1 >> 16) | (p2 & 0xffff0000u)) | ((u64)(p3 >> 16) << 32) | tag
              : (u64)((p1 & 0xffffu) | (p2 << 16)) | ((u64)(p3 & 0xffffu) << 32) | tag;
}

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
// hbuf: [2 slots][ngroups][GG_G members][C columns][GG_U units] granules.
// (gx is not __restrict__: loads the compiler knows to be invariant are sunk through the step, each to its LDS write)
template <int M>
__global__ __launch_bounds__(GG_THREADS) void gru_matrix_group_kernel(const float *gx, const float *__restrict__ whh,
                                                                      const float *__restrict__ bhh, int T, int N,
                                                                      int LD, int reverse, float *__restrict__ y,
                                                                      const int32_t *__restrict__ lengths, u64 *hbuf,
                                                                      int ngroups, uint32_t *status) {
    constexpr int H = GG_H, H3 = 3 * GG_H, C = 16 * M;
    constexpr int GQ = C * 3 * GG_U / 4 / GG_THREADS;   // 16-byte chunks of gx per lane and step: 3 M
    constexpr int YQ = C * GG_U / 4 / GG_THREADS;       // ... of y: M
    constexpr int NP = (GG_G - 1) * C * (GG_U / 2) / GG_THREADS;        // pairs of granules per lane and step: 6 M
    constexpr int SLOT = GG_G * C * GG_U;               // granules of a group's slot
    __shared__ __attribute__((aligned(16))) unsigned short hb[2][3][C * GG_HPITCH];
    __shared__ __attribute__((aligned(16))) float gs[2][C * GG_GPITCH];
    __shared__ __attribute__((aligned(16))) float ys[2][C * GG_YPITCH];
    __shared__ int give_up;

    int group, member;
    place(GG_G, group, member);
    const int tid = threadIdx.x;
    const int wave = tid / 64, lane = tid % 64;
    const int col = lane % 16, quad = lane / 16;
    const int n0 = group * C;
    const int u0 = 16 * wave + 4 * quad;                // the lane's cells of a set: units u0 ... u0 + 3 of the member
    if (tid == 0) give_up = 0;

    // A: row lane % 16 of the tile of gate g is row g H + 64 member + 16 wave + col; k = 32 kb + 8 quad ... + 7
    bf16x8 wf[3][GG_KB][3];
    f32x4 bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const float *row = whh + (size_t)(g * H + GG_U * member + 16 * wave + col) * H + 8 * quad;
#pragma unroll
        for (int kb = 0; kb < GG_KB; ++kb) {
            // (w_hh and b_hh need no more than a float's alignment)
            const row_chunk a = *reinterpret_cast<const row_chunk *>(row + 32 * kb);
            const row_chunk b = *reinterpret_cast<const row_chunk *>(row + 32 * kb + 4);
            uint4 p1, p2, p3;
            split2(a.x, a.y, p1.x, p2.x, p3.x);
            split2(a.z, a.w, p1.y, p2.y, p3.y);
            split2(b.x, b.y, p1.z, p2.z, p3.z);
            split2(b.z, b.w, p1.w, p2.w, p3.w);
            wf[g][kb][0] = as_frag(p1);
            wf[g][kb][1] = as_frag(p2);
            wf[g][kb][2] = as_frag(p3);
        }
        const row_chunk b4 = *reinterpret_cast<const row_chunk *>(bhh + g * H + GG_U * member + u0);
        bh[g] = f32x4{b4.x, b4.y, b4.z, b4.w};
    }

    int len[M];
    f32x4 hp[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int n = n0 + 16 * m + col;
        len[m] = n >= N ? 0 : lengths ? lengths[n] : T;
        hp[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // the lane's chunks of a step's gx: chunk q is floats [4 (q % 16), + 4) of gate (q / 16) % 3 of column q / 48
    size_t goff[GQ];
    int gdst[GQ];
#pragma unroll
    for (int i = 0; i < GQ; ++i) {
        const int q = tid + i * GG_THREADS, c = q / 48, gate = (q / 16) % 3, ch = q % 16;
        const int nn = n0 + c < N ? n0 + c : N - 1;
        goff[i] = (size_t)nn * H3 + gate * H + GG_U * member + 4 * ch;
        gdst[i] = c * GG_GPITCH + gate * GG_U + 4 * ch;
    }
    // ... its chunks of a step's y: chunk q is floats [4 (q % 16), + 4) of column q / 16
    float *ydst[YQ];
    int ysrc[YQ];
#pragma unroll
    for (int i = 0; i < YQ; ++i) {
        const int q = tid + i * GG_THREADS, c = q / 16, ch = q % 16;
        ydst[i] = n0 + c < N ? y + (size_t)(n0 + c) * H + GG_U * member + 4 * ch : nullptr;
        ysrc[i] = c * GG_YPITCH + 4 * ch;
    }
    // ... and its pairs of granules: pair q % 32 of column (q / 32) % C of member (member + 1 + q / (32 C)) % 4
    int poff[NP], pdst[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int q = tid + i * GG_THREADS, p = q % 32, c = (q / 32) % C, mm = (member + 1 + q / (32 * C)) % GG_G;
        poff[i] = (mm * C + c) * GG_U + 2 * p;
        pdst[i] = (c * GG_HPITCH + GG_U * mm) / 2 + p;      // in 4-byte words of an image
    }
    const size_t gstep = (size_t)LD * H3, ystep = (size_t)LD * H;
    u64 *const slots = hbuf + (size_t)group * SLOT;         // slot p: + p * ngroups * SLOT
    const size_t slot_stride = (size_t)ngroups * SLOT;

    for (int i = tid; i < 3 * C * GG_HPITCH / 2; i += GG_THREADS) reinterpret_cast<uint32_t *>(hb[0][0])[i] = 0u;
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
        if (s > 0) {
            const size_t tp = (size_t)(reverse ? t + 1 : t - 1);
#pragma unroll
            for (int i = 0; i < YQ; ++i) {
                if (!ydst[i]) continue;
                const float4 v = *reinterpret_cast<const float4 *>(ys[par ^ 1] + ysrc[i]);
                *reinterpret_cast<row_chunk *>(ydst[i] + tp * ystep) = row_chunk{v.x, v.y, v.z, v.w};
            }
        }

        f32x4 acc[M][3], gxn[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float *g = gs[par] + (16 * m + col) * GG_GPITCH + u0;
            acc[m][0] = *reinterpret_cast<const f32x4 *>(g) + bh[0];
            acc[m][1] = *reinterpret_cast<const f32x4 *>(g + GG_U) + bh[1];
            acc[m][2] = bh[2];
            gxn[m] = *reinterpret_cast<const f32x4 *>(g + 2 * GG_U);
        }
        // W1 h1, W1 h2, W2 h1, W1 h3, W3 h1, W2 h2, k-block by k-block; the sets and gates innermost: 3 M independent
        // accumulators between two instructions on the same one
        constexpr int PW[6] = {0, 0, 1, 0, 2, 1}, PH[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
        for (int kb = 0; kb < GG_KB; ++kb) {
            bf16x8 hf[M][3];
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    hf[m][p] = as_frag(*reinterpret_cast<const uint4 *>(hb[par][p] + (16 * m + col) * GG_HPITCH + 32 * kb +
                                                                        8 * quad));
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int g = 0; g < 3; ++g)
                        acc[m][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[g][kb][PW[x]], hf[m][PH[x]], acc[m][g], 0, 0, 0);
        }

        u64 *const out = slots + (size_t)par * slot_stride;
        const u64 tag = (u64)step_tag(s) << 48;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const bool past = t >= len[m];
            f32x4 h;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float rg = sigmoidf(acc[m][0][j]), zg = sigmoidf(acc[m][1][j]);
                const float ng = tanhf(gxn[m][j] + rg * acc[m][2][j]);
                const float hn = (1.f - zg) * ng + zg * hp[m][j];
                h[j] = past ? 0.f : hn;
            }
            hp[m] = h;
            *reinterpret_cast<f32x4 *>(ys[par] + (16 * m + col) * GG_YPITCH + u0) = h;
            uint2 p1, p2, p3;
            split2(h[0], h[1], p1.x, p2.x, p3.x);
            split2(h[2], h[3], p1.y, p2.y, p3.y);
            const int at = (16 * m + col) * GG_HPITCH + GG_U * member + u0;
            *reinterpret_cast<uint2 *>(hb[par ^ 1][0] + at) = p1;
            *reinterpret_cast<uint2 *>(hb[par ^ 1][1] + at) = p2;
            *reinterpret_cast<uint2 *>(hb[par ^ 1][2] + at) = p3;
            if (s + 1 < T) {                              // (nobody reads the last step's h)
                u64 *g = out + (member * C + 16 * m + col) * GG_U + u0;
                __hip_atomic_store((gu64 *)g, granule(p1.x, p2.x, p3.x, 0, tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store((gu64 *)(g + 1), granule(p1.x, p2.x, p3.x, 1, tag), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store((gu64 *)(g + 2), granule(p1.y, p2.y, p3.y, 0, tag), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store((gu64 *)(g + 3), granule(p1.y, p2.y, p3.y, 1, tag), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int i = 0; i < GQ; ++i) *reinterpret_cast<f32x4 *>(gs[par ^ 1] + gdst[i]) = gn[i];
    }
    if (T > 0) {
        __syncthreads();
        const size_t tl = (size_t)(reverse ? 0 : T - 1);
#pragma unroll
        for (int i = 0; i < YQ; ++i) {
            if (!ydst[i]) continue;
            const float4 v = *reinterpret_cast<const float4 *>(ys[(T - 1) & 1] + ysrc[i]);
            *reinterpret_cast<row_chunk *>(ydst[i] + tl * ystep) = row_chunk{v.x, v.y, v.z, v.w};
        }
    }
}

constexpr bool size_built(size_t H) { return H == GG_H; }
constexpr size_t GG_C = 16 * GG_RELEASE_M;                                             // columns of a group
constexpr size_t GG_GROUP_BYTES = (size_t)2 * GG_G * GG_C * GG_U * sizeof(u64);        // both slots of one group

size_t slab_columns(size_t H, int cu_count) {
    return size_built(H) && cu_count >= GG_G ? (size_t)(cu_count / GG_G) * GG_C : 0;
}

}  // namespace
}  // namespace tk

extern "C" {

int tk_gru_matrix_group_supported(size_t size) { return tk::size_built(size) ? 1 : 0; }

int tk_gru_matrix_group_columns(size_t size) { return tk::size_built(size) ? (int)tk::GG_C : 0; }

size_t tk_gru_matrix_group_slab(size_t size, int cu_count) { return tk::slab_columns(size, cu_count); }

size_t tk_gru_matrix_group_workspace_bytes(size_t nbatch, size_t size, int cu_count) {
    using namespace tk;
    const size_t S = slab_columns(size, cu_count);
    if (S == 0 || nbatch == 0) return 0;
    const size_t n = nbatch < S ? nbatch : S;
    return (n + GG_C - 1) / GG_C * GG_GROUP_BYTES;
}

int tk_gru_matrix_group_forward_dev(const float *gx, const float *w_hh, const float *b_hh, const int32_t *lengths,
                                    size_t nblk, size_t nbatch, size_t size, int reverse, int cu_count, float *y,
                                    void *workspace, size_t workspace_bytes, uint32_t *status, void *stream) {
    using namespace tk;
    if (!gx || !w_hh || !b_hh || !y || !aligned16(gx) || !aligned16(y) || nblk > (size_t)INT32_MAX ||
        nbatch > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
    if (!workspace || !status || !aligned16(workspace)) return TK_ERR_BAD_ARG;
    if (!size_built(size) || nbatch == 0) return TK_ERR_UNSUPPORTED;
    const size_t S = slab_columns(size, cu_count);
    if (S == 0) return TK_ERR_UNSUPPORTED;
    if (workspace_bytes < tk_gru_matrix_group_workspace_bytes(nbatch, size, cu_count)) return TK_ERR_WORKSPACE;
    if (nblk == 0) return TK_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (size_t first = 0; first < nbatch; first += S) {
        const size_t n = nbatch - first < S ? nbatch - first : S;
        const int groups = (int)((n + GG_C - 1) / GG_C);
        const int rc = zero_ws(workspace, groups * GG_GROUP_BYTES, st);
        if (rc != TK_OK) return rc;
        const dim3 grid((unsigned)(groups * GG_G)), block(GG_THREADS);
        hipLaunchKernelGGL(gru_matrix_group_kernel<GG_RELEASE_M>, grid, block, 0, st, gx + first * 3 * GG_H, w_hh, b_hh,
                           (int)nblk, (int)n, (int)nbatch, reverse, y + first * GG_H, at_column(lengths, first, 1),
                           static_cast<u64 *>(workspace), groups, status);
        if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    }
    return TK_OK;
}

}  // extern "C"

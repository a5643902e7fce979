// lstm_matrix.hip -- the forward recurrence of layers.Lstm that saves nothing (gate order i, f, g, o; h0 = c0 = 0) at
// H = 96 on the gfx950 matrix cores, for batches of thousands of columns (include/taiyaki_amd_lstm_matrix.h;
// libtaiyaki_amd_lstm_matrix.so).  The cell, the tensors and the contract of lengths and direction are those of
// lstm_local.hip; the geometry is its own.  lstm_local.hip gives a workgroup 1 or 2 columns, so a weight held in a
// register serves 2 columns per step; here a workgroup owns 16 columns and W_hh h is v_mfma_f32_16x16x32_bf16 on float32
// operands split three ways into bf16 (wgrad_common.h: split2), so a weight in a register serves 16.
//
// Split of the work.  A workgroup is 4 waves and owns all 96 units of 16 batch columns.  Wave w owns the units
// 24 w ... 24 w + 23 with all four of their gates: 96 rows of W_hh as MX_TILES = 6 row tiles of 16.  Row 4 q + i of tile j
// is gate i of unit 24 w + 4 j + q.  The instruction's operands: lane l of A holds row l % 16 at k = 8 (l / 16) ... + 7
// of a 32-wide k-block, lane l of B column l % 16 at the same k, and accumulator register r of lane l is row
// 4 (l / 16) + r of column l % 16.  So a lane's four accumulator registers of tile j are the four gates of ONE (unit,
// column) pair, (24 w + 4 j + l / 16, l % 16): the cell update runs in the lane, with no shuffle and no LDS round trip
// for the gates, and a lane carries the c of its 6 cells in registers through the launch.
//
// Weights.  Each lane loads the 8 consecutive k of its rows once, splits them and keeps the parts: 6 tiles x 3 k-blocks x
// 3 parts x 4 VGPRs = 216 registers (__launch_bounds__(256): one wave per SIMD, 512 registers).
//
// h.  A lane splits its 6 new h into three bf16 parts once and writes them into the image hb[parity][part][column][k].
// The next step's B fragment of (k-block, part) is one 16-byte read, 9 per lane and step.  A column is MX_HPITCH = 104
// bf16 = 13 chunks of 16 bytes: an odd number, so the 16 columns that read together fall on 16 different chunks.
//
// gx.  A step's 16 x 384 floats are loaded as whole rows, 16 bytes per lane, 6 loads per lane, right behind the barrier
// of the step before, and written to LDS in front of the step's own barrier, behind the MFMAs and the cell update they
// drained under.  A column is MX_GPITCH = 388 floats: 4 mod 64 banks, so the 16 columns x 4 units of a wave's 4-byte
// read are 64 different banks (at 384 all 16 columns of a unit are one bank).  The values are the accumulators' start.
//
// y.  h in float32 goes to ys[parity][column] (MX_YPITCH = 100 floats: 36 mod 64, the same argument) and leaves one
// barrier later as whole rows, 16 bytes per lane (rows_to_global's pattern, with the pitch).
//
// One __syncthreads per step.  Step s reads hb, gs of parity s and writes hb, gs of parity s + 1 and ys of parity s; ys of
// parity s - 1 is read behind the barrier between the two steps.  Nothing bound for HBM is waited on in front of a
// barrier but the gx loads issued a whole step earlier.
//
// Order of the sums.  An accumulator starts as gx and takes, k-block by k-block, the six products W1 h1, W1 h2, W2 h1,
// W1 h3, W3 h1, W2 h2 (products of bf16 values are exact in float32; the three dropped terms lie below 2^-24 |w h|).  A
// column of the accumulator is a function of that column of B alone, and the instruction treats its 16 columns alike: a
// column's y does not depend on nbatch, on the other columns or on its place in the workgroup.
//
// Lengths.  Column n has lengths[n] steps (NULL: T).  At t >= lengths[n] the lane writes y = 0 and hands on h = c = 0
// through a select behind the cell update: what gx holds there, a NaN too, stays in that column's accumulators of that
// step.  A column of the last workgroup at or beyond N has length 0, loads column N - 1 and stores nothing.
#include "wgrad_common.h"       // split2, bf16x8; dispatch.h
#include "rnn_common.h"         // sigmoidf, row_chunk

#include "../../include/taiyaki_amd_lstm_matrix.h"

namespace tk {
namespace {

constexpr int MX_H = 96;                // the size
constexpr int MX_COLS = 16;             // batch columns of a workgroup: the instruction's N
constexpr int MX_THREADS = 256;
constexpr int MX_TILES = 6;             // 16-row tiles of a wave: 24 units x 4 gates
constexpr int MX_KB = MX_H / 32;        // k-blocks
constexpr int MX_HPITCH = 104;          // bf16 per column of an h image
constexpr int MX_GPITCH = 4 * MX_H + 4; // floats per column of the gx block
constexpr int MX_YPITCH = MX_H + 4;     // floats per column of the y block
constexpr int MX_GQ = MX_COLS * MX_H / MX_THREADS;                  // 16-byte chunks of gx per lane and step: 6
constexpr int MX_YQ = (MX_COLS * MX_H / 4 + MX_THREADS - 1) / MX_THREADS;    // ... of y: 2 (the second half used)

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

// (gx is not __restrict__: loads the compiler knows to be invariant are sunk through the step, each to its LDS write)
__global__ __launch_bounds__(MX_THREADS) void lstm_matrix_fwd_kernel(const float *gx,
                                                                     const float *__restrict__ whh, int T, int N,
                                                                     int reverse, float *__restrict__ y,
                                                                     const int32_t *__restrict__ lengths) {
    constexpr int H = MX_H, H4 = 4 * MX_H;
    __shared__ __attribute__((aligned(16))) unsigned short hb[2][3][MX_COLS * MX_HPITCH];
    __shared__ __attribute__((aligned(16))) float gs[2][MX_COLS * MX_GPITCH];
    __shared__ __attribute__((aligned(16))) float ys[2][MX_COLS * MX_YPITCH];

    const int tid = threadIdx.x;
    const int wave = tid / 64, lane = tid % 64;
    const int col = lane % 16, quad = lane / 16;
    const int n0 = blockIdx.x * MX_COLS;
    const int u0 = 24 * wave + quad;                   // the lane's cell of tile j: unit u0 + 4 j, column col

    // A: row lane % 16 of tile j is gate col % 4 of unit 24 wave + 4 j + col / 4; k = 32 kb + 8 quad ... + 7
    bf16x8 wf[MX_TILES][MX_KB][3];
#pragma unroll
    for (int j = 0; j < MX_TILES; ++j) {
        const float *row = whh + (size_t)((col % 4) * H + 24 * wave + 4 * j + col / 4) * H + 8 * quad;
#pragma unroll
        for (int kb = 0; kb < MX_KB; ++kb) {
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

    const bool live = n0 + col < N;
    const int len = !live ? 0 : lengths ? lengths[n0 + col] : T;
    float cst[MX_TILES];
#pragma unroll
    for (int j = 0; j < MX_TILES; ++j) cst[j] = 0.f;

    // the lane's chunks of a step's gx (chunk q: floats [4 (q % 96), + 4) of column q / 96) and of its y (q % 24, q / 24)
    size_t goff[MX_GQ];
    int gdst[MX_GQ];
#pragma unroll
    for (int i = 0; i < MX_GQ; ++i) {
        const int q = tid + i * MX_THREADS, c = q / H, nn = n0 + c < N ? n0 + c : N - 1;
        goff[i] = (size_t)nn * H4 + 4 * (q % H);
        gdst[i] = c * MX_GPITCH + 4 * (q % H);
    }
    float *ydst[MX_YQ];
    int ysrc[MX_YQ];
#pragma unroll
    for (int i = 0; i < MX_YQ; ++i) {
        const int q = tid + i * MX_THREADS, c = q / (H / 4);
        ydst[i] = q < MX_COLS * H / 4 && n0 + c < N ? y + (size_t)(n0 + c) * H + 4 * (q % (H / 4)) : nullptr;
        ysrc[i] = (c < MX_COLS ? c : 0) * MX_YPITCH + 4 * (q % (H / 4));
    }
    const size_t gstep = (size_t)N * H4, ystep = (size_t)N * H;

    for (int i = tid; i < 3 * MX_COLS * MX_HPITCH / 2; i += MX_THREADS) reinterpret_cast<uint32_t *>(hb[0][0])[i] = 0u;
    {
        const float *g = gx + (size_t)(reverse ? T - 1 : 0) * gstep;
#pragma unroll
        for (int i = 0; i < MX_GQ; ++i)
            *reinterpret_cast<float4 *>(gs[0] + gdst[i]) = *reinterpret_cast<const float4 *>(g + goff[i]);
    }
    __syncthreads();

    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        const int par = s & 1;
        // behind the barrier: the rows of the step before leave, the rows of the next step are asked for
        if (s > 0) {
            const size_t tp = (size_t)(reverse ? t + 1 : t - 1);
#pragma unroll
            for (int i = 0; i < MX_YQ; ++i) {
                if (!ydst[i]) continue;
                const float4 v = *reinterpret_cast<const float4 *>(ys[par ^ 1] + ysrc[i]);
                *reinterpret_cast<row_chunk *>(ydst[i] + tp * ystep) = row_chunk{v.x, v.y, v.z, v.w};
            }
        }
        // (no branch: the last step asks for its own rows again, and nothing reads them)
        f32x4 gn[MX_GQ];
        const float *gnext = gx + (size_t)(s + 1 == T ? t : reverse ? t - 1 : t + 1) * gstep;
#pragma unroll
        for (int i = 0; i < MX_GQ; ++i) gn[i] = *reinterpret_cast<const f32x4 *>(gnext + goff[i]);
        asm volatile("" ::: "memory");                   // the deferred stores and the prefetch stay here

        f32x4 acc[MX_TILES];
#pragma unroll
        for (int j = 0; j < MX_TILES; ++j) {
            const float *g = gs[par] + col * MX_GPITCH + u0 + 4 * j;
            acc[j] = f32x4{g[0], g[H], g[2 * H], g[3 * H]};
        }
        bf16x8 hf[MX_KB][3];
#pragma unroll
        for (int kb = 0; kb < MX_KB; ++kb)
#pragma unroll
            for (int p = 0; p < 3; ++p)
                hf[kb][p] = as_frag(*reinterpret_cast<const uint4 *>(hb[par][p] + col * MX_HPITCH + 32 * kb + 8 * quad));
        // W1 h1, W1 h2, W2 h1, W1 h3, W3 h1, W2 h2; the tiles innermost: six independent accumulators between two
        // instructions on the same one
        constexpr int PW[6] = {0, 0, 1, 0, 2, 1}, PH[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
        for (int kb = 0; kb < MX_KB; ++kb)
#pragma unroll
            for (int m = 0; m < 6; ++m)
#pragma unroll
                for (int j = 0; j < MX_TILES; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][kb][PW[m]], hf[kb][PH[m]], acc[j], 0, 0, 0);

        float h[MX_TILES];
#pragma unroll
        for (int j = 0; j < MX_TILES; ++j) {
            const float ig = sigmoidf(acc[j][0]), fg = sigmoidf(acc[j][1]), gg = tanhf(acc[j][2]), og = sigmoidf(acc[j][3]);
            cst[j] = fmaf(ig, gg, fg * cst[j]);
            h[j] = og * tanhf(cst[j]);
            if (t >= len) cst[j] = h[j] = 0.f;
            ys[par][col * MX_YPITCH + u0 + 4 * j] = h[j];
        }
#pragma unroll
        for (int j = 0; j < MX_TILES; j += 2) {
            uint32_t p[3];
            split2(h[j], h[j + 1], p[0], p[1], p[2]);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                unsigned short *at = hb[par ^ 1][q] + col * MX_HPITCH + u0 + 4 * j;
                at[0] = (unsigned short)(p[q] & 0xffffu);
                at[4] = (unsigned short)(p[q] >> 16);
            }
        }
#pragma unroll
        for (int i = 0; i < MX_GQ; ++i) *reinterpret_cast<f32x4 *>(gs[par ^ 1] + gdst[i]) = gn[i];
        __syncthreads();
    }
    if (T > 0) {
        const size_t tl = (size_t)(reverse ? 0 : T - 1);
#pragma unroll
        for (int i = 0; i < MX_YQ; ++i) {
            if (!ydst[i]) continue;
            const float4 v = *reinterpret_cast<const float4 *>(ys[(T - 1) & 1] + ysrc[i]);
            *reinterpret_cast<row_chunk *>(ydst[i] + tl * ystep) = row_chunk{v.x, v.y, v.z, v.w};
        }
    }
}

constexpr bool size_built(size_t H) { return H == MX_H; }

}  // namespace
}  // namespace tk

extern "C" {

int tk_lstm_matrix_supported(size_t size) { return tk::size_built(size) ? 1 : 0; }

int tk_lstm_matrix_columns(size_t size) { return tk::size_built(size) ? tk::MX_COLS : 0; }

int tk_lstm_matrix_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                               size_t size, int reverse, float *y, void *stream) {
    using namespace tk;
    if (!gx || !w_hh || !y || !aligned16(gx) || !aligned16(y) || nblk > (size_t)INT32_MAX || nbatch > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
    if (!size_built(size) || nbatch == 0) return TK_ERR_UNSUPPORTED;
    if (nblk == 0) return TK_OK;
    const unsigned grid = (unsigned)((nbatch + MX_COLS - 1) / MX_COLS);
    hipLaunchKernelGGL(lstm_matrix_fwd_kernel, dim3(grid), dim3(MX_THREADS), 0, static_cast<hipStream_t>(stream), gx, w_hh,
                       (int)nblk, (int)nbatch, reverse, y, lengths);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // extern "C"

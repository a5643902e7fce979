// gru_matrix.hip -- the forward recurrence of layers.GruMod that saves nothing (gate order r, z, n; h0 = 0) at H = 96 on
// the gfx950 matrix cores, for batches of thousands of columns (include/taiyaki_amd_gru_matrix.h;
// libtaiyaki_amd_gru_matrix.so).  The cell, the tensors and the contract of lengths and direction are those of
// gru_kernels.hip; the geometry is its own.  gru_kernels.hip gives a workgroup 1 or 2 columns at this size, so a weight
// held in a register serves 2 columns per step; here a workgroup owns 16 columns and W_hh h is
// v_mfma_f32_16x16x32_bf16 on float32 operands split three ways into bf16 (wgrad_common.h: split2), so a weight in a
// register serves 16.  The operator, the operand layout and the movement of gx, h and y are those of lstm_matrix.hip; the
// place of the gates is not.
//
// Split of the work.  The 96 units are GM_UNIT_TILES = 6 unit tiles of 16 consecutive units.  A wave owns UT of them
// (UT = 1: 6 waves, 384 lanes; UT = 2: 3 waves, 192 lanes; both are built, tk_gru_matrix_forward_dev launches
// GM_RELEASE_UT).  Unit tile v has three row tiles of W_hh, rows g 96 + 16 v + i for the gates g = r, z, n, in the
// rows' own order: no permutation.  The instruction's operands: lane l of A holds row l % 16 at k = 8 (l / 16) ... + 7
// of a 32-wide k-block, lane l of B column l % 16 at the same k, and accumulator register j of lane l is row
// 4 (l / 16) + j of column l % 16.  So the three accumulators of a unit tile hold, in register j of lane l, r, z and q of
// ONE (unit, column) pair, (16 v + 4 (l / 16) + j, l % 16): the cell update runs in the lane, 4 cells per unit tile, with
// no shuffle and no LDS round trip for the gates.  The lane that makes h(unit, column) is the same at every step, so
// h_prev for z h_prev stays in a float32 register through the launch and is never rebuilt from its bf16 parts.
//
// Weights.  Each lane loads the 8 consecutive k of its rows once, splits them and keeps the parts: UT x 3 gates x 3
// k-blocks x 3 parts x 4 VGPRs = 108 (UT = 1) or 216 (UT = 2) registers.  b_hh: 12 UT registers more.
//
// Accumulators.  The r and z tiles start as gx + b_hh, the n tile as b_hh alone: q = W_hn h + b_hn is multiplied by r
// before gx_n joins, so b_hn cannot be folded into gx.
//
// h.  A lane's 4 cells of a unit tile are 4 consecutive units: it splits them into three bf16 parts once and writes each
// part's 4 values as one 8-byte store into the image hb[parity][part][column][k].  The next step's B fragment of (k-block,
// part) is one 16-byte read, 9 per lane and step.  A column is GM_HPITCH = 104 bf16 = 13 chunks of 16 bytes: an odd
// number, so the 16 columns that read together fall on 16 different chunks.
//
// gx.  A step's 16 x 288 floats are loaded as whole rows, 16 bytes per lane, right behind the barrier of the step
// before, and written to LDS in front of the step's own barrier, behind the MFMAs and the cell update they drained under.
// A column is GM_GPITCH = 292 floats: 36 mod 64 banks, so the 16 columns of a quarter wave's 16-byte read (4 consecutive
// units of one gate) start 4 banks apart, 64 different banks.
//
// y.  h in float32 goes to ys[parity][column] as one 16-byte store per unit tile (GM_YPITCH = 100 floats: 36 mod 64, the
// same argument) and leaves one barrier later as whole rows, 16 bytes per lane.
//
// One __syncthreads per step.  Step s reads hb, gs of parity s and writes hb, gs of parity s + 1 and ys of parity s; ys of
// parity s - 1 is read behind the barrier between the two steps.  Nothing bound for HBM is waited on in front of a
// barrier but the gx loads issued a whole step earlier.
//
// Order of the sums.  An accumulator takes, k-block by k-block, the six products W1 h1, W1 h2, W2 h1, W1 h3, W3 h1,
// W2 h2 (products of bf16 values are exact in float32; the three dropped terms lie below 2^-24 |w h|).  A column of the
// accumulator is a function of that column of B alone, and the instruction treats its 16 columns alike: a column's y does
// not depend on nbatch, on the other columns or on its place in the workgroup -- nor on UT, which only deals the same
// tiles to other waves.
//
// Lengths.  Column n has lengths[n] steps (NULL: T).  At t >= lengths[n] the lane writes y = 0 and hands on h = 0 through
// a select behind the cell update: what gx holds there, a NaN too, stays in that column's registers of that step.  A
// column of the last workgroup at or beyond N has length 0, loads column N - 1 and stores nothing.
#include "ff_common.h"          // TK_LAB_ENV
#include "wgrad_common.h"       // split2, bf16x8; dispatch.h
#include "rnn_common.h"         // sigmoidf, row_chunk

#include "../../include/taiyaki_amd_gru_matrix.h"

namespace tk {
namespace {

constexpr int GM_H = 96;                // the size
constexpr int GM_COLS = 16;             // batch columns of a workgroup: the instruction's N
constexpr int GM_UNIT_TILES = GM_H / 16;
constexpr int GM_KB = GM_H / 32;        // k-blocks
constexpr int GM_HPITCH = 104;          // bf16 per column of an h image
constexpr int GM_GPITCH = 3 * GM_H + 4; // floats per column of the gx block
constexpr int GM_YPITCH = GM_H + 4;     // floats per column of the y block
constexpr int GM_GCHUNKS = GM_COLS * 3 * GM_H / 4;      // 16-byte chunks of a step's gx: 1152
constexpr int GM_YCHUNKS = GM_COLS * GM_H / 4;          // ... of its y: 384
// Unit tiles per wave of the launch (profiles/r53_gru_matrix.txt: both forms timed from the lab build)
constexpr int GM_RELEASE_UT = 1;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

// (gx is not __restrict__: loads the compiler knows to be invariant are sunk through the step, each to its LDS write)
template <int UT>
__global__ __launch_bounds__(64 * GM_UNIT_TILES / UT) void gru_matrix_fwd_kernel(const float *gx,
                                                                                 const float *__restrict__ whh,
                                                                                 const float *__restrict__ bhh, int T,
                                                                                 int N, int reverse,
                                                                                 float *__restrict__ y,
                                                                                 const int32_t *__restrict__ lengths) {
    constexpr int H = GM_H, H3 = 3 * GM_H;
    constexpr int THREADS = 64 * GM_UNIT_TILES / UT;
    constexpr int GQ = GM_GCHUNKS / THREADS;            // chunks of gx per lane and step: 3 or 6
    constexpr int YQ = GM_YCHUNKS / THREADS;            // ... of y: 1 or 2
    static_assert(GQ * THREADS == GM_GCHUNKS && YQ * THREADS == GM_YCHUNKS, "whole chunks per lane");
    __shared__ __attribute__((aligned(16))) unsigned short hb[2][3][GM_COLS * GM_HPITCH];
    __shared__ __attribute__((aligned(16))) float gs[2][GM_COLS * GM_GPITCH];
    __shared__ __attribute__((aligned(16))) float ys[2][GM_COLS * GM_YPITCH];

    const int tid = threadIdx.x;
    const int wave = tid / 64, lane = tid % 64;
    const int col = lane % 16, quad = lane / 16;
    const int n0 = blockIdx.x * GM_COLS;
    const int u0 = 16 * UT * wave + 4 * quad;           // the lane's cells of unit tile v: units u0 + 16 v ... + 3, column col

    // A: row lane % 16 of the tile of gate g and unit tile v is row g H + 16 (UT wave + v) + col; k = 32 kb + 8 quad ... + 7
    bf16x8 wf[UT][3][GM_KB][3];
    f32x4 bh[UT][3];
#pragma unroll
    for (int v = 0; v < UT; ++v)
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float *row = whh + (size_t)(g * H + 16 * (UT * wave + v) + col) * H + 8 * quad;
#pragma unroll
            for (int kb = 0; kb < GM_KB; ++kb) {
                // (w_hh and b_hh need no more than a float's alignment)
                const row_chunk a = *reinterpret_cast<const row_chunk *>(row + 32 * kb);
                const row_chunk b = *reinterpret_cast<const row_chunk *>(row + 32 * kb + 4);
                uint4 p1, p2, p3;
                split2(a.x, a.y, p1.x, p2.x, p3.x);
                split2(a.z, a.w, p1.y, p2.y, p3.y);
                split2(b.x, b.y, p1.z, p2.z, p3.z);
                split2(b.z, b.w, p1.w, p2.w, p3.w);
                wf[v][g][kb][0] = as_frag(p1);
                wf[v][g][kb][1] = as_frag(p2);
                wf[v][g][kb][2] = as_frag(p3);
            }
            const row_chunk b4 = *reinterpret_cast<const row_chunk *>(bhh + g * H + u0 + 16 * v);
            bh[v][g] = f32x4{b4.x, b4.y, b4.z, b4.w};
        }

    const bool live = n0 + col < N;
    const int len = !live ? 0 : lengths ? lengths[n0 + col] : T;
    f32x4 hp[UT];
#pragma unroll
    for (int v = 0; v < UT; ++v) hp[v] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the lane's chunks of a step's gx (chunk q: floats [4 (q % 72), + 4) of column q / 72) and of its y (q % 24, q / 24)
    size_t goff[GQ];
    int gdst[GQ];
#pragma unroll
    for (int i = 0; i < GQ; ++i) {
        const int q = tid + i * THREADS, c = q / (H3 / 4), nn = n0 + c < N ? n0 + c : N - 1;
        goff[i] = (size_t)nn * H3 + 4 * (q % (H3 / 4));
        gdst[i] = c * GM_GPITCH + 4 * (q % (H3 / 4));
    }
    float *ydst[YQ];
    int ysrc[YQ];
#pragma unroll
    for (int i = 0; i < YQ; ++i) {
        const int q = tid + i * THREADS, c = q / (H / 4);
        ydst[i] = n0 + c < N ? y + (size_t)(n0 + c) * H + 4 * (q % (H / 4)) : nullptr;
        ysrc[i] = c * GM_YPITCH + 4 * (q % (H / 4));
    }
    const size_t gstep = (size_t)N * H3, ystep = (size_t)N * H;

    for (int i = tid; i < 3 * GM_COLS * GM_HPITCH / 2; i += THREADS) reinterpret_cast<uint32_t *>(hb[0][0])[i] = 0u;
    {
        const float *g = gx + (size_t)(reverse ? T - 1 : 0) * gstep;
#pragma unroll
        for (int i = 0; i < GQ; ++i)
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
            for (int i = 0; i < YQ; ++i) {
                if (!ydst[i]) continue;
                const float4 v = *reinterpret_cast<const float4 *>(ys[par ^ 1] + ysrc[i]);
                *reinterpret_cast<row_chunk *>(ydst[i] + tp * ystep) = row_chunk{v.x, v.y, v.z, v.w};
            }
        }
        // (no branch: the last step asks for its own rows again, and nothing reads them)
        f32x4 gn[GQ];
        const float *gnext = gx + (size_t)(s + 1 == T ? t : reverse ? t - 1 : t + 1) * gstep;
#pragma unroll
        for (int i = 0; i < GQ; ++i) gn[i] = *reinterpret_cast<const f32x4 *>(gnext + goff[i]);
        asm volatile("" ::: "memory");                   // the deferred stores and the prefetch stay here

        f32x4 acc[UT][3], gxn[UT];
#pragma unroll
        for (int v = 0; v < UT; ++v) {
            const float *g = gs[par] + col * GM_GPITCH + u0 + 16 * v;
            acc[v][0] = *reinterpret_cast<const f32x4 *>(g) + bh[v][0];
            acc[v][1] = *reinterpret_cast<const f32x4 *>(g + H) + bh[v][1];
            acc[v][2] = bh[v][2];
            gxn[v] = *reinterpret_cast<const f32x4 *>(g + 2 * H);
        }
        bf16x8 hf[GM_KB][3];
#pragma unroll
        for (int kb = 0; kb < GM_KB; ++kb)
#pragma unroll
            for (int p = 0; p < 3; ++p)
                hf[kb][p] = as_frag(*reinterpret_cast<const uint4 *>(hb[par][p] + col * GM_HPITCH + 32 * kb + 8 * quad));
        // W1 h1, W1 h2, W2 h1, W1 h3, W3 h1, W2 h2; the tiles innermost: 3 UT independent accumulators between two
        // instructions on the same one
        constexpr int PW[6] = {0, 0, 1, 0, 2, 1}, PH[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
        for (int kb = 0; kb < GM_KB; ++kb)
#pragma unroll
            for (int m = 0; m < 6; ++m)
#pragma unroll
                for (int v = 0; v < UT; ++v)
#pragma unroll
                    for (int g = 0; g < 3; ++g)
                        acc[v][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[v][g][kb][PW[m]], hf[kb][PH[m]], acc[v][g],
                                                                            0, 0, 0);

        const bool past = t >= len;
#pragma unroll
        for (int v = 0; v < UT; ++v) {
            f32x4 h;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float rg = sigmoidf(acc[v][0][j]), zg = sigmoidf(acc[v][1][j]);
                const float ng = tanhf(gxn[v][j] + rg * acc[v][2][j]);
                const float hn = (1.f - zg) * ng + zg * hp[v][j];
                h[j] = past ? 0.f : hn;
            }
            hp[v] = h;
            *reinterpret_cast<f32x4 *>(ys[par] + col * GM_YPITCH + u0 + 16 * v) = h;
            uint2 p1, p2, p3;
            split2(h[0], h[1], p1.x, p2.x, p3.x);
            split2(h[2], h[3], p1.y, p2.y, p3.y);
            const int at = col * GM_HPITCH + u0 + 16 * v;
            *reinterpret_cast<uint2 *>(hb[par ^ 1][0] + at) = p1;
            *reinterpret_cast<uint2 *>(hb[par ^ 1][1] + at) = p2;
            *reinterpret_cast<uint2 *>(hb[par ^ 1][2] + at) = p3;
        }
#pragma unroll
        for (int i = 0; i < GQ; ++i) *reinterpret_cast<f32x4 *>(gs[par ^ 1] + gdst[i]) = gn[i];
        __syncthreads();
    }
    if (T > 0) {
        const size_t tl = (size_t)(reverse ? 0 : T - 1);
#pragma unroll
        for (int i = 0; i < YQ; ++i) {
            if (!ydst[i]) continue;
            const float4 v = *reinterpret_cast<const float4 *>(ys[(T - 1) & 1] + ysrc[i]);
            *reinterpret_cast<row_chunk *>(ydst[i] + tl * ystep) = row_chunk{v.x, v.y, v.z, v.w};
        }
    }
}

constexpr bool size_built(size_t H) { return H == GM_H; }

// Unit tiles per wave.  The release build: GM_RELEASE_UT.  The lab build: TK_LAB_GRU_MATRIX_UT = 1 or 2 in the
// environment, read at every call (tools/grumatrixbench.py times both forms from one process), else the same.
int release_ut() {
    const char *e = TK_LAB_ENV("TK_LAB_GRU_MATRIX_UT");
    if (e && (e[0] == '1' || e[0] == '2') && !e[1]) return e[0] - '0';
    return GM_RELEASE_UT;
}

}  // namespace
}  // namespace tk

extern "C" {

int tk_gru_matrix_supported(size_t size) { return tk::size_built(size) ? 1 : 0; }

int tk_gru_matrix_columns(size_t size) { return tk::size_built(size) ? tk::GM_COLS : 0; }

int tk_gru_matrix_forward_dev(const float *gx, const float *w_hh, const float *b_hh, const int32_t *lengths, size_t nblk,
                              size_t nbatch, size_t size, int reverse, float *y, void *stream) {
    using namespace tk;
    if (!gx || !w_hh || !b_hh || !y || !aligned16(gx) || !aligned16(y) || nblk > (size_t)INT32_MAX ||
        nbatch > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
    if (!size_built(size) || nbatch == 0) return TK_ERR_UNSUPPORTED;
    if (nblk == 0) return TK_OK;
    const unsigned grid = (unsigned)((nbatch + GM_COLS - 1) / GM_COLS);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (release_ut() == 2)
        hipLaunchKernelGGL(gru_matrix_fwd_kernel<2>, dim3(grid), dim3(64 * GM_UNIT_TILES / 2), 0, st, gx, w_hh, b_hh,
                           (int)nblk, (int)nbatch, reverse, y, lengths);
    else
        hipLaunchKernelGGL(gru_matrix_fwd_kernel<1>, dim3(grid), dim3(64 * GM_UNIT_TILES), 0, st, gx, w_hh, b_hh,
                           (int)nblk, (int)nbatch, reverse, y, lengths);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // extern "C"

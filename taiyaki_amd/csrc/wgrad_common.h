// wgrad_common.h -- the parameter gradients of one recurrent layer, A^T [x | y shifted | 1], as one split-K GEMM on the
// bf16 matrix cores, every float32 operand split into three bf16 parts, and one reduction: the plan, the kernel and the
// reduction, shared by lstm_wgrad.hip and gru_wgrad.hip.  The cell (a template parameter, defined by the including
// file) says where A comes from, how the bias sums are laid out and what the reduction writes.
//
// A (K = T N rows of M = GATES H), x (K x I) and y (K x H) are row-major with the summed index as the row.  A block of
// WG_KB = 16 rows, one k-step of v_mfma_f32_32x32x16_bf16, is staged as it lies in memory, [k][m]: each thread
// splits its float4s a = a1 + a2 + a3 (a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2), round to nearest even,
// both differences exact) and writes 8 bytes into each of three bf16 images per operand.  An image row is 128 bf16 =
// 256 bytes = one LDS bank row, its 16-byte chunk c stored at chunk c ^ ((k & 3) << 2): the four rows that one
// ds_read_b64_tr_b16 gathers per 16 lanes then lie in four different 64-byte bank groups, so the operand reads (the
// summed index is the row in both operands, so both are transposed reads, two per 8-element fragment) are
// conflict-free.  The product is a1 b1 + (a1 b2 + a2 b1 + a2 b2 + a1 b3 + a3 b1): products of bf16 values are exact
// in float32 and the three dropped terms lie below 2^-26 |a b|.  The first term and the five corrections have an
// accumulator set each (WG_ACC_SETS), added once per partial result.  A zero splits into three zeros: rows of A that
// are 0 add exactly 0.
// A workgroup of eight waves owns a 128 x 128 output tile (each wave 64 x 32: 2 x 1 accumulators, twice) over one run
// of rows.  The output's columns are tiled per operand -- x's columns, then y's -- so a tile reads one of the two; a y
// tile reads y at row k -/+ N (the previous step's h of the same batch element), rows outside [0, K) as zeros.  The
// workgroups of the first column of tiles add up the columns of the float32 A block they stage anyway: the bias sums.
// Rows per run are a multiple of WG_KB, so only the last block of all is ragged.  A run longer than WG_CHAIN rows is
// cut again, inside its workgroup, into partial results of their own: no accumulation chain is longer than that.
// blockIdx = column tile * rstride + (row tile * runs + run) with rstride a multiple of 8: the workgroups that
// read the same rows of A sit on one XCD and share its L2.
// The tall form (TALL; wgrad_tall says when): a workgroup owns the two row tiles 2p and 2p + 1, 256 x 128 (each wave
// 64 x 64: 2 x 2 accumulators, twice), over the first or the second half of a run's partial results.  The x / y block is
// split, written and read as fragments once for both row tiles, and a wave issues 24 MFMAs between two barriers, not 12.
// A partial result is the same sums of the same fragments in the same order as in the square form: the same bits.
// blockIdx = column tile * rstride + ((tile pair * runs + run) * 2 + half): same grid, same padding of rstride, and
// with runs a multiple of 4 the workgroups of one (run, half) share blockIdx % 8.
//
// A cell:
//   GATES        M = GATES H
//   SEAM         false: A is dG (leading dimension M) for every tile.  true (the GRU): the x tiles read dG, the y tiles
//                a virtual M-wide A whose column m is dG[k][m] below 2H and dq[k][m - 2H] from there on, chosen per
//                thread at the float4 it stages (H is even: no float4 lies across the seam); the workgroups of the
//                first y tile column add up their columns from 2H on, a second bias sum of H entries
//   EXTRA_BIAS   that second sum's length in units of H: a partial result is [M][I + H] | [M] | [EXTRA_BIAS H]
//   Args         the kernel's argument (WgradArgs, or a struct derived from it that adds dq)
//   Bias         what the reduction writes the bias sums to, through store_bias(db, i, v, M, H) for entry i of
//                [M] | [EXTRA_BIAS H]
//   takes(H)     sizes the cell admits
//   VEC4_EDGE    whether the cell has the WG_VEC4 instantiation (load4)
#pragma once
#include "dispatch.h"

namespace tk {
namespace {

constexpr int WG_TILE = 128;        // output tile edge
constexpr int WG_KB = 16;           // rows per staged block
constexpr int WG_THREADS = 512;     // two waves per SIMD: one wave's split (VALU) runs under the other's MFMAs
constexpr int WG_SROWS = WG_THREADS / 32;           // rows of a block staged per pass of the workgroup
constexpr int WG_SPASS = WG_KB / WG_SROWS;          // ... and passes per block
constexpr int WG_NJ = WG_TILE / 32 / (WG_THREADS / 128);    // 32-column accumulators per wave across (two down)
constexpr size_t WG_CHAIN = 8192;   // the longest accumulation chain, in rows
// accumulator sets: 2 = a1 b1 and the five corrections accumulate apart, 1 = in one set.  Measured at the same speed;
// error against float64 of the LSTM's dW_ih at (T, N, H, I) = (800, 128, 256, 256) 6.3e-7 with two, 1.6e-6 with one
// (the float32 MFMA kernel before: 1.6e-6; rocBLAS: 5.3e-6), and 2.7e-5 against 8.5e-5 on the cancelling input of
// tests/test_lstm_split_gemm.py
constexpr int WG_ACC_SETS = 2;
constexpr int WG_IMAGE = WG_KB * WG_TILE * 2;       // bytes of one bf16 image of a block

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct WgradPlan {
    int tiles_m, tiles_x, tiles_y;  // output tiles down (M) and across (I, then H)
    int splits, nsub;               // runs of rows, partial results per run
    int run_rows, sub_rows;         // rows per run and per partial result (multiples of WG_KB)
    int rstride, grid;
    size_t slab_floats, slabs;      // one partial result [M][I + H] | [M] | [EXTRA_BIAS H], and how many there are
};

int g_lab_splits = 0;   // lab build: force the number of runs (0 = the rule below)

size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// The plan: a function of the shape and the CU count only.  tiles * runs <= cu_count where the tiles alone fit.
template <class Cell>
bool wgrad_plan(size_t T, size_t N, size_t H, size_t I, int cu_count, WgradPlan *p) {
    if (T == 0 || N == 0 || H == 0 || I == 0 || cu_count <= 0 || !Cell::takes(H)) return false;
    if (H > (1u << 20) || I > (1u << 20) || N > (1u << 28) || T > (size_t(1) << 30) / N) return false;
    const size_t K = T * N, M = Cell::GATES * H, W = I + H, B = M + Cell::EXTRA_BIAS * H;
    if (M * W + B >= (size_t(1) << 31)) return false;
    const size_t tm = ceil_div(M, WG_TILE), tx = ceil_div(I, WG_TILE), ty = ceil_div(H, WG_TILE);
    const size_t tiles = tm * (tx + ty);
    size_t G = g_lab_splits > 0 ? (size_t)g_lab_splits : (size_t)cu_count / tiles;
    if (G < 1) G = 1;
    const size_t run = ceil_div(ceil_div(K, G), WG_KB) * WG_KB;
    G = ceil_div(K, run);           // (no empty runs)
    const size_t nsub = ceil_div(run, WG_CHAIN);
    const size_t sub = ceil_div(ceil_div(run, nsub), WG_KB) * WG_KB;
    const size_t rstride = ceil_div(tm * G, 8) * 8;
    if (rstride * (tx + ty) >= (size_t(1) << 31)) return false;
    p->tiles_m = (int)tm, p->tiles_x = (int)tx, p->tiles_y = (int)ty;
    p->splits = (int)G, p->nsub = (int)nsub, p->run_rows = (int)run, p->sub_rows = (int)sub;
    p->rstride = (int)rstride, p->grid = (int)(rstride * (tx + ty));
    p->slab_floats = (M * W + B + 3) / 4 * 4;
    p->slabs = G * nsub;
    return true;
}

struct WgradArgs {
    const float *dg, *x, *y;
    float *ws;
    int K, N, M, I, H, reverse;
    int tiles_m, tiles_x, splits, nsub, run_rows, sub_rows, rstride;
    size_t slab_floats;
};

// How a block is loaded.  WG_FAST: every tile lies inside its matrix and takes 16-byte loads.  WG_VEC4 (the cells with
// VEC4_EDGE): 16-byte loads too -- the tensors are aligned and I and H are multiples of 4, so a float4 lies inside its
// row or past its end as a whole -- but tiles hang over the edges.  WG_GUARDED: anything.
enum { WG_GUARDED = 0, WG_FAST = 1, WG_VEC4 = 2 };

// four floats of row `row` from column `col` on.  WIDE (WG_FAST, WG_VEC4) is one unconditional load, of row 0 where
// the row is not there (WG_VEC4: of column 0 where the column is not, which the caller folds into row_ok): the caller
// zeroes it when it stages the value, so nothing branches or waits for memory before the block's MFMAs.  Otherwise
// zeros where the row is not there or the column is past the edge.
template <bool WIDE>
__device__ __forceinline__ float4 load4(const float *src, int ld, int row, bool row_ok, int col) {
    if (WIDE) return *reinterpret_cast<const float4 *>(src + (size_t)(row_ok ? row : 0) * (size_t)ld + col);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row_ok) {
        const float *p = src + (size_t)row * (size_t)ld + col;
        if (col < ld) v.x = p[0];
        if (col + 1 < ld) v.y = p[1];
        if (col + 2 < ld) v.z = p[2];
        if (col + 3 < ld) v.w = p[3];
    }
    return v;
}

// two floats -> their three bf16 parts, the first float's in the low halves (v_cvt_pk_bf16_f32; bf16 -> float is a shift)
__device__ __forceinline__ void split2(float u, float v, uint32_t &p1, uint32_t &p2, uint32_t &p3) {
    p1 = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{u, v}, bf16x2));
    u -= __uint_as_float(p1 << 16), v -= __uint_as_float(p1 & 0xffff0000u);
    p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{u, v}, bf16x2));
    u -= __uint_as_float(p2 << 16), v -= __uint_as_float(p2 & 0xffff0000u);
    p3 = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{u, v}, bf16x2));
}

// the three parts of four floats into the three images of one operand, 8 bytes each
__device__ __forceinline__ void stage4(unsigned char *img, float4 v) {
    uint2 p1, p2, p3;
    split2(v.x, v.y, p1.x, p2.x, p3.x);
    split2(v.z, v.w, p1.y, p2.y, p3.y);
    *reinterpret_cast<uint2 *>(img) = p1;
    *reinterpret_cast<uint2 *>(img + WG_IMAGE) = p2;
    *reinterpret_cast<uint2 *>(img + 2 * WG_IMAGE) = p3;
}

// rows 8 (lane >> 5) ... + 7 of 32 columns of an image as one operand fragment: `at` is the lane's address for the
// first four rows (wgrad_kernel), the next four are 4 image rows on
__device__ __forceinline__ bf16x8 frag(const unsigned char *at) {
    typedef bf16x4 __attribute__((address_space(3))) * lds_ptr;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)at);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)(at + 4 * WG_TILE * 2));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <class Cell, int LOADS, bool TALL = false>
__global__ __launch_bounds__(WG_THREADS) void wgrad_kernel(const typename Cell::Args a) {
    constexpr int RT = TALL ? 2 : 1;                        // row tiles of a workgroup
    constexpr int WACR = TALL ? 2 : WG_THREADS / 128;       // waves across its 128 columns
    constexpr int NJ = WG_TILE / 32 / WACR;                 // 32-column accumulators per wave across (two down)
    static_assert(!TALL || LOADS == WG_FAST, "the tall form stages whole tiles");
    __shared__ __attribute__((aligned(16))) unsigned char img[2][RT + 1][3][WG_IMAGE];   // [buffer][A's row tiles, x / y][part]
    __shared__ __attribute__((aligned(16))) float colsum[WG_THREADS / 32][RT * WG_TILE];

    const int tnx = blockIdx.x / a.rstride, q = blockIdx.x % a.rstride;
    if (q >= a.tiles_m * a.splits) return;      // (the padding of rstride)
    // square: q = row tile * runs + run, every part of the run.  Tall: q = (tile pair * runs + run) * 2 + half, the
    // first or the second nsub / 2 parts of the run
    const int qr = TALL ? q >> 1 : q;
    const int run = qr % a.splits, tmx = RT * (qr / a.splits);
    const int sub_begin = TALL ? (q & 1) * (a.nsub / 2) : 0, sub_end = TALL ? sub_begin + a.nsub / 2 : a.nsub;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhalf = lane >> 5;
    // tall: the wave's 64 rows lie in A's image wm / 128, from its column wm % 128 on
    const int wm = (wave / WACR) * 64, wn = (wave % WACR) * 32 * NJ;
    const int wmi = TALL ? wm & (WG_TILE - 1) : wm;
    const int c4 = (tid & 31) * 4, r0 = tid >> 5;       // staging: this thread's four columns and first row of a block
    // ... and where they go in an image: chunk c4 / 8 of row r0, swizzled; rows r0 and r0 + 8 swizzle alike
    const int woff = 256 * r0 + 16 * (((tid & 31) >> 1) ^ ((r0 & 3) << 2)) + 8 * (tid & 1);
    // the transposed read: lane 4 tq + tp of each 16 gives the address of row tq, columns 4 tp ... + 3 of its block of
    // 4 rows x 16 columns; the wave's four blocks are columns 0-15 / 16-31 of rows 8 lhalf ... + 3
    const int tq = (lane >> 2) & 3, tp = lane & 3;
    int aoff[2], boff[NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = 256 * (8 * lhalf + tq) + 8 * (tp & 1), chunk = 4 * i + 2 * ((lane >> 4) & 1) + (tp >> 1);
        aoff[i] = row + 16 * ((wmi / 8 + chunk) ^ (tq << 2));
        if constexpr (TALL) aoff[i] += (wm / WG_TILE) * 3 * WG_IMAGE;
        if (i < NJ) boff[i] = row + 16 * ((wn / 8 + chunk) ^ (tq << 2));
    }

    const bool is_x = tnx < a.tiles_x;
    const float *bsrc = is_x ? a.x : a.y;
    const int bld = is_x ? a.I : a.H;
    const int bcol0 = (is_x ? tnx : tnx - a.tiles_x) * WG_TILE;
    const int shift = is_x ? 0 : (a.reverse ? a.N : -a.N);
    const int out_col0 = is_x ? bcol0 : a.I + bcol0;
    const int W = a.I + a.H;
    const bool sum_cols = tnx == 0 || (Cell::SEAM && tnx == a.tiles_x);
    const int acol = tmx * WG_TILE + c4, bcol = bcol0 + c4;
    // where this thread's float4 of A comes from (tall: the second row tile's 128 columns on; with whole tiles 2H is a
    // multiple of 256, so both lie on one side of the seam)
    const float *asrc = a.dg;
    int ald = a.M, acolx = acol;
    if constexpr (Cell::SEAM) {
        if (!is_x && acol >= 2 * a.H) asrc = a.dq, ald = a.H, acolx = acol - 2 * a.H;
    }

    // WG_VEC4: a float4 past the end of its row is loaded from column 0 instead and staged as zeros
    bool acok = true, bcok = true;
    int acl = acolx, bcl = bcol;
    if constexpr (LOADS == WG_VEC4) {
        acok = acolx < ald, bcok = bcol < bld;
        acl = acok ? acolx : 0, bcl = bcok ? bcol : 0;
    }

    const int run_begin = run * a.run_rows;
    const int run_end = min(run_begin + a.run_rows, a.K);

    for (int sub = sub_begin; sub < sub_end; ++sub) {
        const int k0 = run_begin + sub * a.sub_rows;
        const int k1 = min(k0 + a.sub_rows, run_end);
        const int nkb = k1 > k0 ? (k1 - k0 + WG_KB - 1) / WG_KB : 0;

        f32x16 acc[WG_ACC_SETS][2][NJ];
#pragma unroll
        for (int s = 0; s < WG_ACC_SETS; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[s][i][j][r] = 0.f;
        float4 dbacc[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) dbacc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        // two blocks are in flight from memory: block kb + 2 is requested before the MFMAs of block kb, block kb + 1
        // is split and written to LDS after them
        float4 ra[2][WG_SPASS][RT], rb[2][WG_SPASS];
        bool oka[2][WG_SPASS], okb[2][WG_SPASS];

        auto fetch = [&](int kb, int set) {
#pragma unroll
            for (int j = 0; j < WG_SPASS; ++j) {
                const int k = k0 + kb * WG_KB + r0 + WG_SROWS * j;
                const int kk = k + shift;
                oka[set][j] = k < k1 && acok, okb[set][j] = k < k1 && kk >= 0 && kk < a.K && bcok;
                // (the second row tile's load written out: as a loop over the row tiles the guarded form's branches
                // compiled to three more scalar instructions than they had)
                ra[set][j][0] = load4<LOADS != WG_GUARDED>(asrc, ald, k, oka[set][j], acl);
                if constexpr (TALL) ra[set][j][1] = load4<true>(asrc, ald, k, oka[set][j], acl + WG_TILE);
                rb[set][j] = load4<LOADS != WG_GUARDED>(bsrc, bld, kk, okb[set][j], bcl);
            }
        };
        auto stash = [&](int set, int buf) {
#pragma unroll
            for (int j = 0; j < WG_SPASS; ++j) {
                float4 va[RT], vb = rb[set][j];
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    va[t] = ra[set][j][t];
                    if (!oka[set][j]) va[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if (!okb[set][j]) vb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int t = 0; t < RT; ++t) stage4(&img[buf][t][0][woff + 256 * WG_SROWS * j], va[t]);
                stage4(&img[buf][RT][0][woff + 256 * WG_SROWS * j], vb);
#pragma unroll
                for (int t = 0; t < RT; ++t)    // (used where sum_cols)
                    dbacc[t].x += va[t].x, dbacc[t].y += va[t].y, dbacc[t].z += va[t].z, dbacc[t].w += va[t].w;
            }
        };

        // no branch inside the loop: a block past the end is fetched as zeros (row 0 where the loads are unguarded)
        // and adds nothing, so the blocks go in pairs and every fetch and stash is unconditional
        fetch(0, 0);
        fetch(1, 1);
        stash(0, 0);
        __syncthreads();
        for (int kb2 = 0; kb2 < nkb; kb2 += 2) {
#pragma unroll
            for (int cur = 0; cur < 2; ++cur) {     // block kb is in LDS buffer kb & 1 and came through register set kb & 1
                const int kb = kb2 + cur;
                fetch(kb + 2, cur);
                bf16x8 fa[2][3], fb[NJ][3];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        fa[i][p] = frag(&img[cur][0][0][p * WG_IMAGE + aoff[i]]);
                        if (i < NJ) fb[i][p] = frag(&img[cur][RT][p][boff[i]]);
                    }
                // a1 b1, then the corrections, the smallest first
                constexpr int PA[6] = {0, 2, 0, 1, 1, 0}, PB[6] = {0, 0, 2, 1, 0, 1};
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const int s = t > 0 ? WG_ACC_SETS - 1 : 0;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[s][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][PA[t]], fb[j][PB[t]],
                                                                                    acc[s][i][j], 0, 0, 0);
                }
                stash(cur ^ 1, cur ^ 1);    // (its last readers passed the barrier of block kb - 1)
                __syncthreads();
            }
        }

        // this partial result: C[m][n] of accumulator register r sits at row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31
        float *slab = a.ws + (size_t)(run * a.nsub + sub) * a.slab_floats;
        // tall: the stores' addresses are worked out here, after the blocks; left to the compiler they are hoisted out
        // of the loop over the parts and, with 128 accumulators, 38 registers of them spill around the block loop
        int wme = wm, wne = wn;
        if constexpr (TALL) asm volatile("" : "+v"(wme), "+v"(wne));
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int n = wne + 32 * j + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = tmx * WG_TILE + wme + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    const float v = WG_ACC_SETS == 2 ? acc[0][i][j][r] + acc[WG_ACC_SETS - 1][i][j][r] : acc[0][i][j][r];
                    if (m < a.M && bcol0 + n < bld) slab[(size_t)m * W + out_col0 + n] = v;
                }
            }
        if (sum_cols) {
#pragma unroll
            for (int t = 0; t < RT; ++t) *reinterpret_cast<float4 *>(&colsum[r0][c4 + WG_TILE * t]) = dbacc[t];
            __syncthreads();
            if (tid < RT * WG_TILE) {
                float v = colsum[0][tid];
#pragma unroll
                for (int r = 1; r < WG_THREADS / 32; ++r) v += colsum[r][tid];
                const int m = tmx * WG_TILE + tid;
                if constexpr (Cell::SEAM) {
                    // the x side: every column of dG; the y side: the columns that came from dq
                    if (is_x) {
                        if (m < a.M) slab[(size_t)a.M * W + m] = v;
                    } else if (m >= 2 * a.H && m < a.M) {
                        slab[(size_t)a.M * W + a.M + (m - 2 * a.H)] = v;
                    }
                } else {
                    if (m < a.M) slab[(size_t)a.M * W + m] = v;
                }
            }
        }
    }
}

// dw_ih | dw_hh | the bias sums = the partial results added in their order
template <class Cell>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *ws, size_t slab_floats, int slabs, int M, int I,
                                                           int H, int zero_hh, float *dw_ih, float *dw_hh,
                                                           typename Cell::Bias db) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t W = (size_t)I + H, MW = (size_t)M * W;
    if (idx >= MW + M + Cell::EXTRA_BIAS * H) return;
    float v = ws[idx];
#pragma unroll 4
    for (int p = 1; p < slabs; ++p) v += ws[(size_t)p * slab_floats + idx];
    if (idx >= MW) {
        Cell::store_bias(db, idx - MW, v, M, H);
        return;
    }
    const size_t m = idx / W, c = idx % W;
    if (c < (size_t)I)
        dw_ih[m * I + c] = v;
    else
        dw_hh[m * H + (c - I)] = zero_hh ? 0.f : v;
}

template <class Cell>
size_t wgrad_workspace_bytes(size_t T, size_t N, size_t H, size_t I, int cu_count) {
    WgradPlan p;
    if (!wgrad_plan<Cell>(T, N, H, I, cu_count, &p)) return 0;
    return p.slabs * p.slab_floats * sizeof(float);
}

// Which loads a call takes (`aligned`: every operand is 16-byte aligned): whole tiles and 16-byte loads everywhere,
// 16-byte loads and ragged tiles (a cell without that instantiation: the guarded loads), or the guarded loads
template <class Cell>
int wgrad_loads(bool aligned, size_t H, size_t I) {
    if (aligned && H % WG_TILE == 0 && I % WG_TILE == 0) return WG_FAST;
    if (aligned && H % 4 == 0 && I % 4 == 0) return Cell::VEC4_EDGE ? WG_VEC4 : WG_GUARDED;
    return WG_GUARDED;
}

// Which form a call with those loads and that plan takes.  Tall: a workgroup owns two row tiles, 2p and 2p + 1, over
// half of a run's partial results, where a square one owns one tile over all of them; every partial result is made of
// the same sums in the same order either way.  It wants whole tiles, row tiles in pairs and the parts of a run in halves.
inline bool wgrad_tall(int loads, const WgradPlan &p) { return loads == WG_FAST && p.tiles_m % 2 == 0 && p.nsub % 2 == 0; }

// The two launches.  `a` comes with its operand pointers set (the caller has refused NULLs); `aligned`: they are all
// 16-byte aligned.
template <class Cell>
int wgrad_launch(typename Cell::Args a, bool aligned, size_t T, size_t N, size_t H, size_t I, int reverse, int cu_count,
                 float *dw_ih, float *dw_hh, typename Cell::Bias db, void *ws, size_t wsb, hipStream_t stream) {
    WgradPlan p;
    if (!wgrad_plan<Cell>(T, N, H, I, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    if (wsb < p.slabs * p.slab_floats * sizeof(float)) return TK_ERR_WORKSPACE;
    a.ws = static_cast<float *>(ws);
    a.K = (int)(T * N), a.N = (int)N, a.M = (int)(Cell::GATES * H), a.I = (int)I, a.H = (int)H, a.reverse = reverse != 0;
    a.tiles_m = p.tiles_m, a.tiles_x = p.tiles_x, a.splits = p.splits, a.nsub = p.nsub;
    a.run_rows = p.run_rows, a.sub_rows = p.sub_rows, a.rstride = p.rstride;
    a.slab_floats = p.slab_floats;
    // (a cell without the WG_VEC4 instantiation never gets that answer: its case launches the guarded loads again)
    constexpr int EDGE = Cell::VEC4_EDGE ? WG_VEC4 : WG_GUARDED;
    switch (wgrad_loads<Cell>(aligned, H, I)) {
    case WG_FAST:
        if (wgrad_tall(WG_FAST, p))
            hipLaunchKernelGGL((wgrad_kernel<Cell, WG_FAST, true>), dim3(p.grid), dim3(WG_THREADS), 0, stream, a);
        else
            hipLaunchKernelGGL((wgrad_kernel<Cell, WG_FAST>), dim3(p.grid), dim3(WG_THREADS), 0, stream, a);
        break;
    case WG_VEC4:
        hipLaunchKernelGGL((wgrad_kernel<Cell, EDGE>), dim3(p.grid), dim3(WG_THREADS), 0, stream, a);
        break;
    default:
        hipLaunchKernelGGL((wgrad_kernel<Cell, WG_GUARDED>), dim3(p.grid), dim3(WG_THREADS), 0, stream, a);
    }
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    const size_t total = (size_t)a.M * (I + H) + a.M + Cell::EXTRA_BIAS * H;
    hipLaunchKernelGGL(wgrad_reduce_kernel<Cell>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const float *>(ws), p.slab_floats, (int)p.slabs, a.M, a.I, a.H, T == 1 ? 1 : 0,
                       dw_ih, dw_hh, db);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

// the lab hook's view of the plan: out[8] = output tiles down and across, runs, partial results per run, rows per run,
// rows per partial result, grid, partial results in the workspace
template <class Cell>
int wgrad_lab_plan(size_t T, size_t N, size_t H, size_t I, int cu_count, size_t *out) {
    WgradPlan p;
    if (!wgrad_plan<Cell>(T, N, H, I, cu_count, &p)) return 0;
    const size_t v[8] = {(size_t)p.tiles_m, (size_t)(p.tiles_x + p.tiles_y), (size_t)p.splits, (size_t)p.nsub,
                         (size_t)p.run_rows, (size_t)p.sub_rows, (size_t)p.grid, p.slabs};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return 1;
}

}  // namespace
}  // namespace tk

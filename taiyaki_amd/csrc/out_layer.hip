// out_layer.hip -- the models' output layer (GlobalNormFlipFlop, GlobalNormFlipFlopCatMod), forward and backward, on the
// bf16 matrix cores, every float32 operand split into three bf16 parts (include/taiyaki_amd_out_layer.h;
// libtaiyaki_amd_out_layer.so).  The split and the six products are those of wgrad_common.h (split2, the order of the
// products, two accumulator sets), the weights' pre-split images those of rnn_proj.hip.
//
// The output is at most 64 columns wide, so a WAVEFRONT owns 32 rows and every column (L padded to OL_NB = 1 or 2 blocks
// of 32) and the waves of a workgroup share nothing but the epilogue's tables: no operand passes through LDS and no
// barrier sits in a k loop.  An operand fragment of v_mfma_f32_32x32x16_bf16 is 8 consecutive k of one row per lane
// (row = lane & 31, k half = lane >> 5), so a lane loads its 32 bytes of x, splits them in registers and multiplies;
// the weights' fragments come from the workspace (L2) as one coalesced 1 KB load each, as in rnn_proj.hip.
//
// out_fwd_kernel (four waves, OL_RT = 128 rows a workgroup): k in ascending blocks of 16, then z = (leading +
// corrections) + bias crosses LDS once ([32 rows][65]) and the wave writes its 32 O contiguous floats of y in order:
// element (r, o) is scale tanh(z[r][src[o]]) or the log-softmax of z[r][src[o]] over the outputs of its group.
// out_bwd_kernel (two waves, 64 rows a workgroup): dy and y of the wave's rows cross LDS, lane (row, l) forms dz[row][l]
// as the sum over the outputs that read linear column l in ascending o, and dz replaces them in LDS.  From there the
// wave (a) splits dz as the fragments of dz^T -- 8 consecutive ROWS of one column per lane -- and writes them to the
// workspace, [block of 16 rows][column block][part][lane][16 bytes], zeros beyond `rows`, and (b) multiplies dz by the
// images of w^T, 64 columns of dx at a time, the fragments of dz staying in registers.
// out_wgrad_kernel: per run of rows (a multiple of 16, at most 8192) one wave per 32 columns of [x | 1], at most 8 waves a
// workgroup; per block of 16 rows the wave loads dz^T's fragments as they lie, gathers and splits x's (8 rows of one
// column per lane: each load of the wave is two whole 128-byte rows), one block ahead, and accumulates the (32 OL_NB) x
// 32 piece of dz^T [x | 1]: the column of ones gives the bias sums.  out_reduce_kernel adds the runs' partial results in
// their order.
#include "wgrad_common.h"

#include "../../include/taiyaki_amd_out_layer.h"

namespace tk {
namespace {

constexpr int OL_WROWS = 32;                    // rows of a wavefront
constexpr int OL_RT = 128;                      // rows of a forward workgroup: four waves
constexpr int OL_BWD_RT = 64;                   // ... and of a backward one: two (dy, y and dz of 32 rows are 16 KB of LDS)
constexpr int OL_KB = 16;                       // k per MFMA step
constexpr int OL_FRAG = 1024;                   // bytes of one operand fragment: 64 lanes x 16
constexpr int OL_ZS = 65;                       // floats from one row of z / dz to the next in LDS
constexpr int OL_DXC = 2;                       // 32-column blocks of dx a wave holds at a time
constexpr int OL_WG_WAVES = 8;                  // waves of a weight-gradient workgroup at most
constexpr int OL_RED_SLICES = 8;                // pieces the runs are cut into when their partial results are added
constexpr int OL_MAXW = 64;                     // L and O at most
constexpr size_t OL_CHAIN = 8192;               // the longest accumulation chain of the weight gradient, in rows
constexpr unsigned OL_TANH = 0xff, OL_MANY = 0xff, OL_NONE = 0xfe;

// the epilogue's tables, bytes packed in words, passed by value: src[o], group[o] (OL_TANH: scaled tanh), the first and
// the last output of o's group, and per linear column l the one output that reads it (OL_MANY: several, OL_NONE: none)
struct OutTables {
    uint32_t src[16], grp[16], gfirst[16], glast[16], inv[16];
};
constexpr int OL_TAB_WORDS = sizeof(OutTables) / 4;

struct OutPlan {
    int nb, nkb, klb, cb;           // 32-column blocks of L, k blocks of the forward (I / 16) and of dx (L / 16 up), 32-column blocks of I
    int tiles;                      // forward workgroups
    int runs, run_rows, nw;         // weight gradient: runs of rows, rows per run, waves (32-column blocks of [x | 1]) per run
    size_t off_wt, off_dz, off_part, slab_floats, bytes;
};

bool out_width_ok(size_t I, size_t L) {
    const bool known = I == 16 || I == 32 || I == 64 || I == 96 || I == 128 || I == 192 || I == 256 || I == 384;
    return known && L >= 1 && L <= (size_t)OL_MAXW;
}

// The plan: a function of its arguments only.  Workspace: the images of w (forward), those of w^T (dx), the fragments
// of dz^T, the runs' partial results [L][I] | [L]
bool out_plan(size_t rows, size_t I, size_t L, int cu_count, OutPlan *p) {
    if (rows == 0 || cu_count <= 0 || !out_width_ok(I, L)) return false;
    if (rows >= (size_t(1) << 31) / (I > 64 ? I : 64)) return false;
    p->nb = (int)ceil_div(L, 32), p->nkb = (int)(I / OL_KB), p->klb = (int)ceil_div(L, OL_KB), p->cb = (int)ceil_div(I, 32);
    p->tiles = (int)ceil_div(rows, OL_RT);
    // a run's workgroup has one wave per 32 columns of [x | 1]; with few of them, more runs per CU
    p->nw = (int)ceil_div(I + 1, 32);
    const size_t per_cu = ceil_div(OL_WG_WAVES, p->nw);
    size_t run = ceil_div(ceil_div(rows, (size_t)cu_count * per_cu), OL_KB) * OL_KB;
    if (run > OL_CHAIN) run = OL_CHAIN;
    p->run_rows = (int)run, p->runs = (int)ceil_div(rows, run);
    p->slab_floats = (L * I + L + 3) / 4 * 4;
    p->off_wt = (size_t)p->nkb * 3 * p->nb * OL_FRAG;
    p->off_dz = p->off_wt + (size_t)p->klb * 3 * p->cb * OL_FRAG;
    p->off_part = p->off_dz + ceil_div(rows, OL_WROWS) * 2 * p->nb * 3 * OL_FRAG;
    p->bytes = p->off_part + (size_t)p->runs * p->slab_floats * sizeof(float);
    return true;
}

// 8 floats -> the three parts of an operand fragment's 16 bytes
__device__ __forceinline__ void split8(const float *v, bf16x8 *f) {
    uint4 p1, p2, p3;
    split2(v[0], v[1], p1.x, p2.x, p3.x);
    split2(v[2], v[3], p1.y, p2.y, p3.y);
    split2(v[4], v[5], p1.z, p2.z, p3.z);
    split2(v[6], v[7], p1.w, p2.w, p3.w);
    f[0] = __builtin_bit_cast(bf16x8, p1), f[1] = __builtin_bit_cast(bf16x8, p2), f[2] = __builtin_bit_cast(bf16x8, p3);
}

// The three bf16 parts of B as [k block][part][column block][lane][16 bytes], one piece (8 consecutive k of one column
// n) per thread and part.  Forward: B[n][k] = w[n][k] (n < L).  transposed (dx): B[n][k] = w[k][n] (n < I, k < L).
__global__ __launch_bounds__(256) void out_prep_kernel(const float *w, unsigned char *img, int I, int L, int nblk,
                                                       int transposed, unsigned pieces) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= pieces) return;
    const int lane = idx & 63, cbk = (idx >> 6) % nblk, kb = (idx >> 6) / nblk;
    const int n = cbk * 32 + (lane & 31), k0 = kb * OL_KB + 8 * (lane >> 5);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        v[e] = 0.f;
        if (transposed) {
            if (n < I && k < L) v[e] = w[(size_t)k * I + n];
        } else {
            if (n < L) v[e] = w[(size_t)n * I + k];
        }
    }
    bf16x8 f[3];
    split8(v, f);
    unsigned char *at = img + (size_t)kb * 3 * nblk * OL_FRAG + (size_t)cbk * OL_FRAG + lane * 16;
#pragma unroll
    for (int t = 0; t < 3; ++t) *reinterpret_cast<bf16x8 *>(at + (size_t)t * nblk * OL_FRAG) = f[t];
}

// a1 b1, then the corrections, the smallest first (wgrad_common.h)
constexpr int OL_PA[6] = {0, 2, 0, 1, 1, 0}, OL_PB[6] = {0, 0, 2, 1, 0, 1};

struct FwdArgs {
    const float *x;
    const unsigned char *wimg;
    const float *b;
    float *y;
    int rows, I, L, O, nkb;
    float scale;
    OutTables t;
};

// WIDE: x is 16-byte aligned (I is a multiple of 16 by the rule) and takes float4 loads
template <bool WIDE, int NB>
__global__ __launch_bounds__(256, 4) void out_fwd_kernel(const FwdArgs p) {
    __shared__ float zt[OL_RT / OL_WROWS][OL_WROWS * OL_ZS];
    __shared__ uint32_t tab[OL_TAB_WORDS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhalf = lane >> 5;
    if (tid < OL_TAB_WORDS) tab[tid] = reinterpret_cast<const uint32_t *>(&p.t)[tid];
    const int row0 = blockIdx.x * OL_RT + wave * OL_WROWS;
    const int I = p.I, nkb = p.nkb;
    const bool ok = row0 + l31 < p.rows;
    const float *xrow = p.x + (size_t)(ok ? row0 + l31 : 0) * I + 8 * lhalf;
    const unsigned char *bsrc = p.wimg + lane * 16;

    f32x16 acc[WG_ACC_SETS][NB];
#pragma unroll
    for (int s = 0; s < WG_ACC_SETS; ++s)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[s][j][e] = 0.f;

    auto loada = [&](int kb, float *v) {
        const float *at = xrow + kb * OL_KB;
        if (WIDE) {
            const float4 a = *reinterpret_cast<const float4 *>(at), b = *reinterpret_cast<const float4 *>(at + 4);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = at[e];
        }
    };
    auto loadb = [&](int kb, bf16x8 (*fb)[3]) {
        const unsigned char *at = bsrc + (size_t)kb * 3 * NB * OL_FRAG;
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int t = 0; t < 3; ++t) fb[j][t] = *reinterpret_cast<const bf16x8 *>(at + (t * NB + j) * OL_FRAG);
    };

    // the bias ahead of the loop, whose waits cover it (rnn_proj.hip)
    float bias[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) bias[j] = 32 * j + l31 < p.L ? p.b[32 * j + l31] : 0.f;

    // x of block kb + 1 is requested before the MFMAs of block kb (past the end: the last block again, never multiplied);
    // the weights' fragments come from L2 and the other waves of the SIMD (four: 128 registers) cover them
    float va[8], vn[8];
    loada(0, va);
    for (int kb = 0; kb < nkb; ++kb) {
        bf16x8 fb[NB][3];
        loadb(kb, fb);
        loada(kb + 1 < nkb ? kb + 1 : kb, vn);
        if (!ok) {
#pragma unroll
            for (int e = 0; e < 8; ++e) va[e] = 0.f;
        }
        bf16x8 fa[3];
        split8(va, fa);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int set = t > 0 ? WG_ACC_SETS - 1 : 0;
#pragma unroll
            for (int j = 0; j < NB; ++j)
                acc[set][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[OL_PA[t]], fb[j][OL_PB[t]], acc[set][j], 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) va[e] = vn[e];
    }

    // z[r][n] of accumulator register e sits at row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31
    float *zw = zt[wave];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = (e & 3) + 8 * (e >> 2) + 4 * lhalf;
            const float v = WG_ACC_SETS == 2 ? acc[0][j][e] + acc[WG_ACC_SETS - 1][j][e] : acc[0][j][e];
            zw[r * OL_ZS + 32 * j + l31] = v + bias[j];
        }
    __syncthreads();

    // the wave's rows of y are O (valid rows) contiguous floats
    const unsigned char *tb = reinterpret_cast<const unsigned char *>(tab);
    const int O = p.O;
    const int valid = p.rows - row0 < OL_WROWS ? p.rows - row0 : OL_WROWS;
    const int total = valid > 0 ? valid * O : 0;
    float *yw = p.y + (size_t)row0 * O;
    const float scale = p.scale;
    for (int i = lane; i < total; i += 64) {
        const int r = i / O, o = i - r * O;
        const float *zr = zw + r * OL_ZS;
        const float z = zr[tb[o]];
        const unsigned g = tb[64 + o];
        float v;
        if (g == OL_TANH) {
            v = scale * tanhf(z);
        } else {
            const int o0 = tb[128 + o], o1 = tb[192 + o];
            float mx = -INFINITY, sum = 0.f;
            for (int q = o0; q <= o1; ++q) mx = fmaxf(mx, zr[tb[q]]);
            for (int q = o0; q <= o1; ++q) sum += expf(zr[tb[q]] - mx);
            v = (z - mx) - logf(sum);
        }
        yw[i] = v;
    }
}

struct BwdArgs {
    const float *dy, *y;
    const unsigned char *wtimg;
    unsigned char *dzimg;
    float *dx;
    int rows, I, L, O, klb, cb;
    float scale;
    OutTables t;
};

template <int NB>
__global__ __launch_bounds__(128) void out_bwd_kernel(const BwdArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[OL_BWD_RT / OL_WROWS][2 * OL_WROWS * OL_MAXW];  // dy | y, then dz over both
    __shared__ uint32_t tab[OL_TAB_WORDS];
    static_assert(OL_WROWS * OL_ZS <= 2 * OL_WROWS * OL_MAXW, "dz fits where dy and y were");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhalf = lane >> 5;
    if (tid < OL_TAB_WORDS) tab[tid] = reinterpret_cast<const uint32_t *>(&p.t)[tid];
    const unsigned char *tb = reinterpret_cast<const unsigned char *>(tab);
    const int row0 = blockIdx.x * OL_BWD_RT + wave * OL_WROWS;
    const int O = p.O, L = p.L;
    const int valid = p.rows - row0 < OL_WROWS ? p.rows - row0 : OL_WROWS;
    const int total = valid > 0 ? valid * O : 0;
    // rows of dy and y in LDS are an odd number of floats apart (64 outputs: 64): lane = row reads without conflicts
    const int os = O < OL_MAXW ? (O | 1) : OL_MAXW;
    float *dyt = buf[wave], *yt = dyt + OL_WROWS * OL_MAXW, *dzt = buf[wave];

    const float *dyw = p.dy + (size_t)(valid > 0 ? row0 : 0) * O, *yw = p.y + (size_t)(valid > 0 ? row0 : 0) * O;
    for (int i = lane; i < OL_WROWS * O; i += 64) {
        const int r = i / O, o = i - r * O;
        const bool in = i < total;
        dyt[r * os + o] = in ? dyw[i] : 0.f;
        yt[r * os + o] = in ? yw[i] : 0.f;
    }
    __syncthreads();

    const float scale = p.scale;
    const float *dyr = dyt + l31 * os, *yr = yt + l31 * os;
    auto contrib = [&](int o) -> float {
        const float d = dyr[o], yv = yr[o];
        if (tb[64 + o] == OL_TANH) {
            const float t = yv / scale;         // exactly +-1 where y is +-scale: dz is exactly 0 there
            return d * (scale * fmaf(-t, t, 1.f));
        }
        float s = 0.f;
        for (int q = tb[128 + o]; q <= (int)tb[192 + o]; ++q) s += dyr[q];
        return d - expf(yv) * s;
    };
    float dzv[16 * NB];
#pragma unroll
    for (int j = 0; j < 16 * NB; ++j) {
        const int l = 2 * j + lhalf;
        const unsigned inv = l < L ? tb[256 + l] : OL_NONE;
        float v = 0.f;
        if (inv == OL_MANY) {
            for (int o = 0; o < O; ++o)
                if ((int)tb[o] == l) v += contrib(o);
        } else if (inv != OL_NONE) {
            v = contrib((int)inv);
        }
        dzv[j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16 * NB; ++j) dzt[l31 * OL_ZS + 2 * j + lhalf] = dzv[j];
    __syncthreads();
    if (valid <= 0) return;     // (no barrier below)

    // the fragments of dz^T for the weight gradient: 8 consecutive rows of column 32 nb + l31
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = dzt[(16 * h + 8 * lhalf + e) * OL_ZS + 32 * nb + l31];
            bf16x8 f[3];
            split8(v, f);
            unsigned char *at = p.dzimg + ((size_t)(row0 / OL_KB + h) * NB + nb) * 3 * OL_FRAG + lane * 16;
#pragma unroll
            for (int t = 0; t < 3; ++t) *reinterpret_cast<bf16x8 *>(at + t * OL_FRAG) = f[t];
        }
    if (!p.dx) return;

    // dx = dz w: the fragments of dz (row l31, 8 consecutive l) stay in registers, 64 columns of dx at a time
    constexpr int KLB = 2 * NB;
    bf16x8 fa[KLB][3];
#pragma unroll
    for (int kb = 0; kb < KLB; ++kb) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = dzt[l31 * OL_ZS + OL_KB * kb + 8 * lhalf + e];
        split8(v, fa[kb]);
    }
    const int cb = p.cb, klb = p.klb, I = p.I;
    for (int c0 = 0; c0 < cb; c0 += OL_DXC) {
        f32x16 acc[WG_ACC_SETS][OL_DXC];
#pragma unroll
        for (int s = 0; s < WG_ACC_SETS; ++s)
#pragma unroll
            for (int j = 0; j < OL_DXC; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[s][j][e] = 0.f;
        // every fragment of w^T the chunk needs is requested before its first MFMA (past cb or klb: the first one again)
        bf16x8 fb[KLB][OL_DXC][3];
#pragma unroll
        for (int kb = 0; kb < KLB; ++kb)
#pragma unroll
            for (int j = 0; j < OL_DXC; ++j) {
                const bool in = kb < klb && c0 + j < cb;
                const unsigned char *at = p.wtimg + ((size_t)(in ? kb : 0) * 3 * cb + (in ? c0 + j : 0)) * OL_FRAG + lane * 16;
#pragma unroll
                for (int t = 0; t < 3; ++t) fb[kb][j][t] = *reinterpret_cast<const bf16x8 *>(at + (size_t)t * cb * OL_FRAG);
            }
#pragma unroll
        for (int kb = 0; kb < KLB; ++kb) {
            if (kb >= klb) break;
#pragma unroll
            for (int j = 0; j < OL_DXC; ++j) {
                if (c0 + j >= cb) break;
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const int set = t > 0 ? WG_ACC_SETS - 1 : 0;
                    acc[set][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kb][OL_PA[t]], fb[kb][j][OL_PB[t]], acc[set][j], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < OL_DXC; ++j) {
            const int n = (c0 + j) * 32 + l31;
            if (c0 + j >= cb) break;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = row0 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
                const float v = WG_ACC_SETS == 2 ? acc[0][j][e] + acc[WG_ACC_SETS - 1][j][e] : acc[0][j][e];
                if (m < p.rows && n < I) p.dx[(size_t)m * I + n] = v;
            }
        }
    }
}

struct WgArgs {
    const unsigned char *dzimg;
    const float *x;
    float *part;
    int rows, I, L, run_rows, nw, wpg;
    size_t slab_floats;
};

// Wave blockIdx.y wpg + wave of a run owns 32 columns of [x | 1]: column I is the column of ones, whose product is db
template <int NB>
__global__ __launch_bounds__(OL_WG_WAVES * 64) void out_wgrad_kernel(const WgArgs p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhalf = lane >> 5;
    const int cbk = blockIdx.y * p.wpg + wave;
    if (cbk >= p.nw) return;    // (no barrier in this kernel)
    const int run = blockIdx.x, I = p.I, L = p.L;
    const int k0 = run * p.run_rows, k1 = min(k0 + p.run_rows, p.rows);
    const int nblk = (k1 - k0 + OL_KB - 1) / OL_KB, rb0 = k0 / OL_KB;      // (k0 is a multiple of 16)
    const int col = cbk * 32 + l31;
    const bool isx = col < I;
    const float fill = col == I ? 1.f : 0.f;
    const float *xcol = p.x + (isx ? col : 0);

    f32x16 acc[WG_ACC_SETS][NB];
#pragma unroll
    for (int s = 0; s < WG_ACC_SETS; ++s)
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[s][i][e] = 0.f;

    // 8 rows of the lane's column: each load of the wave is two whole 128-byte rows of x
    auto loadx = [&](int blk, float *v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int row = (rb0 + blk) * OL_KB + 8 * lhalf + e;
            v[e] = (isx && row < k1) ? xcol[(size_t)row * I] : fill;
        }
    };
    auto loada = [&](int blk, bf16x8 (*fa)[3]) {
        const unsigned char *at = p.dzimg + (size_t)(rb0 + blk) * NB * 3 * OL_FRAG + lane * 16;
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int t = 0; t < 3; ++t) fa[i][t] = *reinterpret_cast<const bf16x8 *>(at + (i * 3 + t) * OL_FRAG);
    };

    // block blk + 1 is requested before the MFMAs of block blk (past the end: the last block again, never multiplied)
    float v[8], vn[8];
    bf16x8 fa[NB][3], fan[NB][3];
    loadx(0, v);
    loada(0, fa);
    for (int blk = 0; blk < nblk; ++blk) {
        const int nx = blk + 1 < nblk ? blk + 1 : blk;
        loadx(nx, vn);
        loada(nx, fan);
        bf16x8 fx[3];
        split8(v, fx);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int set = t > 0 ? WG_ACC_SETS - 1 : 0;
#pragma unroll
            for (int i = 0; i < NB; ++i)
                acc[set][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][OL_PA[t]], fx[OL_PB[t]], acc[set][i], 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = vn[e];
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int t = 0; t < 3; ++t) fa[i][t] = fan[i][t];
    }

    // C[l][col] of accumulator register e sits at row l = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) of its block
    float *slab = p.part + (size_t)run * p.slab_floats;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int l = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
            const float r = WG_ACC_SETS == 2 ? acc[0][i][e] + acc[WG_ACC_SETS - 1][i][e] : acc[0][i][e];
            if (l < L && isx) slab[(size_t)l * I + col] = r;
            if (l < L && col == I) slab[(size_t)L * I + l] = r;
        }
}

// dw | db = the runs' partial results added in a fixed order: 32 entries a workgroup, the runs cut into OL_RED_SLICES
// consecutive pieces that eight groups of lanes add up side by side (a thread alone would wait for hundreds of loads one
// after the other), then the pieces' sums in their order
__global__ __launch_bounds__(32 * OL_RED_SLICES) void out_reduce_kernel(const float *part, size_t slab_floats, int runs,
                                                                        int LI, int L, float *dw, float *db) {
    __shared__ float sums[OL_RED_SLICES][32];
    const int idx = blockIdx.x * 32 + (threadIdx.x & 31), slice = threadIdx.x >> 5;
    const int per = (runs + OL_RED_SLICES - 1) / OL_RED_SLICES;
    const int r0 = slice * per, r1 = min(r0 + per, runs);
    float v = 0.f;
    if (idx < LI + L) {
#pragma unroll 8
        for (int r = r0; r < r1; ++r) v += part[(size_t)r * slab_floats + idx];
    }
    sums[slice][threadIdx.x & 31] = v;
    __syncthreads();
    if (slice != 0 || idx >= LI + L) return;
    v = sums[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < OL_RED_SLICES; ++q) v += sums[q][threadIdx.x];
    if (idx < LI)
        dw[idx] = v;
    else
        db[idx - LI] = v;
}

void put(uint32_t *words, size_t i, unsigned v) { words[i >> 2] |= (uint32_t)(v & 0xff) << (8 * (i & 3)); }

// the tables from the caller's two arrays (both NULL: the plain layer); false where they are not what the header says
bool out_tables(const int *src, const int *group, size_t L, size_t O, OutTables *t) {
    *t = OutTables{};
    if ((src == nullptr) != (group == nullptr)) return false;
    if (!src && O != L) return false;
    int s[OL_MAXW], g[OL_MAXW], count[OL_MAXW] = {0}, last[OL_MAXW];
    for (size_t o = 0; o < O; ++o) {
        s[o] = src ? src[o] : (int)o, g[o] = group ? group[o] : -1;
        if (s[o] < 0 || (size_t)s[o] >= L || g[o] < -1 || g[o] >= OL_MAXW) return false;
        ++count[s[o]], last[s[o]] = (int)o;
    }
    for (size_t o = 0; o < O; ++o) {
        size_t first = o, end = o;
        if (g[o] >= 0) {
            while (first > 0 && g[first - 1] == g[o]) --first;
            while (end + 1 < O && g[end + 1] == g[o]) ++end;
            for (size_t q = 0; q < O; ++q)
                if (g[q] == g[o] && (q < first || q > end)) return false;   // a group is one contiguous run
        }
        put(t->src, o, (unsigned)s[o]), put(t->grp, o, g[o] < 0 ? OL_TANH : (unsigned)g[o]);
        put(t->gfirst, o, (unsigned)first), put(t->glast, o, (unsigned)end);
    }
    for (size_t l = 0; l < (size_t)OL_MAXW; ++l)
        put(t->inv, l, l >= L || count[l] == 0 ? OL_NONE : count[l] > 1 ? OL_MANY : (unsigned)last[l]);
    return true;
}

bool out_prep(const float *w, unsigned char *img, size_t I, size_t L, int kblocks, int nblk, int transposed,
              hipStream_t stream) {
    const unsigned pieces = (unsigned)kblocks * nblk * 64;
    hipLaunchKernelGGL(out_prep_kernel, dim3((pieces + 255) / 256), dim3(256), 0, stream, w, img, (int)I, (int)L, nblk,
                       transposed, pieces);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

int out_layer_forward(const float *x, const float *w, const float *b, const int *src, const int *group, size_t rows,
                      size_t I, size_t L, size_t O, float scale, int cu_count, float *y, void *ws, size_t wsb,
                      hipStream_t stream) {
    if (!x || !w || !b || !y || !ws || !aligned16(ws)) return TK_ERR_BAD_ARG;
    if (!tk_out_layer_supported(I, L, O)) return TK_ERR_UNSUPPORTED;
    OutPlan p;
    if (!out_plan(rows, I, L, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    FwdArgs a;
    if (!out_tables(src, group, L, O, &a.t)) return TK_ERR_BAD_ARG;
    if (wsb < p.bytes) return TK_ERR_WORKSPACE;
    unsigned char *base = static_cast<unsigned char *>(ws);
    if (!out_prep(w, base, I, L, p.nkb, p.nb, 0, stream)) return TK_ERR_LAUNCH;
    a.x = x, a.wimg = base, a.b = b, a.y = y;
    a.rows = (int)rows, a.I = (int)I, a.L = (int)L, a.O = (int)O, a.nkb = p.nkb, a.scale = scale;
    const dim3 grid(p.tiles), block(256);
    if (aligned16(x)) {
        if (p.nb == 1)
            hipLaunchKernelGGL((out_fwd_kernel<true, 1>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((out_fwd_kernel<true, 2>), grid, block, 0, stream, a);
    } else {
        if (p.nb == 1)
            hipLaunchKernelGGL((out_fwd_kernel<false, 1>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((out_fwd_kernel<false, 2>), grid, block, 0, stream, a);
    }
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

int out_layer_backward(const float *dy, const float *y, const float *x, const float *w, const int *src, const int *group,
                       size_t rows, size_t I, size_t L, size_t O, float scale, int cu_count, float *dx, float *dw,
                       float *db, void *ws, size_t wsb, hipStream_t stream) {
    if (!dy || !y || !x || !w || !dw || !db || !ws || !aligned16(ws)) return TK_ERR_BAD_ARG;
    if (!tk_out_layer_supported(I, L, O)) return TK_ERR_UNSUPPORTED;
    OutPlan p;
    if (!out_plan(rows, I, L, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    BwdArgs a;
    if (!out_tables(src, group, L, O, &a.t)) return TK_ERR_BAD_ARG;
    if (wsb < p.bytes) return TK_ERR_WORKSPACE;
    unsigned char *base = static_cast<unsigned char *>(ws);
    if (dx && !out_prep(w, base + p.off_wt, I, L, p.klb, p.cb, 1, stream)) return TK_ERR_LAUNCH;
    a.dy = dy, a.y = y, a.wtimg = base + p.off_wt, a.dzimg = base + p.off_dz, a.dx = dx;
    a.rows = (int)rows, a.I = (int)I, a.L = (int)L, a.O = (int)O, a.klb = p.klb, a.cb = p.cb, a.scale = scale;
    const dim3 grid((unsigned)ceil_div(rows, OL_BWD_RT)), block(128);
    if (p.nb == 1)
        hipLaunchKernelGGL(out_bwd_kernel<1>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(out_bwd_kernel<2>, grid, block, 0, stream, a);
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    WgArgs g;
    g.dzimg = base + p.off_dz, g.x = x, g.part = reinterpret_cast<float *>(base + p.off_part);
    g.rows = (int)rows, g.I = (int)I, g.L = (int)L, g.run_rows = p.run_rows, g.slab_floats = p.slab_floats;
    const unsigned groups = (unsigned)ceil_div(p.nw, OL_WG_WAVES);      // the run's waves in workgroups of equal size
    g.nw = p.nw, g.wpg = (int)ceil_div(p.nw, groups);
    const dim3 wgrid(p.runs, groups), wblock(64 * g.wpg);
    if (p.nb == 1)
        hipLaunchKernelGGL(out_wgrad_kernel<1>, wgrid, wblock, 0, stream, g);
    else
        hipLaunchKernelGGL(out_wgrad_kernel<2>, wgrid, wblock, 0, stream, g);
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    const int LI = (int)(L * I);
    hipLaunchKernelGGL(out_reduce_kernel, dim3((LI + (int)L + 31) / 32), dim3(32 * OL_RED_SLICES), 0, stream, g.part, p.slab_floats,
                       p.runs, LI, (int)L, dw, db);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // namespace tk

extern "C" {

int tk_out_layer_supported(size_t I, size_t L, size_t O) {
    return tk::out_width_ok(I, L) && O >= L && O <= (size_t)tk::OL_MAXW ? 1 : 0;
}

size_t tk_out_layer_workspace_bytes(size_t rows, size_t I, size_t L, int cu_count) {
    tk::OutPlan p;
    return tk::out_plan(rows, I, L, cu_count, &p) ? p.bytes : 0;
}

int tk_out_layer_forward_dev(const float *x, const float *w, const float *b, const int *src, const int *group,
                             size_t rows, size_t I, size_t L, size_t O, float scale, int cu_count, float *y,
                             void *workspace, size_t workspace_bytes, void *stream) {
    return tk::out_layer_forward(x, w, b, src, group, rows, I, L, O, scale, cu_count, y, workspace, workspace_bytes,
                                 static_cast<hipStream_t>(stream));
}

int tk_out_layer_backward_dev(const float *dy, const float *y, const float *x, const float *w, const int *src,
                              const int *group, size_t rows, size_t I, size_t L, size_t O, float scale, int cu_count,
                              float *dx, float *dw, float *db, void *workspace, size_t workspace_bytes, void *stream) {
    return tk::out_layer_backward(dy, y, x, w, src, group, rows, I, L, O, scale, cu_count, dx, dw, db, workspace,
                                  workspace_bytes, static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
int tk_lab_out_layer_plan(size_t rows, size_t I, size_t L, size_t O, int cu_count, size_t *out) {
    tk::OutPlan p;
    if (!tk_out_layer_supported(I, L, O) || !tk::out_plan(rows, I, L, cu_count, &p)) return 0;
    const size_t v[7] = {(size_t)tk::OL_RT, (size_t)(32 * p.nb), (size_t)p.nkb, (size_t)p.tiles, (size_t)p.runs,
                         (size_t)p.run_rows, p.bytes};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    return 1;
}
#endif

}  // extern "C"

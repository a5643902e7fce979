// conv_strided.hip -- Convolution(16 -> Cout, window 19, stride 5, swish) of the mLstm models, forward and backward, on
// the bf16 matrix cores with every float32 operand split into three bf16 parts (include/taiyaki_amd_conv_strided.h;
// libtaiyaki_amd_conv_strided.so).  The split, the six products, the two accumulator sets and the fragment layouts are
// those of wgrad_common.h; the two GEMM bodies are rnn_proj.hip's proj_kernel and wgrad_common.h's wgrad_kernel with an
// address map in place of a row pitch, so that the window matrix (rows x 304, 124 MB at 4000 x 128) is never written.
//
// Rows are m = t N + n, t < Tout = ceil(T / 5).  Window t covers input times 5 t - 9 + j, tap j < 19.
//
// Forward (cs_gemm_kernel<CS_FWD>): k' = 16 j + c, so k block j of a row is the 16 channels of one input time: 64
// contiguous bytes of x at ((5 t - 9 + j) N + n) 16, zeros where that time is outside [0, T).  19 blocks, Cout columns.
// The epilogue adds the bias and writes z (where wanted) and y = z sigmoid(z).
// dx (cs_gemm_kernel<CS_DX>): the gather form.  Input time 5 u + r of column n, r < 5, lies in the windows u + d, d =
// -1 ... 2, at tap r - 5 d + 9 (d = 2 only for r >= 1).  Row (u, n) of this GEMM has the 80 outputs (r, c) and k =
// (d + 1) Cout + o: block kb reads 16 channels of dz at row m + d N (zeros outside [0, rows)), and the weights' image
// holds w[o][c][r - 5 d + 9], zero where that tap does not exist.  The windows of one input time are summed in
// ascending t, and the epilogue writes dx[(5 u + r) N + n][c] for 5 u + r < T: every element of dx once.
// Both walk k in ascending blocks inside one workgroup: a row's bits do not depend on N, T or the row's tile.
// dW, db (cs_wgrad_kernel): dW'[o][k'] = sum over rows of dz[row][o] window[row][k'], split-K over runs of rows, chains
// cut at WG_CHAIN, the first tile column adds up dz's columns (db); cs_reduce_kernel adds the partial results in their
// order and writes dW[o][c][j].  2 x 3 tiles of 128 x 128 (the last 48 wide): cu_count / 6 runs.
//
// The window, the stride and what follows from them are a template argument of every kernel (CsGeo); the text above is
// the geometry (19, 5), the one this library instantiates.  Compiled a second time with -DTK_CONV_WINDOW the same
// source is libtaiyaki_amd_conv_window.so (include/taiyaki_amd_conv_window.h): the entry points take the window and
// the stride as arguments, the geometries (31, 10) and (31, 12) are instantiated beside (19, 5), and Cout 96 and 128
// are admitted.  There input time S u + r lies in the windows u + d, d = -1 ... 2 as well, at tap r - S d + h: a dx row
// has 16 S = 160 or 192 outputs (two column tiles), a window 496 columns (dW: 4 tiles, the last 112 wide; 31 k blocks in
// the forward), and Cout 96 is one tile with 96 of its 128 columns (dW: rows) used.
#include "wgrad_common.h"

#ifdef TK_CONV_WINDOW
#include "../../include/taiyaki_amd_conv_window.h"
#else
#include "../../include/taiyaki_amd_conv_strided.h"
#endif

namespace tk {
namespace {

constexpr int CS_CIN = 16;
constexpr int CS_DXD = 4;                      // windows per input time: d = -1 ... 2

// a geometry: window 19, stride 5 has K = 304 and 80 outputs per row of the gather GEMM
template <int WIN_, int STRIDE_>
struct CsGeo {
    static constexpr int WIN = WIN_, STRIDE = STRIDE_, HALO = WIN_ / 2;
    static constexpr int K = CS_CIN * WIN_;            // columns of a window
    static constexpr int DXN = STRIDE_ * CS_CIN;       // outputs per row of the gather GEMM
    static_assert(WIN_ % 2 == 1, "the window is centred on its time");
    static_assert(DXN <= K, "an index into x is below rows x K (cs_plan's bound)");
    // input time S u + r, r < S, lies in no window before u - 1 (tap r + 2 S + h is past the last) or after u + 2
    // (tap r - 3 S + h is negative)
    static_assert(2 * STRIDE_ + HALO >= WIN_ && STRIDE_ - 1 - 3 * STRIDE_ + HALO < 0, "d = -1 ... 2 are all the windows");
};

// f(geometry) for the geometry (win, stride), where this library has it
template <class F>
bool cs_geometry(size_t win, size_t stride, F f) {
    if (win == 19 && stride == 5) return f(CsGeo<19, 5>()), true;
#ifdef TK_CONV_WINDOW
    if (win == 31 && stride == 10) return f(CsGeo<31, 10>()), true;
    if (win == 31 && stride == 12) return f(CsGeo<31, 12>()), true;
#endif
    return false;
}

// the projection geometry (rnn_proj.hip)
constexpr int PJ_RT = 128, PJ_NT = 128, PJ_KB = 16, PJ_THREADS = 256;
constexpr int PJ_A_HALF = 576;
constexpr int PJ_A_MB = 2 * PJ_A_HALF;
constexpr int PJ_A_PART = (PJ_RT / 32) * PJ_A_MB;
constexpr int PJ_A_PASSES = PJ_RT * (PJ_KB / 4) / PJ_THREADS;
constexpr int PJ_B_PART = (PJ_NT / 32) * 1024;
constexpr int PJ_B_BLOCK = 3 * PJ_B_PART;
constexpr int PJ_B_COPIES = PJ_B_BLOCK / 16 / PJ_THREADS;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
static_assert(PJ_B_COPIES * 16 * PJ_THREADS == PJ_B_BLOCK, "the B block is copied in whole passes");
static_assert(PJ_A_PASSES * PJ_THREADS == PJ_RT * (PJ_KB / 4), "the block of `a` is staged in whole passes");
static_assert(PJ_KB == CS_CIN, "one k block of the forward is one tap");

enum { CS_FWD = 0, CS_DX = 1 };

struct CsPlan {
    size_t rows;
    int tout, win, stride;
    // forward and dx GEMMs
    int tiles_m, f_tiles_n, f_nkb, f_grid, d_tiles_n, d_nkb, d_grid;
    // weight gradient
    int w_tiles_m, w_tiles_n, splits, nsub, run_rows, sub_rows, rstride, w_grid;
    size_t slab_floats, slabs;
    size_t off_dx, off_slabs, bytes;
};

bool cs_cout_ok(size_t cout) {
#ifdef TK_CONV_WINDOW
    if (cout == 96 || cout == 128) return true;
#endif
    return cout == 192 || cout == 256 || cout == 384;
}

bool cs_supported(size_t cin, size_t cout, size_t win, size_t stride) {
    return cin == CS_CIN && cs_cout_ok(cout) && cs_geometry(win, stride, [](auto) {});
}

bool cs_plan(size_t T, size_t N, size_t cout, size_t win, size_t stride, int cu_count, CsPlan *p) {
    if (T == 0 || N == 0 || cu_count <= 0 || !cs_supported(CS_CIN, cout, win, stride)) return false;
    if (T > (size_t(1) << 31) || N > (size_t(1) << 31)) return false;
    const size_t tout = ceil_div(T, stride), K = CS_CIN * win, dxn = CS_CIN * stride;
    // the kernels index in int: the widest row is a window (304 floats at window 19) or a row of z, dz (Cout floats);
    // a row of x's S input times is narrower than its window
    const size_t width = cout > K ? cout : K;
    if (tout > ((size_t(1) << 31) - 1) / width / N) return false;
    const size_t rows = tout * N;
    if (rows * width >= (size_t(1) << 31)) return false;
    p->rows = rows, p->tout = (int)tout, p->win = (int)win, p->stride = (int)stride;
    const size_t tm = ceil_div(rows, PJ_RT);
    p->tiles_m = (int)tm;
    p->f_tiles_n = (int)ceil_div(cout, PJ_NT), p->f_nkb = (int)win;
    p->d_tiles_n = (int)ceil_div(dxn, PJ_NT), p->d_nkb = (int)(CS_DXD * cout / PJ_KB);
    if (ceil_div(tm, 8) * 8 * p->f_tiles_n >= (size_t(1) << 31)) return false;
    p->f_grid = (int)(ceil_div(tm, 8) * 8 * p->f_tiles_n);
    p->d_grid = (int)(ceil_div(tm, 8) * 8 * p->d_tiles_n);
    // the weight gradient: wgrad_plan's rule
    const size_t wm = ceil_div(cout, WG_TILE), wn = ceil_div(K, WG_TILE);
    size_t G = g_lab_splits > 0 ? (size_t)g_lab_splits : (size_t)cu_count / (wm * wn);
    if (G < 1) G = 1;
    const size_t run = ceil_div(ceil_div(rows, G), WG_KB) * WG_KB;
    G = ceil_div(rows, run);
    const size_t nsub = ceil_div(run, WG_CHAIN);
    const size_t sub = ceil_div(ceil_div(run, nsub), WG_KB) * WG_KB;
    const size_t rstride = ceil_div(wm * G, 8) * 8;
    if (rstride * wn >= (size_t(1) << 31)) return false;
    p->w_tiles_m = (int)wm, p->w_tiles_n = (int)wn, p->splits = (int)G, p->nsub = (int)nsub;
    p->run_rows = (int)run, p->sub_rows = (int)sub, p->rstride = (int)rstride, p->w_grid = (int)(rstride * wn);
    p->slab_floats = (cout * K + cout + 3) / 4 * 4;
    p->slabs = G * nsub;
    p->off_dx = (size_t)p->f_tiles_n * p->f_nkb * PJ_B_BLOCK;
    p->off_slabs = p->off_dx + (size_t)p->d_tiles_n * p->d_nkb * PJ_B_BLOCK;
    p->bytes = p->off_slabs + p->slabs * p->slab_floats * sizeof(float);
    return true;
}

// B (nout x k) of one of the two GEMMs from w (Cout, 16, WIN), as proj_prep_kernel lays it out
template <class G>
__device__ __forceinline__ float cs_b(const float *w, int mode, int cout, int n, int k) {
    if (mode == CS_FWD) return n < cout ? w[(size_t)n * G::K + (k & 15) * G::WIN + (k >> 4)] : 0.f;
    if (n >= G::DXN) return 0.f;
    const int r = n >> 4, c = n & 15, d = k / cout - 1, o = k % cout;
    const int j = r - G::STRIDE * d + G::HALO;
    return j >= 0 && j < G::WIN ? w[(size_t)o * G::K + c * G::WIN + j] : 0.f;
}

template <class G>
__global__ __launch_bounds__(256) void cs_prep_kernel(const float *w, unsigned char *img, int mode, int cout, int nkb,
                                                      unsigned pieces) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= pieces) return;
    const int lane = idx & 63, nb = (idx >> 6) & 3, blk = idx >> 8;     // blk = column tile * nkb + k block
    const int n = (blk / nkb) * PJ_NT + nb * 32 + (lane & 31);
    const int k0 = (blk % nkb) * PJ_KB + 8 * (lane >> 5);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = cs_b<G>(w, mode, cout, n, k0 + e);
    uint4 p1, p2, p3;
    split2(v[0], v[1], p1.x, p2.x, p3.x);
    split2(v[2], v[3], p1.y, p2.y, p3.y);
    split2(v[4], v[5], p1.z, p2.z, p3.z);
    split2(v[6], v[7], p1.w, p2.w, p3.w);
    unsigned char *at = img + (size_t)blk * PJ_B_BLOCK + (size_t)(idx & 255) * 16;
    *reinterpret_cast<uint4 *>(at) = p1;
    *reinterpret_cast<uint4 *>(at + PJ_B_PART) = p2;
    *reinterpret_cast<uint4 *>(at + 2 * PJ_B_PART) = p3;
}

struct CsGemmArgs {
    const float *a;             // CS_FWD: x (T, N, 16); CS_DX: dz (rows, Cout)
    const unsigned char *bimg;
    const float *bias;          // CS_FWD
    float *out, *out2;          // CS_FWD: z (may be NULL), y; CS_DX: dx
    int M, N, T, cout;
    int tiles_m, tiles_n, nkb;
};

// proj_kernel (rnn_proj.hip) with `a` read through the map of MODE; every load of `a` is one float4
template <class G, int MODE>
__global__ __launch_bounds__(PJ_THREADS, 2) void cs_gemm_kernel(const CsGemmArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char imga[2][3 * PJ_A_PART];   // [buffer][part]
    __shared__ __attribute__((aligned(16))) unsigned char imgb[2][PJ_B_BLOCK];

    const float *asrc = p.a;
    const int M = p.M, N = p.N, nkb = p.nkb;
    const int grp = blockIdx.x / (8 * p.tiles_n), rem = blockIdx.x % (8 * p.tiles_n);
    const int nt = rem >> 3, mt = grp * 8 + (rem & 7);
    if (mt >= p.tiles_m) return;        // (the padding of the last group of eight)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhalf = lane >> 5;
    const int wmb = (wave >> 1) * 2, wnb = (wave & 1) * 2;

    const int q = tid & 3, r = tid >> 2;
    const int awoff = (r >> 5) * PJ_A_MB + (q >> 1) * PJ_A_HALF + (r & 31) * 16 + 8 * (q & 1);
    const int m_first = mt * PJ_RT + r;
    const u32x4 *bsrc = reinterpret_cast<const u32x4 *>(p.bimg + (size_t)nt * nkb * PJ_B_BLOCK) + tid;
    const int aroff = wmb * PJ_A_MB + lhalf * PJ_A_HALF + l31 * 16;
    const int broff = (wnb * 64 + lane) * 16;

    // the map of this thread's rows.  CS_FWD: the row's first input time S t - h and its column; CS_DX: the row itself
    int rowa[PJ_A_PASSES], rown[PJ_A_PASSES];
    bool mok[PJ_A_PASSES];
#pragma unroll
    for (int j = 0; j < PJ_A_PASSES; ++j) {
        const int m = m_first + 64 * j;
        mok[j] = m < M;
        if (MODE == CS_FWD) {
            const int t = m / N;
            rowa[j] = G::STRIDE * t - G::HALO, rown[j] = m - t * N;
        } else {
            rowa[j] = m, rown[j] = 0;
        }
    }
    const int kpd = p.cout / PJ_KB;     // CS_DX: k blocks per window

    f32x16 acc[WG_ACC_SETS][2][2];
#pragma unroll
    for (int s = 0; s < WG_ACC_SETS; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[s][i][j][e] = 0.f;

    float4 ra[2][PJ_A_PASSES];
    bool oka[2][PJ_A_PASSES];
    u32x4 rb[2][PJ_B_COPIES];

    // a block past the end, a row past the end and a block outside the input are fetched from element 0 and staged as
    // zeros
    auto fetch = [&](int kb, int set) {
        const bool kok = kb < nkb;
#pragma unroll
        for (int j = 0; j < PJ_A_PASSES; ++j) {
            int off;
            bool ok = mok[j] && kok;
            if (MODE == CS_FWD) {
                const int time = rowa[j] + kb;
                ok = ok && time >= 0 && time < p.T;
                off = (time * N + rown[j]) * CS_CIN + 4 * q;
            } else {
                const int row = rowa[j] + (kb / kpd - 1) * N;
                ok = ok && row >= 0 && row < M;
                off = row * p.cout + (kb % kpd) * PJ_KB + 4 * q;
            }
            oka[set][j] = ok;
            ra[set][j] = *reinterpret_cast<const float4 *>(asrc + (ok ? off : 0));
        }
        const int kbb = kok ? kb : nkb - 1;
#pragma unroll
        for (int c = 0; c < PJ_B_COPIES; ++c) rb[set][c] = bsrc[(size_t)kbb * (PJ_B_BLOCK / 16) + c * PJ_THREADS];
    };
    auto stash = [&](int set, int buf) {
#pragma unroll
        for (int j = 0; j < PJ_A_PASSES; ++j) {
            float4 v = ra[set][j];
            if (!oka[set][j]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            uint2 p1, p2, p3;
            split2(v.x, v.y, p1.x, p2.x, p3.x);
            split2(v.z, v.w, p1.y, p2.y, p3.y);
            unsigned char *at = &imga[buf][awoff + 2 * j * PJ_A_MB];
            *reinterpret_cast<uint2 *>(at) = p1;
            *reinterpret_cast<uint2 *>(at + PJ_A_PART) = p2;
            *reinterpret_cast<uint2 *>(at + 2 * PJ_A_PART) = p3;
        }
#pragma unroll
        for (int c = 0; c < PJ_B_COPIES; ++c) reinterpret_cast<u32x4 *>(imgb[buf])[tid + c * PJ_THREADS] = rb[set][c];
    };

    fetch(0, 0);
    fetch(1, 1);
    stash(0, 0);
    __syncthreads();
    for (int kb2 = 0; kb2 < nkb; kb2 += 2) {
#pragma unroll
        for (int cur = 0; cur < 2; ++cur) {     // block kb is in LDS buffer kb & 1 and came through register set kb & 1
            const int kb = kb2 + cur;
            if (kb >= nkb) break;
            fetch(kb + 2, cur);
            bf16x8 fa[2][3], fb[2][3];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    fa[i][t] = *reinterpret_cast<const bf16x8 *>(&imga[cur][t * PJ_A_PART + i * PJ_A_MB + aroff]);
                    fb[i][t] = *reinterpret_cast<const bf16x8 *>(&imgb[cur][t * PJ_B_PART + i * 1024 + broff]);
                }
            // a1 b1, then the corrections, the smallest first
            constexpr int PA[6] = {0, 2, 0, 1, 1, 0}, PB[6] = {0, 0, 2, 1, 0, 1};
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int set = t > 0 ? WG_ACC_SETS - 1 : 0;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[set][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][PA[t]], fb[j][PB[t]],
                                                                                  acc[set][i][j], 0, 0, 0);
            }
            stash(cur ^ 1, cur ^ 1);    // (its last readers passed the barrier of block kb - 1)
            __syncthreads();
        }
    }

    // C[m][n] of accumulator register e sits at row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = nt * PJ_NT + (wnb + j) * 32 + l31;
        const bool nok = n < (MODE == CS_FWD ? p.cout : G::DXN);
        const float b = (MODE == CS_FWD && nok) ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = mt * PJ_RT + (wmb + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
                const float v = WG_ACC_SETS == 2 ? acc[0][i][j][e] + acc[WG_ACC_SETS - 1][i][j][e] : acc[0][i][j][e];
                if (!nok || m >= M) continue;
                if (MODE == CS_FWD) {
                    const float z = v + b;
                    const size_t at = (size_t)m * p.cout + n;
                    if (p.out) p.out[at] = z;
                    p.out2[at] = z / (1.f + __expf(-z));
                } else {
                    const int u = m / N, col = m - u * N;
                    const int time = G::STRIDE * u + (n >> 4);
                    if (time < p.T) p.out[((size_t)time * N + col) * CS_CIN + (n & 15)] = v;
                }
            }
    }
}

// dz = dy (s + z s (1 - s)), s = sigmoid(z): four elements per thread
__global__ __launch_bounds__(256) void cs_dz_kernel(const float4 *dy, const float4 *z, float4 *dz, unsigned quads) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= quads) return;
    const float4 g = dy[idx], v = z[idx];
    auto f = [](float g, float z) {
        const float s = 1.f / (1.f + __expf(-z));
        return g * (s + z * s * (1.f - s));
    };
    dz[idx] = make_float4(f(g.x, v.x), f(g.y, v.y), f(g.z, v.z), f(g.w, v.w));
}

struct CsWgradArgs {
    const float *dz, *x;
    float *ws;
    int K, N, T, M;             // rows, columns of the batch, input times, Cout
    int tiles_m, splits, nsub, run_rows, sub_rows, rstride;
    size_t slab_floats;
};

// wgrad_kernel (wgrad_common.h) with its second operand, the windows in k' = 16 j + c order, read from x through the
// window map: this thread's four columns are four channels of one tap.  Every load is one float4.
template <class G>
__global__ __launch_bounds__(WG_THREADS) void cs_wgrad_kernel(const CsWgradArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char img[2][2][3][WG_IMAGE];    // [buffer][dz, windows][part]
    __shared__ __attribute__((aligned(16))) float colsum[WG_THREADS / 32][WG_TILE];

    const int tnx = blockIdx.x / a.rstride, q = blockIdx.x % a.rstride;
    if (q >= a.tiles_m * a.splits) return;      // (the padding of rstride)
    const int run = q % a.splits, tmx = q / a.splits;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhalf = lane >> 5;
    const int wm = (wave / (WG_THREADS / 128)) * 64, wn = (wave % (WG_THREADS / 128)) * 32 * WG_NJ;
    const int c4 = (tid & 31) * 4, r0 = tid >> 5;
    const int woff = 256 * r0 + 16 * (((tid & 31) >> 1) ^ ((r0 & 3) << 2)) + 8 * (tid & 1);
    const int tq = (lane >> 2) & 3, tp = lane & 3;
    int aoff[2], boff[WG_NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = 256 * (8 * lhalf + tq) + 8 * (tp & 1), chunk = 4 * i + 2 * ((lane >> 4) & 1) + (tp >> 1);
        aoff[i] = row + 16 * ((wm / 8 + chunk) ^ (tq << 2));
        if (i < WG_NJ) boff[i] = row + 16 * ((wn / 8 + chunk) ^ (tq << 2));
    }

    const int bcol0 = tnx * WG_TILE;
    const bool sum_cols = tnx == 0;
    const int acol = tmx * WG_TILE + c4, bcol = bcol0 + c4;
    const bool acok = acol < a.M, bcok = bcol < G::K;
    const int acl = acok ? acol : 0;
    const int tap = bcol >> 4, chan = bcol & 15;    // this thread's float4 of a window

    const int run_begin = run * a.run_rows;
    const int run_end = min(run_begin + a.run_rows, a.K);

    for (int sub = 0; sub < a.nsub; ++sub) {
        const int k0 = run_begin + sub * a.sub_rows;
        const int k1 = min(k0 + a.sub_rows, run_end);
        const int nkb = k1 > k0 ? (k1 - k0 + WG_KB - 1) / WG_KB : 0;

        f32x16 acc[WG_ACC_SETS][2][WG_NJ];
#pragma unroll
        for (int s = 0; s < WG_ACC_SETS; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < WG_NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[s][i][j][r] = 0.f;
        float4 dbacc = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 ra[2][WG_SPASS], rb[2][WG_SPASS];
        bool oka[2][WG_SPASS], okb[2][WG_SPASS];

        auto fetch = [&](int kb, int set) {
#pragma unroll
            for (int j = 0; j < WG_SPASS; ++j) {
                const int k = k0 + kb * WG_KB + r0 + WG_SROWS * j;
                const bool kok = k < k1;
                const int t = k / a.N, n = k - t * a.N;
                const int time = G::STRIDE * t - G::HALO + tap;
                oka[set][j] = kok && acok;
                okb[set][j] = kok && bcok && time >= 0 && time < a.T;
                ra[set][j] = load4<true>(a.dz, a.M, k, oka[set][j], acl);
                const int off = (time * a.N + n) * CS_CIN + chan;
                rb[set][j] = *reinterpret_cast<const float4 *>(a.x + (okb[set][j] ? off : 0));
            }
        };
        auto stash = [&](int set, int buf) {
#pragma unroll
            for (int j = 0; j < WG_SPASS; ++j) {
                float4 va = ra[set][j], vb = rb[set][j];
                if (!oka[set][j]) va = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!okb[set][j]) vb = make_float4(0.f, 0.f, 0.f, 0.f);
                stage4(&img[buf][0][0][woff + 256 * WG_SROWS * j], va);
                stage4(&img[buf][1][0][woff + 256 * WG_SROWS * j], vb);
                dbacc.x += va.x, dbacc.y += va.y, dbacc.z += va.z, dbacc.w += va.w;     // (used where sum_cols)
            }
        };

        fetch(0, 0);
        fetch(1, 1);
        stash(0, 0);
        __syncthreads();
        for (int kb2 = 0; kb2 < nkb; kb2 += 2) {
#pragma unroll
            for (int cur = 0; cur < 2; ++cur) {
                const int kb = kb2 + cur;
                fetch(kb + 2, cur);
                bf16x8 fa[2][3], fb[WG_NJ][3];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        fa[i][p] = frag(&img[cur][0][p][aoff[i]]);
                        if (i < WG_NJ) fb[i][p] = frag(&img[cur][1][p][boff[i]]);
                    }
                constexpr int PA[6] = {0, 2, 0, 1, 1, 0}, PB[6] = {0, 0, 2, 1, 0, 1};
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const int s = t > 0 ? WG_ACC_SETS - 1 : 0;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < WG_NJ; ++j)
                            acc[s][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][PA[t]], fb[j][PB[t]],
                                                                                    acc[s][i][j], 0, 0, 0);
                }
                stash(cur ^ 1, cur ^ 1);
                __syncthreads();
            }
        }

        // this partial result: [M][K] in k' order | [M]
        float *slab = a.ws + (size_t)(run * a.nsub + sub) * a.slab_floats;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < WG_NJ; ++j) {
                const int n = bcol0 + wn + 32 * j + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = tmx * WG_TILE + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    const float v = WG_ACC_SETS == 2 ? acc[0][i][j][r] + acc[WG_ACC_SETS - 1][i][j][r] : acc[0][i][j][r];
                    if (m < a.M && n < G::K) slab[(size_t)m * G::K + n] = v;
                }
            }
        if (sum_cols) {
            *reinterpret_cast<float4 *>(&colsum[r0][c4]) = dbacc;
            __syncthreads();
            if (tid < WG_TILE) {
                float v = colsum[0][tid];
#pragma unroll
                for (int r = 1; r < WG_THREADS / 32; ++r) v += colsum[r][tid];
                const int m = tmx * WG_TILE + tid;
                if (m < a.M) slab[(size_t)a.M * G::K + m] = v;
            }
        }
    }
}

// dw (Cout, 16, WIN) | db = the partial results added in their order
template <class G>
__global__ __launch_bounds__(256) void cs_reduce_kernel(const float *ws, size_t slab_floats, int slabs, int M, float *dw,
                                                        float *db) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    const unsigned MW = (unsigned)M * G::K;
    if (idx >= MW + M) return;
    float v = ws[idx];
#pragma unroll 4
    for (int p = 1; p < slabs; ++p) v += ws[(size_t)p * slab_floats + idx];
    if (idx >= MW) {
        db[idx - MW] = v;
        return;
    }
    const unsigned m = idx / G::K, k = idx % G::K;
    dw[(size_t)m * G::K + (k & 15) * G::WIN + (k >> 4)] = v;
}

template <class G>
int cs_launch_gemm(int mode, const CsPlan &p, const float *w, CsGemmArgs g, unsigned char *img, hipStream_t stream) {
    const int tiles_n = mode == CS_FWD ? p.f_tiles_n : p.d_tiles_n, nkb = mode == CS_FWD ? p.f_nkb : p.d_nkb;
    const unsigned pieces = (unsigned)(tiles_n * nkb) * (PJ_B_PART / 16);
    hipLaunchKernelGGL(cs_prep_kernel<G>, dim3((pieces + 255) / 256), dim3(256), 0, stream, w, img, mode, g.cout, nkb,
                       pieces);
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    g.bimg = img, g.tiles_m = p.tiles_m, g.tiles_n = tiles_n, g.nkb = nkb;
    if (mode == CS_FWD)
        hipLaunchKernelGGL((cs_gemm_kernel<G, CS_FWD>), dim3(p.f_grid), dim3(PJ_THREADS), 0, stream, g);
    else
        hipLaunchKernelGGL((cs_gemm_kernel<G, CS_DX>), dim3(p.d_grid), dim3(PJ_THREADS), 0, stream, g);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

// the backward's launches at one geometry
template <class G>
int cs_launch_backward(const CsPlan &p, const float *dy, const float *x, const float *z, const float *w, size_t T,
                       size_t N, size_t cout, float *dz, float *dx, float *dw, float *db, unsigned char *base,
                       hipStream_t stream) {
    const unsigned quads = (unsigned)(p.rows * cout / 4);
    hipLaunchKernelGGL(cs_dz_kernel, dim3((quads + 255) / 256), dim3(256), 0, stream,
                       reinterpret_cast<const float4 *>(dy), reinterpret_cast<const float4 *>(z),
                       reinterpret_cast<float4 *>(dz), quads);
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    if (dx) {
        CsGemmArgs g = {};
        g.a = dz, g.out = dx;
        g.M = (int)p.rows, g.N = (int)N, g.T = (int)T, g.cout = (int)cout;
        const int rc = cs_launch_gemm<G>(CS_DX, p, w, g, base + p.off_dx, stream);
        if (rc != TK_OK) return rc;
    }
    CsWgradArgs a;
    a.dz = dz, a.x = x, a.ws = reinterpret_cast<float *>(base + p.off_slabs);
    a.K = (int)p.rows, a.N = (int)N, a.T = (int)T, a.M = (int)cout;
    a.tiles_m = p.w_tiles_m, a.splits = p.splits, a.nsub = p.nsub, a.run_rows = p.run_rows, a.sub_rows = p.sub_rows;
    a.rstride = p.rstride, a.slab_floats = p.slab_floats;
    hipLaunchKernelGGL(cs_wgrad_kernel<G>, dim3(p.w_grid), dim3(WG_THREADS), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    const unsigned total = (unsigned)(cout * G::K + cout);
    hipLaunchKernelGGL(cs_reduce_kernel<G>, dim3((total + 255) / 256), dim3(256), 0, stream,
                       static_cast<const float *>(a.ws), p.slab_floats, (int)p.slabs, (int)cout, dw, db);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // namespace

int conv_strided_forward(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cout, size_t win,
                         size_t stride, int cu_count, float *z, float *y, void *ws, size_t wsb, hipStream_t stream) {
    if (!x || !w || !b || !y || !ws) return TK_ERR_BAD_ARG;
    if (!aligned16(x) || !aligned16(y) || !aligned16(z) || !aligned16(ws)) return TK_ERR_BAD_ARG;
    CsPlan p;
    if (!cs_plan(T, N, cout, win, stride, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    if (wsb < p.bytes) return TK_ERR_WORKSPACE;
    CsGemmArgs g = {};
    g.a = x, g.bias = b, g.out = z, g.out2 = y;
    g.M = (int)p.rows, g.N = (int)N, g.T = (int)T, g.cout = (int)cout;
    int rc = TK_ERR_UNSUPPORTED;
    cs_geometry(win, stride, [&](auto geo) {
        rc = cs_launch_gemm<decltype(geo)>(CS_FWD, p, w, g, static_cast<unsigned char *>(ws), stream);
    });
    return rc;
}

int conv_strided_backward(const float *dy, const float *x, const float *z, const float *w, size_t T, size_t N,
                          size_t cout, size_t win, size_t stride, int cu_count, float *dz, float *dx, float *dw,
                          float *db, void *ws, size_t wsb, hipStream_t stream) {
    if (!dy || !x || !z || !w || !dz || !dw || !db || !ws) return TK_ERR_BAD_ARG;
    if (!aligned16(dy) || !aligned16(x) || !aligned16(z) || !aligned16(dz) || !aligned16(dx) || !aligned16(ws))
        return TK_ERR_BAD_ARG;
    CsPlan p;
    if (!cs_plan(T, N, cout, win, stride, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    if (wsb < p.bytes) return TK_ERR_WORKSPACE;
    int rc = TK_ERR_UNSUPPORTED;
    cs_geometry(win, stride, [&](auto geo) {
        rc = cs_launch_backward<decltype(geo)>(p, dy, x, z, w, T, N, cout, dz, dx, dw, db,
                                               static_cast<unsigned char *>(ws), stream);
    });
    return rc;
}

#ifdef TK_LAB
// the lab hook's view of the plan
int cs_lab_plan(size_t T, size_t N, size_t cout, size_t win, size_t stride, int cu_count, size_t *out) {
    CsPlan p;
    if (!cs_plan(T, N, cout, win, stride, cu_count, &p)) return 0;
    const size_t v[12] = {(size_t)p.tiles_m, (size_t)p.f_tiles_n, (size_t)p.f_nkb, (size_t)p.f_grid,
                          (size_t)p.d_tiles_n, (size_t)p.d_nkb, (size_t)p.splits, (size_t)p.nsub,
                          (size_t)p.run_rows, (size_t)p.sub_rows, (size_t)p.w_grid, p.bytes};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return 1;
}
#endif

}  // namespace tk

extern "C" {

#ifndef TK_CONV_WINDOW

int tk_conv_strided_supported(size_t cin, size_t cout, size_t winlen, size_t stride) {
    return tk::cs_supported(cin, cout, winlen, stride);
}

size_t tk_conv_strided_workspace_bytes(size_t T, size_t N, size_t cout, int cu_count) {
    tk::CsPlan p;
    return tk::cs_plan(T, N, cout, 19, 5, cu_count, &p) ? p.bytes : 0;
}

int tk_conv_strided_forward_dev(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cout,
                                int cu_count, float *z, float *y, void *workspace, size_t workspace_bytes,
                                void *stream) {
    return tk::conv_strided_forward(x, w, b, T, N, cout, 19, 5, cu_count, z, y, workspace, workspace_bytes,
                                    static_cast<hipStream_t>(stream));
}

int tk_conv_strided_backward_dev(const float *dy, const float *x, const float *z, const float *w, size_t T, size_t N,
                                 size_t cout, int cu_count, float *dz, float *dx, float *dw, float *db,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    return tk::conv_strided_backward(dy, x, z, w, T, N, cout, 19, 5, cu_count, dz, dx, dw, db, workspace,
                                     workspace_bytes, static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
void tk_lab_conv_strided_set_splits(int splits) { tk::g_lab_splits = splits; }

int tk_lab_conv_strided_plan(size_t T, size_t N, size_t cout, int cu_count, size_t *out) {
    return tk::cs_lab_plan(T, N, cout, 19, 5, cu_count, out);
}
#endif

#else   // TK_CONV_WINDOW: include/taiyaki_amd_conv_window.h

int tk_conv_window_supported(size_t cin, size_t cout, size_t winlen, size_t stride) {
    return tk::cs_supported(cin, cout, winlen, stride);
}

size_t tk_conv_window_workspace_bytes(size_t T, size_t N, size_t cout, size_t winlen, size_t stride, int cu_count) {
    tk::CsPlan p;
    return tk::cs_plan(T, N, cout, winlen, stride, cu_count, &p) ? p.bytes : 0;
}

int tk_conv_window_forward_dev(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cout,
                               size_t winlen, size_t stride, int cu_count, float *z, float *y, void *workspace,
                               size_t workspace_bytes, void *stream) {
    return tk::conv_strided_forward(x, w, b, T, N, cout, winlen, stride, cu_count, z, y, workspace, workspace_bytes,
                                    static_cast<hipStream_t>(stream));
}

int tk_conv_window_backward_dev(const float *dy, const float *x, const float *z, const float *w, size_t T, size_t N,
                                size_t cout, size_t winlen, size_t stride, int cu_count, float *dz, float *dx, float *dw,
                                float *db, void *workspace, size_t workspace_bytes, void *stream) {
    return tk::conv_strided_backward(dy, x, z, w, T, N, cout, winlen, stride, cu_count, dz, dx, dw, db, workspace,
                                     workspace_bytes, static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
void tk_lab_conv_window_set_splits(int splits) { tk::g_lab_splits = splits; }

int tk_lab_conv_window_plan(size_t T, size_t N, size_t cout, size_t winlen, size_t stride, int cu_count, size_t *out) {
    return tk::cs_lab_plan(T, N, cout, winlen, stride, cu_count, out);
}
#endif

#endif  // TK_CONV_WINDOW

}  // extern "C"

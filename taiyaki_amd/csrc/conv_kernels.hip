// conv_kernels.hip -- the narrow Convolution layers at the head of the model (layers.Convolution with
// swish, stride 1; (Cin, Cout, winlen) = (1, 4, 5) and (4, 16, 5)) as fused gfx950 kernels.
//
// Tensors are time-major (T, N, C) float32, the weight is nn.Conv1d's (Cout, Cin, winlen), the padding is the
// layer's (winlen / 2, (winlen - 1) / 2) zeros:
//   z[t, n, co] = b[co] + sum_ci sum_k w[co, ci, k] x[t + k - winlen / 2, n, ci],   y = z sigmoid(z)
// These layers run on raw samples (T N = 512 000 positions at the flagship shape) with a 4 x 5 or 16 x 20
// weight: as GEMMs their weight gradients fill one macro tile (nine split-K workgroups on the whole chip).
//
// Arithmetic is double from the float32 inputs to ONE rounding of each output (y, dx, dW, db): the vector FP64 rate
// of this chip is half its FP32 rate, the work is 0.3 / 1 GFLOP per pass, and every result is then the float32
// number nearest to the exact one -- no float32 evaluation order, the GEMM path's included, can be closer.
//
// A lane owns one position (t, n) and CPL neighbouring output channels (4 forward: one float4 of y; 2 backward,
// for the registers); the Cout / CPL lanes of a position are neighbours, and so are the positions' n.  A wave's
// y store and dy load are then one contiguous run, its x loads contiguous too (the lanes of one position read
// the same address).  The lane's CPL x Cin x winlen weights stay in registers.
//
//   forward   pad + window + contraction + bias + swish; writes y only.  z is NOT stored: the backward
//             recomputes it from x and w (20 / 320 FMAs per position against 16 / 64 B written and read back).
//   backward  a workgroup walks tiles of ROWS time rows x 64 / G columns (G = Cout / 2).  Per tile: recompute z,
//             dz = dy swish'(z); dW and db accumulate in registers (2 x Cin x winlen + 2 doubles per lane); with
//             an input gradient wanted, the tile's first and last winlen / 2 rows are halo: dz of all ROWS goes
//             to LDS once, and dx[t] = sum_k sum_co dz[t - k + winlen / 2, co] w[co, ci, k] of the inner rows is
//             read from there (the weights for it sit in LDS too), one lane per (t, n, ci).  At the end the
//             accumulators are summed across the wave (xor butterfly over the lanes of one channel group) and
//             across the waves through LDS, and the workgroup writes ONE slab (dW | db, double).
//             conv_slab_sum_kernel adds the slabs, one wave per element, in a fixed order, and rounds.
// No atomics: grid and slab count depend on (T, N, CU count) only, so results are bit-identical run to run.
#include "dispatch.h"
#include "ff_common.h"

namespace tk {
namespace {

constexpr int CONV_THREADS = 256;
constexpr int CONV_WAVES = CONV_THREADS / WAVE;
constexpr int CONV_FWD_CPL = 4;         // output channels per lane, forward (one float4 of y)
constexpr int CONV_BWD_CPL = 2;         // and backward (one float2 of dy; 2 x Cin x winlen double accumulators)
constexpr int CONV_ROWS = 16;           // time rows of a backward tile, halo included
constexpr int CONV_BWD_PER_CU = 2;      // backward workgroups per CU
constexpr int CONV_FWD_PER_CU = 8;

// the winlen input rows under output (t, n); rows outside [0, T) are the padding's zeros
template <int CIN, int K>
__device__ __forceinline__ void load_window(const float *__restrict__ x, int t, int n, int T, int N, double (&xv)[K][CIN]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int tt = t + k - K / 2;
        const bool in = tt >= 0 && tt < T;
        const size_t pos = in ? (size_t)tt * N + n : 0;
        if constexpr (CIN == 4) {
            f4 q = {0.f, 0.f, 0.f, 0.f};
            if (in) q = *reinterpret_cast<const f4 *>(x + pos * 4);
            xv[k][0] = q.x, xv[k][1] = q.y, xv[k][2] = q.z, xv[k][3] = q.w;
        } else {
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) xv[k][ci] = in ? x[pos * CIN + ci] : 0.f;
        }
    }
}

// the lane's weights w[CPL g .. CPL g + CPL - 1][.][.] and biases
template <int CPL, int CIN, int K>
__device__ __forceinline__ void load_weights(const float *__restrict__ w, const float *__restrict__ b, int g,
                                             float (&wr)[CPL][CIN][K], float (&br)[CPL]) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        br[c] = b[g * CPL + c];
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int k = 0; k < K; ++k) wr[c][ci][k] = w[((g * CPL + c) * CIN + ci) * K + k];
    }
}

template <int CPL, int CIN, int K>
__device__ __forceinline__ void preactivation(const float (&wr)[CPL][CIN][K], const float (&br)[CPL],
                                              const double (&xv)[K][CIN], double (&z)[CPL]) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        double a = br[c];
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int k = 0; k < K; ++k) a = fma((double)wr[c][ci][k], xv[k][ci], a);
        z[c] = a;
    }
}

__device__ __forceinline__ double sigmoid(double z) { return 1.0 / (1.0 + exp(-z)); }

template <int CIN, int COUT, int K>
__global__ __launch_bounds__(CONV_THREADS) void conv_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                const float *__restrict__ b, int T, int N,
                                                                f4 *__restrict__ y) {
    constexpr int CPL = CONV_FWD_CPL, G = COUT / CPL;
    const unsigned total = (unsigned)T * (unsigned)N * G;
    const unsigned first = blockIdx.x * CONV_THREADS + threadIdx.x;
    const unsigned stride = gridDim.x * CONV_THREADS;       // a multiple of G: the lane keeps its channel group
    float wr[CPL][CIN][K], br[CPL];
    load_weights<CPL, CIN, K>(w, b, first % G, wr, br);
    for (unsigned i = first; i < total; i += stride) {
        const unsigned p = i / G;
        const int t = p / (unsigned)N, n = p - (unsigned)t * N;
        double xv[K][CIN], z[CPL];
        load_window<CIN, K>(x, t, n, T, N, xv);
        preactivation<CPL, CIN, K>(wr, br, xv, z);
        f4 out;
        out.x = (float)(z[0] * sigmoid(z[0])), out.y = (float)(z[1] * sigmoid(z[1]));
        out.z = (float)(z[2] * sigmoid(z[2])), out.w = (float)(z[3] * sigmoid(z[3]));
        y[i] = out;
    }
}

template <int CIN, int COUT, int K, bool DX>
struct ConvTile {
    static constexpr int G = COUT / CONV_BWD_CPL;
    static constexpr int NT = WAVE / G;                     // columns: one tile row is one wave
    static constexpr int HALO_LO = DX ? K - 1 - K / 2 : 0;  // rows before the inner ones whose dz dx needs
    static constexpr int TT = CONV_ROWS - (DX ? K - 1 : 0); // inner rows: those whose dW, db and dx the tile owns
    static constexpr int CS = COUT + (COUT > 4 ? 2 : 0);    // LDS doubles per position (padded against bank conflicts)
    static constexpr int SLAB = COUT * CIN * K + COUT;      // dW | db
    static constexpr int LDS_DZ = DX ? CONV_ROWS * NT * CS : 0;
    static constexpr int LDS_W = DX ? COUT * CIN * K : 0;   // the weights as (winlen, Cin, Cout), for dx
    static constexpr int LDS_RED = CONV_WAVES * SLAB;
    static constexpr int LDS = LDS_DZ + LDS_W > LDS_RED ? LDS_DZ + LDS_W : LDS_RED;     // doubles
};

template <int CIN, int COUT, int K, bool DX>
__global__ __launch_bounds__(CONV_THREADS, CONV_BWD_PER_CU) void conv_bwd_kernel(
    const float2 *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ b,
    int T, int N, int tiles_n, int ntiles, float *__restrict__ dx, double *__restrict__ slabs) {
    using Tile = ConvTile<CIN, COUT, K, DX>;
    constexpr int CPL = CONV_BWD_CPL, G = Tile::G, NT = Tile::NT, TT = Tile::TT, CS = Tile::CS, SLAB = Tile::SLAB;
    __shared__ __attribute__((aligned(16))) double lds[Tile::LDS];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const int g = lane % G, nl = lane / G;
    float wr[CPL][CIN][K], br[CPL];
    load_weights<CPL, CIN, K>(w, b, g, wr, br);
    if (DX) {
        // dx wants all Cout x Cin x winlen weights in every lane: LDS (as 320 uniform loads they would be hoisted
        // out of the loops into more scalar registers than there are)
        for (int e = threadIdx.x; e < COUT * CIN * K; e += CONV_THREADS) {
            const int co = e / (CIN * K), ci = (e / K) % CIN, k = e % K;
            lds[Tile::LDS_DZ + (k * CIN + ci) * COUT + co] = w[e];
        }
    }
    double dw[CPL][CIN][K], db[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        db[c] = 0.0;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int k = 0; k < K; ++k) dw[c][ci][k] = 0.0;
    }

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int t0 = (tile / tiles_n) * TT, n0 = (tile % tiles_n) * NT;
        const int n = n0 + nl;
        if (DX) __syncthreads();        // the previous tile's dx has been read out of LDS (first tile: the weights are in)
#pragma unroll 1
        for (int r = wave; r < CONV_ROWS; r += CONV_WAVES) {
            const int t = t0 - Tile::HALO_LO + r;
            const bool inner = r >= Tile::HALO_LO && r < Tile::HALO_LO + TT;
            double dz[CPL];
#pragma unroll
            for (int c = 0; c < CPL; ++c) dz[c] = 0.0;
            if (t >= 0 && t < T && n < N) {
                double xv[K][CIN], z[CPL];
                load_window<CIN, K>(x, t, n, T, N, xv);
                preactivation<CPL, CIN, K>(wr, br, xv, z);
                const float2 d = dy[((size_t)t * N + n) * G + g];
                const double dyv[CPL] = {d.x, d.y};
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    const double s = sigmoid(z[c]);
                    dz[c] = dyv[c] * (s + z[c] * s * (1.0 - s));
                }
                if (inner) {
#pragma unroll
                    for (int c = 0; c < CPL; ++c) {
                        db[c] += dz[c];
#pragma unroll
                        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                            for (int k = 0; k < K; ++k) dw[c][ci][k] = fma(dz[c], xv[k][ci], dw[c][ci][k]);
                    }
                }
            }
            if (DX) {
#pragma unroll
                for (int c = 0; c < CPL; ++c) lds[(r * NT + nl) * CS + g * CPL + c] = dz[c];
            }
        }
        if (DX) {
            __syncthreads();
            // one lane per (inner row o, column, ci); row o reads LDS rows o .. o + K - 1: dz at t - k + K / 2 is
            // row o + K - 1 - k.  The tap loop stays rolled (unrolled, all its LDS reads are issued ahead).
#pragma unroll 1
            for (int i = threadIdx.x; i < TT * NT * CIN; i += CONV_THREADS) {
                const int ci = i % CIN, c = (i / CIN) % NT, o = i / (CIN * NT);
                const int t = t0 + o, nn = n0 + c;
                if (t < T && nn < N) {
                    double a = 0.0;
#pragma unroll 1
                    for (int k = 0; k < K; ++k) {
                        const double *row = &lds[((o + K - 1 - k) * NT + c) * CS];
                        const double *wk = &lds[Tile::LDS_DZ + (k * CIN + ci) * COUT];
#pragma unroll
                        for (int co = 0; co < COUT; ++co) a = fma(row[co], wk[co], a);
                    }
                    dx[((size_t)t * N + nn) * CIN + ci] = (float)a;
                }
            }
        }
    }

    // wave: butterfly over the lanes of one channel group (lane distances G, 2 G, ... 32); workgroup: through LDS,
    // waves added in order.  Element order of a slab: dW as (Cout, Cin, winlen), then db.
    __syncthreads();
    double *red = lds + wave * SLAB;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double v = dw[c][ci][k];
#pragma unroll
                for (int off = G; off < WAVE; off <<= 1) v += __shfl_xor(v, off, WAVE);
                if (nl == 0) red[((g * CPL + c) * CIN + ci) * K + k] = v;
            }
        double v = db[c];
#pragma unroll
        for (int off = G; off < WAVE; off <<= 1) v += __shfl_xor(v, off, WAVE);
        if (nl == 0) red[COUT * CIN * K + g * CPL + c] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SLAB; e += CONV_THREADS) {
        double v = lds[e];
#pragma unroll
        for (int wv = 1; wv < CONV_WAVES; ++wv) v += lds[wv * SLAB + e];
        slabs[(size_t)blockIdx.x * SLAB + e] = v;
    }
}

// dW | db = the sum of the workgroups' slabs: one wave per element, lane l adds slabs l, l + 64, ... in order,
// then a butterfly -- the same order whatever the slabs held before and however the waves are scheduled
__global__ __launch_bounds__(CONV_THREADS) void conv_slab_sum_kernel(const double *__restrict__ slabs, int nslab, int slab,
                                                                     int nw, float *__restrict__ dw, float *__restrict__ db) {
    const int e = blockIdx.x * CONV_WAVES + threadIdx.x / WAVE;
    if (e >= slab) return;
    double v = 0.0;
    for (int s = lane_id(); s < nslab; s += WAVE) v += slabs[(size_t)s * slab + e];
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    if (lane_id() == 0) {
        if (e < nw) dw[e] = (float)v;
        else db[e - nw] = (float)v;
    }
}

struct ConvPlan {
    int tiles_n, ntiles;
    unsigned grid;
    size_t slab;        // elements (doubles)
};

// tile counts by the kernel's own constants; the grid (= slab count) is a function of (T, N, CU count) only
template <int CIN, int COUT, int K, bool DX>
ConvPlan conv_plan(size_t T, size_t N, int cu_count) {
    using Tile = ConvTile<CIN, COUT, K, DX>;
    ConvPlan p;
    p.tiles_n = (int)((N + Tile::NT - 1) / Tile::NT);
    p.ntiles = (int)((T + Tile::TT - 1) / Tile::TT) * p.tiles_n;
    const int cap = cu_count * CONV_BWD_PER_CU;
    p.grid = (unsigned)(p.ntiles < cap ? p.ntiles : cap);
    p.slab = Tile::SLAB;
    return p;
}

template <int CIN, int COUT, int K>
int conv_forward(const float *x, const float *w, const float *b, size_t T, size_t N, int cu_count, float *y,
                 hipStream_t stream) {
    const size_t total = T * N * (COUT / CONV_FWD_CPL);
    const size_t blocks = (total + CONV_THREADS - 1) / CONV_THREADS, cap = (size_t)cu_count * CONV_FWD_PER_CU;
    hipLaunchKernelGGL((conv_fwd_kernel<CIN, COUT, K>), dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(CONV_THREADS),
                       0, stream, x, w, b, (int)T, (int)N, reinterpret_cast<f4 *>(y));
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

template <int CIN, int COUT, int K>
int conv_backward(const float *dy, const float *x, const float *w, const float *b, size_t T, size_t N, int cu_count,
                  float *dx, float *dw, float *db, double *ws, size_t wsb, hipStream_t stream) {
    const ConvPlan p = dx ? conv_plan<CIN, COUT, K, true>(T, N, cu_count) : conv_plan<CIN, COUT, K, false>(T, N, cu_count);
    if (wsb < p.grid * p.slab * sizeof(double)) return TK_ERR_WORKSPACE;
    const float2 *dy2 = reinterpret_cast<const float2 *>(dy);
    if (dx)
        hipLaunchKernelGGL((conv_bwd_kernel<CIN, COUT, K, true>), dim3(p.grid), dim3(CONV_THREADS), 0, stream, dy2, x, w,
                           b, (int)T, (int)N, p.tiles_n, p.ntiles, dx, ws);
    else
        hipLaunchKernelGGL((conv_bwd_kernel<CIN, COUT, K, false>), dim3(p.grid), dim3(CONV_THREADS), 0, stream, dy2, x,
                           w, b, (int)T, (int)N, p.tiles_n, p.ntiles, dx, ws);
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    const int slab = (int)p.slab;
    hipLaunchKernelGGL(conv_slab_sum_kernel, dim3((slab + CONV_WAVES - 1) / CONV_WAVES), dim3(CONV_THREADS), 0, stream,
                       ws, (int)p.grid, slab, COUT * CIN * K, dw, db);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

// every element index of the kernels fits 32 bits
bool conv_size_ok(size_t T, size_t N, size_t cout) {
    return T <= (size_t)INT32_MAX && N <= (size_t)INT32_MAX && (N == 0 || T <= (size_t)INT32_MAX / N) &&
           T * N <= (size_t)INT32_MAX / cout;
}

}  // namespace

bool conv_small_supported(size_t cin, size_t cout, size_t winlen, size_t stride) {
    return stride == 1 && winlen == 5 && ((cin == 1 && cout == 4) || (cin == 4 && cout == 16));
}

// the slabs of the backward with an input gradient (its tiles have the fewest inner rows, so it has the most)
size_t conv_small_workspace_bytes(size_t T, size_t N, size_t cin, size_t cout, size_t winlen, int cu_count) {
    if (!conv_small_supported(cin, cout, winlen, 1) || T == 0 || N == 0 || cu_count <= 0 || !conv_size_ok(T, N, cout))
        return 0;
    const ConvPlan p = cin == 1 ? conv_plan<1, 4, 5, true>(T, N, cu_count) : conv_plan<4, 16, 5, true>(T, N, cu_count);
    return p.grid * p.slab * sizeof(double);
}

int conv_small_forward_dispatch(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cin,
                                size_t cout, size_t winlen, int cu_count, float *y, hipStream_t stream) {
    if (!x || !w || !b || !y || cu_count <= 0 || !aligned16(x) || !aligned16(y)) return TK_ERR_BAD_ARG;
    if (!conv_small_supported(cin, cout, winlen, 1) || !conv_size_ok(T, N, cout)) return TK_ERR_UNSUPPORTED;
    if (T == 0 || N == 0) return TK_OK;
    return cin == 1 ? conv_forward<1, 4, 5>(x, w, b, T, N, cu_count, y, stream)
                    : conv_forward<4, 16, 5>(x, w, b, T, N, cu_count, y, stream);
}

int conv_small_backward_dispatch(const float *dy, const float *x, const float *w, const float *b, size_t T, size_t N,
                                 size_t cin, size_t cout, size_t winlen, int cu_count, float *dx, float *dw, float *db,
                                 void *ws, size_t wsb, hipStream_t stream) {
    if (!dy || !x || !w || !b || !dw || !db || !ws || cu_count <= 0 || !aligned16(dy) || !aligned16(x) ||
        !aligned16(dx) || !aligned16(ws))
        return TK_ERR_BAD_ARG;
    if (!conv_small_supported(cin, cout, winlen, 1) || !conv_size_ok(T, N, cout)) return TK_ERR_UNSUPPORTED;
    if (T == 0 || N == 0) return TK_ERR_BAD_ARG;        // (dW and db would be sums over nothing)
    return cin == 1 ? conv_backward<1, 4, 5>(dy, x, w, b, T, N, cu_count, dx, dw, db, static_cast<double *>(ws), wsb, stream)
                    : conv_backward<4, 16, 5>(dy, x, w, b, T, N, cu_count, dx, dw, db, static_cast<double *>(ws), wsb,
                                              stream);
}

}  // namespace tk

// conv_signal.hip -- Convolution(1 -> Cout, window 19, stride s, tanh) on the raw signal, the mGru models' first layer,
// forward and backward as plain float32 FMA kernels (include/taiyaki_amd_conv_signal.h; libtaiyaki_amd_conv_signal.so).
// 19 FMAs and one tanh per output: the passes move y (and dy) once and are bound by issue as much as by that traffic.
//
// Rows are (t, n), t < Tout = ceil(T / s); window t covers input times s t - 9 + k, tap k < 19.
//
// Layout (both kernels).  A lane owns four consecutive channels, Cout / 4 lanes cover a row, a workgroup of Cout / 4 x RP
// lanes works on RP rows at a time and walks tiles of tt x nt rows (nt = min(N, 16) columns, tt = 64 / nt window
// positions; tile index = blockIdx + i gridDim).  The tile's signal, (s (tt - 1) + 19) x nt floats with zeros outside
// [0, T) x [0, N), is staged once in LDS; the lanes of a row read a tap by broadcast.
// Forward: the lane's 76 weights sit in registers (staged through LDS: coalesced global reads, 19 ds_read_b128 per lane
// at a 304-byte pitch, which no 16-lane group conflicts on).  acc = b, then k = 0 ... 18 in order, tanh, one float4 store.
// Backward: dz = dy (1 - y^2) from two float4 loads, 76 + 4 accumulators in registers over every row the lane visits;
// then the RP lanes that own the same channels add their accumulators into one LDS image, row group 0, 1, ... in turn,
// and the workgroup writes that image, [20][Cout] (tap-major, row 19 = db), as its partial result.
// sg_reduce_kernel adds the G partial results: 16 runs of ceil(G / 16) consecutive partial results, each in index order,
// then the 16 sums in index order, and writes dw[c][k] and db[c].
#include "dispatch.h"

#include "../../include/taiyaki_amd_conv_signal.h"

namespace tk {
namespace {

constexpr int SG_WIN = 19, SG_HALO = 9, SG_MAX_STRIDE = 8;
constexpr int SG_NT = 16;           // columns of a tile, at most
constexpr int SG_TILE_ROWS = 64;    // rows of a tile, at most
constexpr int SG_XS = SG_MAX_STRIDE * SG_TILE_ROWS + (SG_WIN - 1) * SG_NT;  // floats of a tile's signal, at most (800)
constexpr int SG_FWD_PER_CU = 4, SG_BWD_PER_CU = 2;     // workgroups per CU of a full grid
constexpr int SG_RUNS = 16;         // runs of partial results in the reduction
constexpr int SG_RED_THREADS = 256;

// rows a workgroup works on at a time: Cout / 4 * RP = 256 or 192 lanes, whole waves
constexpr int sg_rp(int cout) { return cout <= 32 ? 32 : cout <= 64 ? 16 : cout <= 128 ? 8 : cout <= 256 ? 4 : 2; }

struct SgPlan {
    int rows, tout, nt, tt, tiles_n, ntiles, fgrid, bgrid;
    size_t bytes;
};

bool sg_cout_ok(size_t c) {
    return c == 32 || c == 64 || c == 96 || c == 128 || c == 192 || c == 256 || c == 384;
}

bool sg_plan(size_t T, size_t N, size_t cout, size_t stride, int cu_count, SgPlan *p) {
    if (!sg_cout_ok(cout) || stride < 1 || stride > SG_MAX_STRIDE || T == 0 || N == 0 || cu_count < 1) return false;
    const size_t lim = (size_t)1 << 31;
    const size_t tout = (T - 1) / stride + 1;
    if (tout >= lim || N >= lim) return false;
    const size_t rows = tout * N;
    if (rows >= lim || rows * cout >= lim) return false;
    p->rows = (int)rows, p->tout = (int)tout;
    p->nt = N < (size_t)SG_NT ? (int)N : SG_NT;
    p->tt = SG_TILE_ROWS / p->nt;
    p->tiles_n = (int)((N + p->nt - 1) / p->nt);
    const size_t ntiles = (size_t)p->tiles_n * ((tout + p->tt - 1) / p->tt);
    p->ntiles = (int)ntiles;
    const size_t cus = (size_t)(cu_count > 4096 ? 4096 : cu_count);
    p->fgrid = (int)(ntiles < cus * SG_FWD_PER_CU ? ntiles : cus * SG_FWD_PER_CU);
    p->bgrid = (int)(ntiles < cus * SG_BWD_PER_CU ? ntiles : cus * SG_BWD_PER_CU);
    p->bytes = (size_t)p->bgrid * cout * (SG_WIN + 1) * sizeof(float);
    return true;
}

struct SgArgs {
    const float *x;
    int T, N, tout, stride, nt, tt, tiles_n, ntiles;
};

// 1 - 2 / (e^(2 |z|) + 1) with z's sign, on the hardware's exp2 and reciprocal (a dozen instructions: with four of them
// per 76 FMAs a library tanh would bound the kernel): e^(2 |z|) overflows to +inf, its reciprocal is 0 and the result
// exactly 1; a NaN stays one.  Below 1/8, where that form cancels, the odd series to z^7 (the next term is below 2e-9
// of the result)
__device__ __forceinline__ float sg_tanh(float z) {
    const float a = fabsf(z), q = z * z;
    const float big = 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * a) + 1.0f);
    const float small = a * fmaf(q, fmaf(q, fmaf(q, -17.0f / 315.0f, 2.0f / 15.0f), -1.0f / 3.0f), 1.0f);
    return copysignf(a < 0.125f ? small : big, z);
}

// the signal of tile (t0, n0): xs[(time - (s t0 - 9)) nt + (n - n0)], zeros outside the tensor
__device__ __forceinline__ void sg_stage(const SgArgs &a, int t0, int n0, float *xs, int tid, int threads) {
    const int ntimes = a.stride * (a.tt - 1) + SG_WIN, base = a.stride * t0 - SG_HALO;
    for (int i = tid; i < ntimes * a.nt; i += threads) {
        const int tl = i / a.nt, nl = i - tl * a.nt;
        const int time = base + tl, n = n0 + nl;
        xs[i] = (time >= 0 && time < a.T && n < a.N) ? a.x[(size_t)time * a.N + n] : 0.0f;
    }
}

template <int COUT>
__global__ __launch_bounds__(COUT / 4 * sg_rp(COUT)) void sg_fwd_kernel(SgArgs a, const float *__restrict__ w,
                                                                         const float *__restrict__ b,
                                                                         float *__restrict__ y) {
    constexpr int L = COUT / 4, RP = sg_rp(COUT), THREADS = L * RP;
    __shared__ __attribute__((aligned(16))) float wl[COUT * SG_WIN];
    __shared__ __attribute__((aligned(16))) float xs[SG_XS];
    const int tid = threadIdx.x, lc = tid % L, rg = tid / L;

    for (int i = tid; i < COUT * SG_WIN; i += THREADS) wl[i] = w[i];
    __syncthreads();
    float wf[4 * SG_WIN];       // wf[j * 19 + k] = w[4 lc + j][k]
#pragma unroll
    for (int i = 0; i < SG_WIN; ++i) {
        const float4 v = *reinterpret_cast<const float4 *>(&wl[lc * 4 * SG_WIN + 4 * i]);
        wf[4 * i] = v.x, wf[4 * i + 1] = v.y, wf[4 * i + 2] = v.z, wf[4 * i + 3] = v.w;
    }
    const float b0 = b[4 * lc], b1 = b[4 * lc + 1], b2 = b[4 * lc + 2], b3 = b[4 * lc + 3];

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int tile_t = tile / a.tiles_n, t0 = tile_t * a.tt, n0 = (tile - tile_t * a.tiles_n) * a.nt;
        __syncthreads();        // (the tile before is read to its end)
        sg_stage(a, t0, n0, xs, tid, THREADS);
        __syncthreads();
        for (int r = rg; r < a.tt * a.nt; r += RP) {
            const int tl = r / a.nt, nl = r - tl * a.nt;
            const int t = t0 + tl, n = n0 + nl;
            if (t >= a.tout || n >= a.N) continue;
            const float *xr = xs + a.stride * tl * a.nt + nl;
            float xv[SG_WIN];
#pragma unroll
            for (int k = 0; k < SG_WIN; ++k) xv[k] = xr[k * a.nt];
            float z0 = b0, z1 = b1, z2 = b2, z3 = b3;
#pragma unroll
            for (int k = 0; k < SG_WIN; ++k) {
                z0 = fmaf(wf[k], xv[k], z0);
                z1 = fmaf(wf[SG_WIN + k], xv[k], z1);
                z2 = fmaf(wf[2 * SG_WIN + k], xv[k], z2);
                z3 = fmaf(wf[3 * SG_WIN + k], xv[k], z3);
            }
            const float4 out = make_float4(sg_tanh(z0), sg_tanh(z1), sg_tanh(z2), sg_tanh(z3));
            *reinterpret_cast<float4 *>(&y[((size_t)t * a.N + n) * COUT + 4 * lc]) = out;
        }
    }
}

template <int COUT>
__global__ __launch_bounds__(COUT / 4 * sg_rp(COUT)) void sg_bwd_kernel(SgArgs a, const float *__restrict__ dy,
                                                                         const float *__restrict__ y,
                                                                         float *__restrict__ ws) {
    constexpr int L = COUT / 4, RP = sg_rp(COUT), THREADS = L * RP, SLAB = COUT * (SG_WIN + 1);
    __shared__ __attribute__((aligned(16))) float red[SLAB];
    __shared__ __attribute__((aligned(16))) float xs[SG_XS];
    const int tid = threadIdx.x, lc = tid % L, rg = tid / L;

    float acc[4 * SG_WIN];      // acc[j * 19 + k]: channel 4 lc + j, tap k
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
    for (int i = 0; i < 4 * SG_WIN; ++i) acc[i] = 0.0f;

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int tile_t = tile / a.tiles_n, t0 = tile_t * a.tt, n0 = (tile - tile_t * a.tiles_n) * a.nt;
        __syncthreads();
        sg_stage(a, t0, n0, xs, tid, THREADS);
        __syncthreads();
        for (int r = rg; r < a.tt * a.nt; r += RP) {
            const int tl = r / a.nt, nl = r - tl * a.nt;
            const int t = t0 + tl, n = n0 + nl;
            if (t >= a.tout || n >= a.N) continue;
            const size_t at = ((size_t)t * a.N + n) * COUT + 4 * lc;
            const float4 g = *reinterpret_cast<const float4 *>(&dy[at]);
            const float4 v = *reinterpret_cast<const float4 *>(&y[at]);
            const float d0 = g.x * (1.0f - v.x * v.x), d1 = g.y * (1.0f - v.y * v.y);
            const float d2 = g.z * (1.0f - v.z * v.z), d3 = g.w * (1.0f - v.w * v.w);
            s0 += d0, s1 += d1, s2 += d2, s3 += d3;
            const float *xr = xs + a.stride * tl * a.nt + nl;
#pragma unroll
            for (int k = 0; k < SG_WIN; ++k) {
                const float xk = xr[k * a.nt];
                acc[k] = fmaf(d0, xk, acc[k]);
                acc[SG_WIN + k] = fmaf(d1, xk, acc[SG_WIN + k]);
                acc[2 * SG_WIN + k] = fmaf(d2, xk, acc[2 * SG_WIN + k]);
                acc[3 * SG_WIN + k] = fmaf(d3, xk, acc[3 * SG_WIN + k]);
            }
        }
    }

    // the row groups' accumulators, group 0, 1, ... in turn: red[k][4 lc + j]
    for (int turn = 0; turn < RP; ++turn) {
        if (rg == turn) {
            float4 *mine = reinterpret_cast<float4 *>(&red[4 * lc]);
#pragma unroll
            for (int k = 0; k <= SG_WIN; ++k) {
                float4 v = make_float4(s0, s1, s2, s3);
                if (k < SG_WIN) v = make_float4(acc[k], acc[SG_WIN + k], acc[2 * SG_WIN + k], acc[3 * SG_WIN + k]);
                if (turn > 0) {
                    const float4 o = mine[k * L];
                    v.x += o.x, v.y += o.y, v.z += o.z, v.w += o.w;
                }
                mine[k * L] = v;
            }
        }
        __syncthreads();
    }
    float *slab = ws + (size_t)blockIdx.x * SLAB;
    for (int i = tid; i < SLAB; i += THREADS) slab[i] = red[i];
}

// dw (Cout, 1, 19) and db (Cout) = the G partial results [20][Cout] added up: thread (run q, output j) adds run q's
// partial results in index order, then the runs' sums are added q = 0 ... 15
__global__ __launch_bounds__(SG_RED_THREADS) void sg_reduce_kernel(const float *__restrict__ ws, int G, int cout,
                                                                    float *__restrict__ dw, float *__restrict__ db) {
    constexpr int OUTS = SG_RED_THREADS / SG_RUNS;      // 16 outputs per workgroup
    __shared__ float part[SG_RUNS][OUTS];
    const int j = threadIdx.x % OUTS, q = threadIdx.x / OUTS;
    const int slab = cout * (SG_WIN + 1), idx = blockIdx.x * OUTS + j;      // (slab is a multiple of OUTS)
    const int per = (G + SG_RUNS - 1) / SG_RUNS;
    const int g0 = q * per, g1 = g0 + per < G ? g0 + per : G;
    float v = 0.0f;
#pragma unroll 8
    for (int g = g0; g < g1; ++g) v += ws[(size_t)g * slab + idx];
    part[q][j] = v;
    __syncthreads();
    if (q == 0) {
        v = part[0][j];
#pragma unroll
        for (int r = 1; r < SG_RUNS; ++r) v += part[r][j];
        const int k = idx / cout, c = idx - k * cout;
        if (k < SG_WIN)
            dw[c * SG_WIN + k] = v;
        else
            db[c] = v;
    }
}

SgArgs sg_args(const float *x, size_t T, size_t N, size_t stride, const SgPlan &p) {
    SgArgs a;
    a.x = x, a.T = (int)T, a.N = (int)N, a.tout = p.tout, a.stride = (int)stride;
    a.nt = p.nt, a.tt = p.tt, a.tiles_n = p.tiles_n, a.ntiles = p.ntiles;
    return a;
}

int conv_signal_forward(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cout, size_t stride,
                        int cu_count, float *y, hipStream_t stream) {
    if (!x || !w || !b || !y) return TK_ERR_BAD_ARG;
    if (!aligned16(y) || (reinterpret_cast<uintptr_t>(x) & 3)) return TK_ERR_BAD_ARG;
    SgPlan p;
    if (!sg_plan(T, N, cout, stride, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    const SgArgs a = sg_args(x, T, N, stride, p);
#define SG_FWD(C)                                                                                                     \
    case C:                                                                                                           \
        hipLaunchKernelGGL(sg_fwd_kernel<C>, dim3(p.fgrid), dim3(C / 4 * sg_rp(C)), 0, stream, a, w, b, y);            \
        break;
    switch (cout) {
        SG_FWD(32) SG_FWD(64) SG_FWD(96) SG_FWD(128) SG_FWD(192) SG_FWD(256) SG_FWD(384)
    default:
        return TK_ERR_UNSUPPORTED;
    }
#undef SG_FWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

int conv_signal_backward(const float *dy, const float *x, const float *y, size_t T, size_t N, size_t cout,
                         size_t stride, int cu_count, float *dw, float *db, void *ws, size_t wsb,
                         hipStream_t stream) {
    if (!dy || !x || !y || !dw || !db || !ws) return TK_ERR_BAD_ARG;
    if (!aligned16(dy) || !aligned16(y) || !aligned16(ws) || (reinterpret_cast<uintptr_t>(x) & 3))
        return TK_ERR_BAD_ARG;
    SgPlan p;
    if (!sg_plan(T, N, cout, stride, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    if (wsb < p.bytes) return TK_ERR_WORKSPACE;
    const SgArgs a = sg_args(x, T, N, stride, p);
    float *slabs = static_cast<float *>(ws);
#define SG_BWD(C)                                                                                                     \
    case C:                                                                                                           \
        hipLaunchKernelGGL(sg_bwd_kernel<C>, dim3(p.bgrid), dim3(C / 4 * sg_rp(C)), 0, stream, a, dy, y, slabs);       \
        break;
    switch (cout) {
        SG_BWD(32) SG_BWD(64) SG_BWD(96) SG_BWD(128) SG_BWD(192) SG_BWD(256) SG_BWD(384)
    default:
        return TK_ERR_UNSUPPORTED;
    }
#undef SG_BWD
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    const int outs = (int)cout * (SG_WIN + 1);
    hipLaunchKernelGGL(sg_reduce_kernel, dim3(outs / (SG_RED_THREADS / SG_RUNS)), dim3(SG_RED_THREADS), 0, stream,
                       static_cast<const float *>(slabs), p.bgrid, (int)cout, dw, db);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // namespace
}  // namespace tk

extern "C" {

int tk_conv_signal_supported(size_t cin, size_t cout, size_t winlen, size_t stride) {
    return cin == 1 && winlen == tk::SG_WIN && stride >= 1 && stride <= tk::SG_MAX_STRIDE && tk::sg_cout_ok(cout);
}

size_t tk_conv_signal_workspace_bytes(size_t T, size_t N, size_t cout, size_t stride, int cu_count) {
    tk::SgPlan p;
    return tk::sg_plan(T, N, cout, stride, cu_count, &p) ? p.bytes : 0;
}

int tk_conv_signal_forward_dev(const float *x, const float *w, const float *b, size_t T, size_t N, size_t cout,
                               size_t stride, int cu_count, float *y, void *stream) {
    return tk::conv_signal_forward(x, w, b, T, N, cout, stride, cu_count, y, static_cast<hipStream_t>(stream));
}

int tk_conv_signal_backward_dev(const float *dy, const float *x, const float *y, size_t T, size_t N, size_t cout,
                                size_t stride, int cu_count, float *dw, float *db, void *workspace,
                                size_t workspace_bytes, void *stream) {
    return tk::conv_signal_backward(dy, x, y, T, N, cout, stride, cu_count, dw, db, workspace, workspace_bytes,
                                    static_cast<hipStream_t>(stream));
}

}  // extern "C"

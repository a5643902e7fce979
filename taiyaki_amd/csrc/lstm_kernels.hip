// lstm_kernels.hip -- the recurrence of layers.Lstm (one nn.LSTM layer, gate order i, f, g, o; h0 = c0 = 0)
// as one persistent, weight-stationary launch per layer and direction of the pass.
//
// Geometry.  A workgroup owns kUnits = 16 hidden units (their 64 gate rows of W_hh, held in VGPRs for the whole
// launch: H / 4 floats per lane) and C batch columns.  The G = H / 16 workgroups that share C columns form a
// group; a group needs nothing from another group.  Grid = ceil(N / C) * G <= the CU count, one workgroup per CU.
//
// Hand-off.  Inside a group every step is an all-to-all: forward, each member needs the whole h_{t-1} of its
// columns; backward, each member needs the sum over members of W_hh[rows(m), J]^T dG_{t+1}[rows(m)] for its units J
// (a reduce-scatter, summed in producer order: bit-reproducible).  Both go through 8-byte granules {value, tag}
// written by ONE sc1 store and read by sc1 loads until every tag matches (cdna_hip_programming.md Guideline 16,
// R2: the data is the flag, no fence).  Tag = step + 1, two slots by step parity: no member can publish step s + 2
// before every member has read step s.  The granule buffers are zeroed by a kernel in front of every launch.
// Every spin is bounded by a clock budget; on expiry TK_STATUS_LSTM_TIMEOUT is OR-ed into *status and the whole
// grid leaves (the other spins see the bit).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/taiyaki_amd_flipflop.h"
#include "ff_common.h"

namespace tk {
namespace {

constexpr int kThreads = 256;
constexpr int kUnits = 16;                      // hidden units per workgroup
constexpr int kRows = 4 * kUnits;               // their gate rows
constexpr uint64_t kSpinTicks = 200000000ull;   // 2 s of s_memrealtime (100 MHz) per wait

typedef unsigned long long u64;
typedef __attribute__((address_space(1))) u64 gu64;
typedef __attribute__((address_space(1))) uint32_t gu32;

__device__ __forceinline__ void store_granule(u64 *g, unsigned tag, float v) {
    __hip_atomic_store((gu64 *)g, ((u64)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// This lane's NG granules g[q * stride] (q < nvalid) until every lane of the wave sees `tag` in all of its own;
// false when the clock budget runs out or another workgroup has already given up.
template <int NG>
__device__ __forceinline__ bool sweep(const u64 *g, int stride, int nvalid, unsigned tag, float (&v)[NG],
                                      uint32_t *status) {
    const uint64_t start = __builtin_amdgcn_s_memrealtime();
    for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            if (q < nvalid) {
                const u64 x = __hip_atomic_load((gu64 *)(g + q * stride), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v[q] = __uint_as_float((unsigned)x);
                ok &= (unsigned)(x >> 32) == tag;
            }
        }
        if (__all(ok)) return true;
        if ((spins & 31) == 31) {
            const uint32_t st = __hip_atomic_load((gu32 *)status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((st & TK_STATUS_LSTM_TIMEOUT) || __builtin_amdgcn_s_memrealtime() - start > kSpinTicks) {
                __hip_atomic_fetch_or((gu32 *)status, TK_STATUS_LSTM_TIMEOUT, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Block -> (group, member).  Blocks b and b + 8 share an XCD under round-robin placement; members of a group are
// taken from one residue of b mod 8 where the grid allows (speed only: the hand-off does not depend on placement).
__device__ __forceinline__ void place(int G, int &group, int &member) {
    const int b = blockIdx.x, nb = gridDim.x;
    int L = b;
    if (nb % 8 == 0 && (nb / 8) % G == 0) L = (b % 8) * (nb / 8) + b / 8;
    group = L / G;
    member = L % G;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__global__ void zero_u64x2_kernel(uint4 *p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// Forward.  gx (T, N, 4H) = x W_ih^T + b_ih + b_hh.  Writes y = h (T, N, H), the gate activations (T, N, 4H) and
// c (T, N, H).  Recurrence step s runs time t = s (reverse: T - 1 - s).  hbuf: [2][ngroups][C][H] granules.
template <int H, int C>
constexpr int fwd_lds_bytes() { return (kRows * H + H * C + kRows * C) * 4 + 16; }

template <int H, int C>
__global__ __launch_bounds__(kThreads, 1) void lstm_fwd_kernel(const float *__restrict__ gx,
                                                               const float *__restrict__ whh, int T, int N,
                                                               int reverse, int ngroups, float *__restrict__ y,
                                                               float *__restrict__ gates, float *__restrict__ cell,
                                                               u64 *hbuf, uint32_t *status) {
    constexpr int G = H / kUnits;
    constexpr int NG = (H * C + kThreads - 1) / kThreads;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *wl = reinterpret_cast<float4 *>(smem);                 // this lane's W_hh: [H / 16][lane] float4
    float *hs = reinterpret_cast<float *>(smem) + kRows * H;       // h_{t-1} as [k][c]
    float *pre = hs + H * C;                                       // W_hh h_{t-1} as [row][c]
    int *give_up = reinterpret_cast<int *>(pre + kRows * C);

    int group, member;
    place(G, group, member);
    const int tid = threadIdx.x;
    const int j0 = member * kUnits, n0 = group * C;

    // lane (r, kc): local gate row r = gate * 16 + unit, columns k = 16 i + 4 kc + (0..3).  Its W_hh values sit in
    // LDS in lane order (each lane reads back only what it wrote: one conflict-free ds_read_b128 per 4 columns)
    const int r = tid >> 2, kc = tid & 3;
    const int grow = (r / kUnits) * H + j0 + (r % kUnits);
    for (int i = 0; i < H / 16; ++i) {
        const float *p = whh + (size_t)grow * H + 16 * i + 4 * kc;
        wl[i * kThreads + tid] = make_float4(p[0], p[1], p[2], p[3]);
    }

    // cell lane (c, u)
    const bool cell_lane = tid < kUnits * C;
    const int cc = tid / kUnits, u = tid % kUnits;
    const int n = n0 + cc;
    const bool valid = cell_lane && n < N;
    float cst = 0.f;

    for (int i = tid; i < H * C; i += kThreads) hs[i] = 0.f;
    if (tid == 0) *give_up = 0;
    __syncthreads();

    const size_t H4 = 4 * (size_t)H;
    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        float gxv[4] = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
            const float *p = gx + ((size_t)t * N + n) * H4 + j0 + u;
#pragma unroll
            for (int g = 0; g < 4; ++g) gxv[g] = p[(size_t)g * H];
        }
        if (s > 0) {
            const u64 *src = hbuf + ((size_t)((s - 1) & 1) * ngroups + group) * (H * C);
            float v[NG];
            const int nvalid = tid < H * C ? (H * C - tid + kThreads - 1) / kThreads : 0;
            if (!sweep<NG>(src + tid, kThreads, nvalid, (unsigned)s, v, status)) *give_up = 1;
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                const int e = tid + q * kThreads;        // granule e = c * H + k
                if (q < nvalid) hs[(e % H) * C + e / H] = v[q];
            }
            __syncthreads();
            if (*give_up) return;
        }

        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll 2
        for (int i = 0; i < H / 16; ++i) {
            const float4 w4 = wl[i * kThreads + tid];
            const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 *hp = reinterpret_cast<const float4 *>(hs + (16 * i + 4 * kc + j) * C);
#pragma unroll
                for (int c4 = 0; c4 < C / 4; ++c4) {
                    const float4 h4 = hp[c4];
                    acc[4 * c4 + 0] = fmaf(wv[j], h4.x, acc[4 * c4 + 0]);
                    acc[4 * c4 + 1] = fmaf(wv[j], h4.y, acc[4 * c4 + 1]);
                    acc[4 * c4 + 2] = fmaf(wv[j], h4.z, acc[4 * c4 + 2]);
                    acc[4 * c4 + 3] = fmaf(wv[j], h4.w, acc[4 * c4 + 3]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            acc[c] += __shfl_xor(acc[c], 1);
            acc[c] += __shfl_xor(acc[c], 2);
            if ((c & 3) == kc) pre[r * C + c] = acc[c];
        }
        __syncthreads();

        if (cell_lane) {
            const float zi = pre[(0 * kUnits + u) * C + cc] + gxv[0];
            const float zf = pre[(1 * kUnits + u) * C + cc] + gxv[1];
            const float zg = pre[(2 * kUnits + u) * C + cc] + gxv[2];
            const float zo = pre[(3 * kUnits + u) * C + cc] + gxv[3];
            const float ig = sigmoidf(zi), fg = sigmoidf(zf), gg = tanhf(zg), og = sigmoidf(zo);
            cst = fg * cst + ig * gg;
            const float h = og * tanhf(cst);
            if (valid) {
                const size_t o = ((size_t)t * N + n) * H + j0 + u;
                y[o] = h;
                cell[o] = cst;
                float *gp = gates + ((size_t)t * N + n) * H4 + j0 + u;
                gp[0] = ig;
                gp[(size_t)H] = fg;
                gp[2 * (size_t)H] = gg;
                gp[3 * (size_t)H] = og;
            }
            if (s + 1 < T)
                store_granule(hbuf + ((size_t)(s & 1) * ngroups + group) * (H * C) + cc * H + j0 + u,
                              (unsigned)(s + 1), h);
        }
    }
}

// Backward.  From the saved gate activations and c, and dy = dL/dy (T, N, H), writes dgates = dL/d(pre-activation)
// (T, N, 4H) walking the recurrence from its last step.  pbuf: [2][ngroups][G producers][C][H] granules.
template <int H, int C>
__global__ __launch_bounds__(kThreads, 1) void lstm_bwd_kernel(const float *__restrict__ whh,
                                                               const float *__restrict__ gates,
                                                               const float *__restrict__ cell,
                                                               const float *__restrict__ dy, int T, int N,
                                                               int reverse, int ngroups, float *__restrict__ dgates,
                                                               u64 *pbuf, uint32_t *status) {
    constexpr int G = H / kUnits;
    constexpr int RP = kThreads / H;                  // row partitions: lane (k, rp) holds W_hh[rows of rp, k]
    constexpr int R = kRows / RP;                     // = H / 4 floats per lane
    constexpr int PAIRS = kUnits * C;                 // (c, u) pairs of the cell update
    constexpr int PL = kThreads / PAIRS >= 1 ? kThreads / PAIRS : 1;   // producer planes of the gather
    constexpr int NP = (G + PL - 1) / PL;
    static_assert(PAIRS <= kThreads, "one cell lane per (column, unit)");
    __shared__ __attribute__((aligned(16))) float dgs[kRows * C];      // dG_t of the owned rows as [row][c]
    __shared__ float gath[PL * PAIRS];
    __shared__ __attribute__((aligned(16))) float red[RP > 1 ? RP * C * H : 1];
    __shared__ int give_up;

    int group, member;
    place(G, group, member);
    const int tid = threadIdx.x;
    const int j0 = member * kUnits, n0 = group * C;

    const int k = tid % H, rp = tid / H;
    float w[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int r = rp * R + i;
        w[i] = whh[((size_t)(r / kUnits) * H + j0 + (r % kUnits)) * H + k];
    }

    const bool cell_lane = tid < PAIRS;
    const int pair = tid % PAIRS, plane = tid / PAIRS;
    const int cc = pair / kUnits, u = pair % kUnits;
    const int n = n0 + cc;
    const bool valid = cell_lane && n < N;
    float dc_next = 0.f, f_next = 0.f;
    if (tid == 0) give_up = 0;
    __syncthreads();

    const size_t H4 = 4 * (size_t)H;
    const u64 *mine = pbuf + (size_t)group * G * C * H + cc * H + j0 + u;
    for (int s = 0; s < T; ++s) {
        const int tt = T - 1 - s;                         // recurrence position
        const int t = reverse ? T - 1 - tt : tt;          // time index
        const int tp = reverse ? t + 1 : t - 1;           // time index of the recurrence's previous step
        float dyv = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, ct = 0.f, cp = 0.f;
        if (valid) {
            const size_t o = ((size_t)t * N + n) * H + j0 + u;
            dyv = dy[o];
            ct = cell[o];
            if (tt > 0) cp = cell[((size_t)tp * N + n) * H + j0 + u];
            const float *gp = gates + ((size_t)t * N + n) * H4 + j0 + u;
            ig = gp[0];
            fg = gp[(size_t)H];
            gg = gp[2 * (size_t)H];
            og = gp[3 * (size_t)H];
        }
        float dhr = 0.f;
        if (s > 0) {
            if (plane < PL) {
                float v[NP];
                const int nvalid = plane < G ? (G - plane + PL - 1) / PL : 0;
                const u64 *src = mine + (size_t)((s - 1) & 1) * ngroups * G * C * H + (size_t)plane * C * H;
                if (!sweep<NP>(src, PL * C * H, nvalid, (unsigned)s, v, status)) give_up = 1;
                float sum = 0.f;
#pragma unroll
                for (int q = 0; q < NP; ++q)
                    if (q < nvalid) sum += v[q];
                gath[plane * PAIRS + pair] = sum;
            }
            __syncthreads();
            if (give_up) return;
            if (cell_lane) {
#pragma unroll
                for (int p = 0; p < PL; ++p) dhr += gath[p * PAIRS + pair];
            }
        }

        if (cell_lane) {
            const float dh = dyv + dhr;
            const float tc = tanhf(ct);
            const float dc = dh * og * (1.f - tc * tc) + dc_next * f_next;
            const float di = dc * gg * ig * (1.f - ig);
            const float df = dc * cp * fg * (1.f - fg);
            const float dg = dc * ig * (1.f - gg * gg);
            const float dout = dh * tc * og * (1.f - og);
            dc_next = dc;
            f_next = fg;
            if (valid) {
                float *dp = dgates + ((size_t)t * N + n) * H4 + j0 + u;
                dp[0] = di;
                dp[(size_t)H] = df;
                dp[2 * (size_t)H] = dg;
                dp[3 * (size_t)H] = dout;
            }
            dgs[(0 * kUnits + u) * C + cc] = valid ? di : 0.f;
            dgs[(1 * kUnits + u) * C + cc] = valid ? df : 0.f;
            dgs[(2 * kUnits + u) * C + cc] = valid ? dg : 0.f;
            dgs[(3 * kUnits + u) * C + cc] = valid ? dout : 0.f;
        }
        __syncthreads();
        if (s + 1 == T) break;                            // the first step has no predecessor to feed

        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float4 *dp = reinterpret_cast<const float4 *>(dgs + (rp * R + i) * C);
#pragma unroll
            for (int c4 = 0; c4 < C / 4; ++c4) {
                const float4 d4 = dp[c4];
                acc[4 * c4 + 0] = fmaf(w[i], d4.x, acc[4 * c4 + 0]);
                acc[4 * c4 + 1] = fmaf(w[i], d4.y, acc[4 * c4 + 1]);
                acc[4 * c4 + 2] = fmaf(w[i], d4.z, acc[4 * c4 + 2]);
                acc[4 * c4 + 3] = fmaf(w[i], d4.w, acc[4 * c4 + 3]);
            }
        }
        u64 *dst = pbuf + (((size_t)(s & 1) * ngroups + group) * G + member) * C * H;
        if constexpr (RP == 1) {
#pragma unroll
            for (int c = 0; c < C; ++c) store_granule(dst + c * H + k, (unsigned)(s + 1), acc[c]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) red[(rp * C + c) * H + k] = acc[c];
            __syncthreads();
            for (int e = tid; e < C * H; e += kThreads) {
                float v = 0.f;
#pragma unroll
                for (int q = 0; q < RP; ++q) v += red[q * C * H + e];
                store_granule(dst + e, (unsigned)(s + 1), v);
            }
        }
    }
}

int g_lab_cols = 0;     // lab build: force the batch columns per workgroup (0 = the rule below)

// The launch geometry: batch columns per workgroup C and groups; false where the kernels do not run.
bool lstm_geometry(size_t N, size_t H, int cu_count, int *C_out, int *groups_out) {
    if (!(H == 16 || H == 32 || H == 64 || H == 128 || H == 256) || N == 0 || cu_count <= 0) return false;
    const size_t G = H / kUnits;
    for (int C : {8, 16}) {
        if (g_lab_cols != 0 && C != g_lab_cols) continue;
        const size_t groups = (N + C - 1) / C;
        if (groups * G <= (size_t)cu_count) {
            *C_out = C;
            *groups_out = (int)groups;
            return true;
        }
    }
    return false;
}

size_t ws_bytes(size_t H, int C, int groups, bool backward) {
    const size_t G = H / kUnits;
    return 2 * (size_t)groups * (backward ? G : 1) * C * H * sizeof(u64);
}

int zero_ws(void *ws, size_t bytes, hipStream_t stream) {
    // (a kernel, not hipMemsetAsync: see clip_kernels.hip on memset nodes replayed from a hipGraph)
    const size_t n = bytes / 16;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(zero_u64x2_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<uint4 *>(ws), n);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

template <int C>
int launch_fwd(size_t H, dim3 grid, hipStream_t st, const float *gx, const float *whh, int T, int N, int rev,
               int groups, float *y, float *gates, float *cell, u64 *ws, uint32_t *status) {
#define TK_LSTM_FWD(HH)                                                                                       \
    case HH:                                                                                                  \
        if (raise_dynamic_lds((const void *)lstm_fwd_kernel<HH, C>, fwd_lds_bytes<HH, C>())) return TK_ERR_LAUNCH; \
        hipLaunchKernelGGL((lstm_fwd_kernel<HH, C>), grid, dim3(kThreads), (fwd_lds_bytes<HH, C>()), st, gx, whh, T, N, \
                           rev, groups, y, gates, cell, ws, status);                                          \
        break;
    switch (H) {
        TK_LSTM_FWD(16) TK_LSTM_FWD(32) TK_LSTM_FWD(64) TK_LSTM_FWD(128) TK_LSTM_FWD(256)
        default: return TK_ERR_UNSUPPORTED;
    }
#undef TK_LSTM_FWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

template <int C>
int launch_bwd(size_t H, dim3 grid, hipStream_t st, const float *whh, const float *gates, const float *cell,
               const float *dy, int T, int N, int rev, int groups, float *dg, u64 *ws, uint32_t *status) {
#define TK_LSTM_BWD(HH)                                                                                        \
    case HH:                                                                                                   \
        hipLaunchKernelGGL((lstm_bwd_kernel<HH, C>), grid, dim3(kThreads), 0, st, whh, gates, cell, dy, T, N, \
                           rev, groups, dg, ws, status);                                                       \
        break;
    switch (H) {
        TK_LSTM_BWD(16) TK_LSTM_BWD(32) TK_LSTM_BWD(64) TK_LSTM_BWD(128) TK_LSTM_BWD(256)
        default: return TK_ERR_UNSUPPORTED;
    }
#undef TK_LSTM_BWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

size_t lstm_workspace_bytes(size_t N, size_t H, int cu_count) {
    int C = 0, groups = 0;
    if (!lstm_geometry(N, H, cu_count, &C, &groups)) return 0;
    return ws_bytes(H, C, groups, true);        // the backward's is the larger
}

int lstm_forward_dispatch(const float *gx, const float *whh, size_t T, size_t N, size_t H, int reverse,
                          int cu_count, float *y, float *gates, float *cell, void *ws, size_t wsb,
                          uint32_t *status, hipStream_t stream) {
    if (!gx || !whh || !y || !gates || !cell || !ws || !status || !aligned16(ws) || T > (size_t)INT32_MAX ||
        N > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
    int C = 0, groups = 0;
    if (!lstm_geometry(N, H, cu_count, &C, &groups)) return TK_ERR_UNSUPPORTED;
    const size_t need = ws_bytes(H, C, groups, false);
    if (wsb < need) return TK_ERR_WORKSPACE;
    if (T == 0) return TK_OK;
    int rc = zero_ws(ws, need, stream);
    if (rc != TK_OK) return rc;
    const dim3 grid((unsigned)(groups * (H / kUnits)));
    u64 *hb = static_cast<u64 *>(ws);
    return C == 8 ? launch_fwd<8>(H, grid, stream, gx, whh, (int)T, (int)N, reverse, groups, y, gates, cell, hb, status)
                  : launch_fwd<16>(H, grid, stream, gx, whh, (int)T, (int)N, reverse, groups, y, gates, cell, hb,
                                   status);
}

int lstm_backward_dispatch(const float *whh, const float *gates, const float *cell, const float *dy, size_t T,
                           size_t N, size_t H, int reverse, int cu_count, float *dgates, void *ws, size_t wsb,
                           uint32_t *status, hipStream_t stream) {
    if (!whh || !gates || !cell || !dy || !dgates || !ws || !status || !aligned16(ws) || T > (size_t)INT32_MAX ||
        N > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
    int C = 0, groups = 0;
    if (!lstm_geometry(N, H, cu_count, &C, &groups)) return TK_ERR_UNSUPPORTED;
    const size_t need = ws_bytes(H, C, groups, true);
    if (wsb < need) return TK_ERR_WORKSPACE;
    if (T == 0) return TK_OK;
    int rc = zero_ws(ws, need, stream);
    if (rc != TK_OK) return rc;
    const dim3 grid((unsigned)(groups * (H / kUnits)));
    u64 *pb = static_cast<u64 *>(ws);
    return C == 8 ? launch_bwd<8>(H, grid, stream, whh, gates, cell, dy, (int)T, (int)N, reverse, groups, dgates, pb,
                                  status)
                  : launch_bwd<16>(H, grid, stream, whh, gates, cell, dy, (int)T, (int)N, reverse, groups, dgates,
                                   pb, status);
}

#ifdef TK_LAB
void lstm_lab_cols(int cols) { g_lab_cols = cols; }
#endif

}  // namespace tk

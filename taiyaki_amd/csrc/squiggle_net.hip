// The squiggle predictor network (include/taiyaki_amd_squiggle_net.h): Convolution(3 -> S, tanh), `depth` residual
// Convolution(S -> S, tanh) layers and Convolution(S -> 3, linear), the whole stack in one launch per pass.
//
// A workgroup of 256 threads owns `tile` positions of one column and works on SN_ROWS = tile + 2 R buffer rows, R =
// (depth + 2) (W / 2): buffer row j is position t0 - R + j.  Every layer is computed on ALL buffer rows; what a layer
// reads beyond the buffer are guard rows that stay zero, so a row within (l + 1) (W / 2) rows of the buffer's edge is
// wrong after layer l -- and after depth + 2 layers the wrong rows are exactly the halo, which nobody stores.  Positions
// outside [0, length) are forced to +0 after every layer: the next window then reads its own padding there.
//
// Thread tile of a S -> S layer: RT = S / 8 rows x 4 channels; per tap the weights are staged in LDS as [cin][cout] (the
// backward's transposed convolution: [cout][cin]) and every thread runs cin in ascending order through one fmaf chain per
// output and tap; a tap's sum is added to the output whole.  Weight gradients: thread tile (S / 16)^2 (cin, cout) pairs
// x W taps, one pass over the owned rows with the W rows of the layer's input that a row meets kept in registers (a
// window that rotates at compile time).
#include <hip/hip_runtime.h>

#include "../../include/taiyaki_amd_squiggle_net.h"

namespace tk {
namespace {

constexpr int SN_ROWS = 128, SN_THREADS = 256, SN_GUARD = 4, SN_MAX_DEPTH = 8, SN_MAX_LAYERS = SN_MAX_DEPTH + 2;
constexpr int SN_BROWS = SN_ROWS + 2 * SN_GUARD;

struct SnParams {
    const float *w[SN_MAX_LAYERS];
    const float *b[SN_MAX_LAYERS];
};
struct SnGrads {
    float *w[SN_MAX_LAYERS];
    float *b[SN_MAX_LAYERS];
};

struct SnPlan {
    int R, tile, tiles, fwd_grid, bwd_grid;
    size_t items, slab_floats, bytes;
};

struct SnArgs {
    const float *x, *dy;
    const int *lengths;
    float *y, *dx;
    float *saved;          // forward: written (NULL: not wanted); backward: read
    float *ws;
    SnParams p;
    int P, N, depth, R, tile, tiles, items;
    unsigned slab_floats;
};

inline bool sn_shape_ok(size_t size, size_t depth, size_t winlen) {
    return (size == 16 || size == 32 || size == 64) && (winlen == 5 || winlen == 9) && depth >= 1 && depth <= SN_MAX_DEPTH;
}

inline size_t sn_slab_floats(size_t S, size_t depth, size_t W) {
    return (3 * S * W + S) + depth * (S * S * W + S) + (3 * S * W + 4);
}

bool sn_plan(size_t P, size_t N, size_t size, size_t depth, size_t winlen, int cu_count, SnPlan *p) {
    if (!sn_shape_ok(size, depth, winlen) || P == 0 || N == 0 || P >= ((size_t)1 << 31)) return false;
    p->R = (int)((depth + 2) * (winlen / 2));
    p->tile = SN_ROWS - 2 * p->R;
    const size_t tiles = (P + p->tile - 1) / p->tile;
    if (tiles * N >= ((size_t)1 << 31)) return false;
    p->tiles = (int)tiles;
    p->items = tiles * N;
    p->fwd_grid = (int)p->items;
    const size_t wgs = (size_t)(cu_count < 1 ? 1 : cu_count) * (size == 64 ? 1 : 2);
    p->bwd_grid = (int)(p->items < wgs ? p->items : wgs);
    p->slab_floats = sn_slab_floats(size, depth, winlen);
    p->bytes = (size_t)p->bwd_grid * p->slab_floats * sizeof(float);
    return true;
}

template <int S, int W>
struct SnLay {
    static constexpr int SP = S + 4, RT = S / 8, NCG = S / 4, H = W / 2, BUF = SN_BROWS * SP, WT = S * SP;
    static constexpr int SMALL = SN_BROWS * 4, W0 = 3 * W * S, WL = 3 * S * W;
    static constexpr size_t FWD_LDS = sizeof(float) * (2 * BUF + WT + SMALL + W0 + WL);
    static constexpr size_t BWD_LDS = sizeof(float) * (3 * BUF + WT + 2 * SMALL + W0 + WL);
};

__device__ inline float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ inline void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

// acc[i][e] += per tap (ascending) the sum over the input's channels (ascending, one fmaf chain from 0) of
// in[row + tap offset][c] w[c -> c0 + e]: a tap's sum is added whole, which keeps the chains short (S terms, then W)
template <int S, int W, bool FWD>
__device__ inline void sn_conv_taps(const float *in, const float *w, float *wt, float (&acc)[S / 8][4], int r0, int c0,
                                    int tid) {
    using L = SnLay<S, W>;
#pragma unroll 1
    for (int k = 0; k < W; ++k) {
        __syncthreads();        // the tap before is done with wt (tap 0: `in` is complete)
        for (int e = tid; e < S * S; e += SN_THREADS) {
            const int co = e / S, ci = e % S;
            const float v = w[(size_t)e * W + k];
            wt[FWD ? ci * L::SP + co : co * L::SP + ci] = v;
        }
        __syncthreads();
        const float *base = in + (r0 + (FWD ? k - L::H : L::H - k) + SN_GUARD) * L::SP;
        float part[L::RT][4];
#pragma unroll
        for (int i = 0; i < L::RT; ++i) part[i][0] = part[i][1] = part[i][2] = part[i][3] = 0.f;
#pragma unroll 2
        for (int c4 = 0; c4 < S / 4; ++c4) {
            const float4 w0 = ld4(&wt[(4 * c4 + 0) * L::SP + c0]), w1 = ld4(&wt[(4 * c4 + 1) * L::SP + c0]);
            const float4 w2 = ld4(&wt[(4 * c4 + 2) * L::SP + c0]), w3 = ld4(&wt[(4 * c4 + 3) * L::SP + c0]);
#pragma unroll
            for (int i = 0; i < L::RT; ++i) {
                const float4 a = ld4(&base[i * L::SP + 4 * c4]);
                part[i][0] = fmaf(a.w, w3.x, fmaf(a.z, w2.x, fmaf(a.y, w1.x, fmaf(a.x, w0.x, part[i][0]))));
                part[i][1] = fmaf(a.w, w3.y, fmaf(a.z, w2.y, fmaf(a.y, w1.y, fmaf(a.x, w0.y, part[i][1]))));
                part[i][2] = fmaf(a.w, w3.z, fmaf(a.z, w2.z, fmaf(a.y, w1.z, fmaf(a.x, w0.z, part[i][2]))));
                part[i][3] = fmaf(a.w, w3.w, fmaf(a.z, w2.w, fmaf(a.y, w1.w, fmaf(a.x, w0.w, part[i][3]))));
            }
        }
#pragma unroll
        for (int i = 0; i < L::RT; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][e] += part[i][e];
    }
}

// the guard rows of `n` activation buffers, once per launch: no layer writes them
template <int S, int W>
__device__ inline void sn_zero_guards(float *bufs, int n, int tid) {
    using L = SnLay<S, W>;
    for (int e = tid; e < n * 2 * SN_GUARD * L::SP; e += SN_THREADS) {
        const int b = e / (2 * SN_GUARD * L::SP), r = e % (2 * SN_GUARD * L::SP);
        const int row = r / L::SP, c = r % L::SP;
        bufs[b * L::BUF + (row < SN_GUARD ? row : SN_ROWS + row) * L::SP + c] = 0.f;
    }
}

// a (P, N, 3) tensor's rows t0 - R - guard ... as [row][4] in LDS, zero outside [0, len)
__device__ inline void sn_load3(const float *src, float *dst, int t0R, int len, int N, int n, int tid) {
    for (int e = tid; e < SN_BROWS * 4; e += SN_THREADS) {
        const int c = e & 3, p = t0R + (e >> 2) - SN_GUARD;
        dst[e] = (c < 3 && p >= 0 && p < len) ? src[((size_t)p * N + n) * 3 + c] : 0.f;
    }
}

// w_0 (S, 3, W) as [k][ci][co]; w_last (3, S, W) as [c][k][ci]
template <int S, int W>
__device__ inline void sn_stage_ends(const float *w0, const float *wl, float *w0s, float *wls, int tid) {
    for (int e = tid; e < 3 * W * S; e += SN_THREADS) {
        const int co = e / (3 * W), ci = (e / W) % 3, k = e % W;
        w0s[(k * 3 + ci) * S + co] = w0[e];
    }
    for (int e = tid; e < 3 * S * W; e += SN_THREADS) {
        const int c = e / (S * W), ci = (e / W) % S, k = e % W;
        wls[(c * W + k) * S + ci] = wl[e];
    }
}

template <int S, int W>
__global__ __launch_bounds__(SN_THREADS) void sn_forward_kernel(SnArgs a) {
    using L = SnLay<S, W>;
    extern __shared__ float4 sn_smem[];
    float *sm = reinterpret_cast<float *>(sn_smem);
    float *cur = sm, *nxt = cur + L::BUF, *wt = nxt + L::BUF, *xs = wt + L::WT, *w0s = xs + L::SMALL, *wls = w0s + L::W0;
    const int tid = threadIdx.x, n = blockIdx.x / a.tiles, t0 = (blockIdx.x % a.tiles) * a.tile;
    const int P = a.P, N = a.N, R = a.R;
    int len = a.lengths ? a.lengths[n] : P;
    len = len < 0 ? 0 : (len > P ? P : len);
    const int own_n = (P - t0 < a.tile ? P - t0 : a.tile);

    if (t0 >= len) {    // nothing of this column here: +0
        for (int e = tid; e < own_n * 3; e += SN_THREADS) a.y[((size_t)(t0 + e / 3) * N + n) * 3 + e % 3] = 0.f;
        if (a.saved)
            for (int l = 0; l <= a.depth; ++l)
                for (int e = tid; e < own_n * (S / 4); e += SN_THREADS)
                    st4(&a.saved[(((size_t)l * P + t0 + e / (S / 4)) * N + n) * S + 4 * (e % (S / 4))],
                        make_float4(0.f, 0.f, 0.f, 0.f));
        return;
    }

    sn_zero_guards<S, W>(cur, 2, tid);
    sn_load3(a.x, xs, t0 - R, len, N, n, tid);
    sn_stage_ends<S, W>(a.p.w[0], a.p.w[a.depth + 1], w0s, wls, tid);
    __syncthreads();

    const int c0 = 4 * (tid % L::NCG), r0 = L::RT * (tid / L::NCG);
    float acc[L::RT][4];

    for (int l = 0; l <= a.depth; ++l) {
        const float *bl = a.p.b[l] + c0;
        const float4 b = make_float4(bl[0], bl[1], bl[2], bl[3]);
#pragma unroll
        for (int i = 0; i < L::RT; ++i) acc[i][0] = b.x, acc[i][1] = b.y, acc[i][2] = b.z, acc[i][3] = b.w;
        if (l == 0) {
#pragma unroll 3
            for (int kc = 0; kc < 3 * W; ++kc) {
                const float4 w = ld4(&w0s[kc * S + c0]);
                const int k = kc / 3, ci = kc % 3;
#pragma unroll
                for (int i = 0; i < L::RT; ++i) {
                    const float xv = xs[(r0 + i + k - L::H + SN_GUARD) * 4 + ci];
                    acc[i][0] = fmaf(xv, w.x, acc[i][0]), acc[i][1] = fmaf(xv, w.y, acc[i][1]);
                    acc[i][2] = fmaf(xv, w.z, acc[i][2]), acc[i][3] = fmaf(xv, w.w, acc[i][3]);
                }
            }
        } else {
            sn_conv_taps<S, W, true>(cur, a.p.w[l], wt, acc, r0, c0, tid);
        }
        float *out = l == 0 ? cur : nxt;
#pragma unroll
        for (int i = 0; i < L::RT; ++i) {
            const int j = r0 + i, p = t0 - R + j;
            const bool valid = p >= 0 && p < len;
            float4 t;
            t.x = valid ? tanhf(acc[i][0]) : 0.f, t.y = valid ? tanhf(acc[i][1]) : 0.f;
            t.z = valid ? tanhf(acc[i][2]) : 0.f, t.w = valid ? tanhf(acc[i][3]) : 0.f;
            if (a.saved && j >= R && j < R + own_n) st4(&a.saved[(((size_t)l * P + p) * N + n) * S + c0], t);
            if (l > 0) {
                const float4 r = ld4(&cur[(j + SN_GUARD) * L::SP + c0]);
                t.x = r.x + t.x, t.y = r.y + t.y, t.z = r.z + t.z, t.w = r.w + t.w;
            }
            st4(&out[(j + SN_GUARD) * L::SP + c0], t);
        }
        if (l > 0) {
            float *s = cur;
            cur = nxt, nxt = s;
        }
    }
    __syncthreads();

    for (int e = tid; e < own_n * 3; e += SN_THREADS) {
        const int jr = e / 3, c = e % 3, p = t0 + jr;
        float s = a.p.b[a.depth + 1][c];
        for (int k = 0; k < W; ++k) {
            const float *in = cur + (R + jr + k - L::H + SN_GUARD) * L::SP, *w = wls + (c * W + k) * S;
            float part = 0.f;
#pragma unroll 4
            for (int c4 = 0; c4 < S / 4; ++c4) {
                const float4 v = ld4(&in[4 * c4]), ww = ld4(&w[4 * c4]);
                part = fmaf(v.w, ww.w, fmaf(v.z, ww.z, fmaf(v.y, ww.y, fmaf(v.x, ww.x, part))));
            }
            s += part;
        }
        a.y[((size_t)p * N + n) * 3 + c] = p < len ? s : 0.f;
    }
}

// dw[k][ci][co] (+)= sum over the owned rows of dz[row][co] a[row + k - H][ci], into the workgroup's slab
template <int S, int W>
__device__ inline void sn_wgrad_mid(const float *Z, const float *A, float *slab, bool add, int R, int own_n, int tid) {
    using L = SnLay<S, W>;
    constexpr int CT = S / 16;
    const int ci0 = CT * (tid % 16), co0 = CT * (tid / 16);
    float acc[W][CT][CT], win[W][CT];
#pragma unroll
    for (int k = 0; k < W; ++k)
#pragma unroll
        for (int u = 0; u < CT; ++u)
#pragma unroll
            for (int v = 0; v < CT; ++v) acc[k][u][v] = 0.f;
    // slot of buffer row r: (r - (R - H)) mod W; rows R - H ... R + H - 1 first
#pragma unroll
    for (int s = 0; s < W - 1; ++s)
#pragma unroll
        for (int u = 0; u < CT; ++u) win[s][u] = A[(R - L::H + s + SN_GUARD) * L::SP + ci0 + u];
    for (int j0 = 0; j0 < own_n; j0 += W) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int row = R + j0 + j;
            float dz[CT];
#pragma unroll
            for (int u = 0; u < CT; ++u) {
                win[(j + W - 1) % W][u] = A[(row + L::H + SN_GUARD) * L::SP + ci0 + u];
                dz[u] = j0 + j < own_n ? Z[(row + SN_GUARD) * L::SP + co0 + u] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < W; ++k)
#pragma unroll
                for (int u = 0; u < CT; ++u)
#pragma unroll
                    for (int v = 0; v < CT; ++v) acc[k][u][v] = fmaf(win[(j + k) % W][u], dz[v], acc[k][u][v]);
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k)
#pragma unroll
        for (int u = 0; u < CT; ++u)
#pragma unroll
            for (int v = 0; v < CT; ++v) {
                float *d = &slab[(k * S + ci0 + u) * S + co0 + v];
                *d = add ? *d + acc[k][u][v] : acc[k][u][v];
            }
}

template <int S, int W>
__global__ __launch_bounds__(SN_THREADS) void sn_backward_kernel(SnArgs a) {
    using L = SnLay<S, W>;
    extern __shared__ float4 sn_smem[];
    float *sm = reinterpret_cast<float *>(sn_smem);
    float *A = sm, *D = A + L::BUF, *Z = D + L::BUF, *wt = Z + L::BUF, *dyb = wt + L::WT, *xs = dyb + L::SMALL;
    float *w0s = xs + L::SMALL, *wls = w0s + L::W0;
    const int tid = threadIdx.x, P = a.P, N = a.N, R = a.R, depth = a.depth;
    float *slab = a.ws + (size_t)blockIdx.x * a.slab_floats;
    constexpr int OFF_MID = 3 * S * W + S, MID = S * S * W + S;
    const int off_last = OFF_MID + depth * MID;
    const int c0 = 4 * (tid % L::NCG), r0 = L::RT * (tid / L::NCG);
    bool wrote = false;

    sn_zero_guards<S, W>(A, 3, tid);
    sn_stage_ends<S, W>(a.p.w[0], a.p.w[depth + 1], w0s, wls, tid);

    for (int item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int n = item / a.tiles, t0 = (item % a.tiles) * a.tile;
        int len = a.lengths ? a.lengths[n] : P;
        len = len < 0 ? 0 : (len > P ? P : len);
        const int own_n = (P - t0 < a.tile ? P - t0 : a.tile);
        if (t0 >= len) {
            if (a.dx)
                for (int e = tid; e < own_n * 3; e += SN_THREADS) a.dx[((size_t)(t0 + e / 3) * N + n) * 3 + e % 3] = 0.f;
            continue;
        }
        __syncthreads();        // the tile before is done with every buffer
        sn_load3(a.dy, dyb, t0 - R, len, N, n, tid);
        sn_load3(a.x, xs, t0 - R, len, N, n, tid);
        // a_depth, in the forward's order
#pragma unroll
        for (int i = 0; i < L::RT; ++i) {
            const int j = r0 + i, p = t0 - R + j;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p >= 0 && p < len) {
                s = ld4(&a.saved[((size_t)p * N + n) * S + c0]);
                for (int l = 1; l <= depth; ++l) {
                    const float4 t = ld4(&a.saved[(((size_t)l * P + p) * N + n) * S + c0]);
                    s.x = s.x + t.x, s.y = s.y + t.y, s.z = s.z + t.z, s.w = s.w + t.w;
                }
            }
            st4(&A[(j + SN_GUARD) * L::SP + c0], s);
        }
        __syncthreads();

        // the linear layer: dw (3, S, W), db (3); D = its transposed convolution of dy
        for (int e = tid; e < 3 * S * W; e += SN_THREADS) {
            const int c = e / (S * W), ci = (e / W) % S, k = e % W;
            float s = 0.f;
            for (int jr = 0; jr < own_n; ++jr)
                s = fmaf(dyb[(R + jr + SN_GUARD) * 4 + c], A[(R + jr + k - L::H + SN_GUARD) * L::SP + ci], s);
            slab[off_last + e] = wrote ? slab[off_last + e] + s : s;
        }
        if (tid < 3) {
            float s = 0.f;
            for (int jr = 0; jr < own_n; ++jr) s += dyb[(R + jr + SN_GUARD) * 4 + tid];
            float *d = &slab[off_last + 3 * S * W + tid];
            *d = wrote ? *d + s : s;
        }
        float acc[L::RT][4];
#pragma unroll
        for (int i = 0; i < L::RT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;
        for (int k = 0; k < W; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 w = ld4(&wls[(c * W + k) * S + c0]);
#pragma unroll
                for (int i = 0; i < L::RT; ++i) {
                    const float dv = dyb[(r0 + i + L::H - k + SN_GUARD) * 4 + c];
                    acc[i][0] = fmaf(dv, w.x, acc[i][0]), acc[i][1] = fmaf(dv, w.y, acc[i][1]);
                    acc[i][2] = fmaf(dv, w.z, acc[i][2]), acc[i][3] = fmaf(dv, w.w, acc[i][3]);
                }
            }
#pragma unroll
        for (int i = 0; i < L::RT; ++i)
            st4(&D[(r0 + i + SN_GUARD) * L::SP + c0], make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));

        for (int l = depth; l >= 0; --l) {
            __syncthreads();    // the layer above is done with A and Z
#pragma unroll
            for (int i = 0; i < L::RT; ++i) {
                const int j = r0 + i, p = t0 - R + j;
                float4 dz = make_float4(0.f, 0.f, 0.f, 0.f), s = dz;
                if (p >= 0 && p < len) {
                    const float4 t = ld4(&a.saved[(((size_t)l * P + p) * N + n) * S + c0]);
                    const float4 d = ld4(&D[(j + SN_GUARD) * L::SP + c0]);
                    dz.x = d.x * fmaf(-t.x, t.x, 1.f), dz.y = d.y * fmaf(-t.y, t.y, 1.f);
                    dz.z = d.z * fmaf(-t.z, t.z, 1.f), dz.w = d.w * fmaf(-t.w, t.w, 1.f);
                    if (l > 0) {        // a_(l-1), in the forward's order
                        s = ld4(&a.saved[((size_t)p * N + n) * S + c0]);
                        for (int m = 1; m < l; ++m) {
                            const float4 u = ld4(&a.saved[(((size_t)m * P + p) * N + n) * S + c0]);
                            s.x = s.x + u.x, s.y = s.y + u.y, s.z = s.z + u.z, s.w = s.w + u.w;
                        }
                    }
                }
                st4(&Z[(j + SN_GUARD) * L::SP + c0], dz);
                if (l > 0) st4(&A[(j + SN_GUARD) * L::SP + c0], s);
            }
            __syncthreads();
            float *gl = slab + (l == 0 ? 0 : OFF_MID + (l - 1) * MID);
            const int wn = l == 0 ? 3 * S * W : S * S * W;
            if (tid < S) {      // db
                float s = 0.f;
                for (int jr = 0; jr < own_n; ++jr) s += Z[(R + jr + SN_GUARD) * L::SP + tid];
                gl[wn + tid] = wrote ? gl[wn + tid] + s : s;
            }
            if (l == 0) break;
            sn_wgrad_mid<S, W>(Z, A, gl, wrote, R, own_n, tid);
#pragma unroll
            for (int i = 0; i < L::RT; ++i) {
                const float4 d = ld4(&D[(r0 + i + SN_GUARD) * L::SP + c0]);
                acc[i][0] = d.x, acc[i][1] = d.y, acc[i][2] = d.z, acc[i][3] = d.w;
            }
            sn_conv_taps<S, W, false>(Z, a.p.w[l], wt, acc, r0, c0, tid);
#pragma unroll
            for (int i = 0; i < L::RT; ++i)
                st4(&D[(r0 + i + SN_GUARD) * L::SP + c0], make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));
        }

        // layer 0: dw (S, 3, W) and dx
        for (int e = tid; e < 3 * W * S; e += SN_THREADS) {
            const int co = e / (3 * W), ci = (e / W) % 3, k = e % W;
            float s = 0.f;
            for (int jr = 0; jr < own_n; ++jr)
                s = fmaf(Z[(R + jr + SN_GUARD) * L::SP + co], xs[(R + jr + k - L::H + SN_GUARD) * 4 + ci], s);
            slab[e] = wrote ? slab[e] + s : s;
        }
        if (a.dx)
            for (int e = tid; e < own_n * 3; e += SN_THREADS) {
                const int jr = e / 3, ci = e % 3, p = t0 + jr;
                float s = 0.f;
                for (int k = 0; k < W; ++k) {
                    const float *in = Z + (R + jr + L::H - k + SN_GUARD) * L::SP, *w = w0s + (k * 3 + ci) * S;
                    float part = 0.f;
#pragma unroll 4
                    for (int c4 = 0; c4 < S / 4; ++c4) {
                        const float4 v = ld4(&in[4 * c4]), ww = ld4(&w[4 * c4]);
                        part = fmaf(v.w, ww.w, fmaf(v.z, ww.z, fmaf(v.y, ww.y, fmaf(v.x, ww.x, part))));
                    }
                    s += part;
                }
                a.dx[((size_t)p * N + n) * 3 + ci] = p < len ? s : 0.f;
            }
        wrote = true;
    }
    if (!wrote)
        for (unsigned e = tid; e < a.slab_floats; e += SN_THREADS) slab[e] = 0.f;
}

// the slabs added in their order, each gradient written in its parameter's layout
__global__ __launch_bounds__(256) void sn_reduce_kernel(const float *ws, unsigned slab_floats, int slabs, int S, int W,
                                                        int depth, SnGrads g) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= slab_floats) return;
    float v = 0.f;      // blocks of 16 slabs, each summed on its own: no chain longer than 16, then slabs / 16
    for (int p0 = 0; p0 < slabs; p0 += 16) {
        float b = ws[(size_t)p0 * slab_floats + idx];
        const int p1 = p0 + 16 < slabs ? p0 + 16 : slabs;
        for (int p = p0 + 1; p < p1; ++p) b += ws[(size_t)p * slab_floats + idx];
        v = p0 == 0 ? b : v + b;
    }
    const unsigned end = 3u * S * W, off_mid = end + S, mid_w = (unsigned)S * S * W, mid = mid_w + S;
    if (idx < off_mid) {
        if (idx < end) g.w[0][idx] = v;
        else g.b[0][idx - end] = v;
        return;
    }
    unsigned r = idx - off_mid;
    if (r < mid * depth) {
        const unsigned l = 1 + r / mid;
        r %= mid;
        if (r < mid_w) {
            const unsigned k = r / (S * S), ci = (r / S) % S, co = r % S;
            g.w[l][((size_t)co * S + ci) * W + k] = v;
        } else {
            g.b[l][r - mid_w] = v;
        }
        return;
    }
    r -= mid * depth;
    if (r < end) g.w[depth + 1][r] = v;
    else if (r < end + 3) g.b[depth + 1][r - end] = v;
}

template <int S, int W>
int sn_launch(bool backward, const SnArgs &a, int grid, hipStream_t stream) {
    using L = SnLay<S, W>;
    const size_t lds = backward ? L::BWD_LDS : L::FWD_LDS;
    const void *fn = backward ? reinterpret_cast<const void *>(&sn_backward_kernel<S, W>)
                              : reinterpret_cast<const void *>(&sn_forward_kernel<S, W>);
    // more than 64 KB of LDS has to be asked for (per device: asked at every launch, it is no stream operation)
    if (lds > 65536 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return TK_ERR_LAUNCH;
    if (backward)
        hipLaunchKernelGGL((sn_backward_kernel<S, W>), dim3(grid), dim3(SN_THREADS), lds, stream, a);
    else
        hipLaunchKernelGGL((sn_forward_kernel<S, W>), dim3(grid), dim3(SN_THREADS), lds, stream, a);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

int sn_dispatch(bool backward, size_t S, size_t W, const SnArgs &a, int grid, hipStream_t stream) {
#define SN_CASE(s, w) \
    if (S == s && W == w) return sn_launch<s, w>(backward, a, grid, stream);
    SN_CASE(16, 5) SN_CASE(16, 9) SN_CASE(32, 5) SN_CASE(32, 9) SN_CASE(64, 5) SN_CASE(64, 9)
#undef SN_CASE
    return TK_ERR_UNSUPPORTED;
}

inline bool sn_is16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool sn_is4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

bool sn_take_params(void **params, size_t depth, SnParams *out) {
    if (!params) return false;
    for (size_t l = 0; l < depth + 2; ++l) {
        if (!params[2 * l] || !params[2 * l + 1] || !sn_is4(params[2 * l]) || !sn_is4(params[2 * l + 1])) return false;
        out->w[l] = static_cast<const float *>(params[2 * l]);
        out->b[l] = static_cast<const float *>(params[2 * l + 1]);
    }
    return true;
}

}  // namespace

int squiggle_net_forward(const float *x, void **params, const int *lengths, size_t P, size_t N, size_t size,
                         size_t depth, size_t winlen, int cu_count, float *saved, float *y, hipStream_t stream) {
    if (!sn_shape_ok(size, depth, winlen)) return TK_ERR_UNSUPPORTED;
    SnArgs a = {};
    if (!x || !y || !sn_take_params(params, depth, &a.p)) return TK_ERR_BAD_ARG;
    if (!sn_is4(x) || !sn_is4(y) || !sn_is4(lengths) || !sn_is16(saved)) return TK_ERR_BAD_ARG;
    SnPlan p;
    if (!sn_plan(P, N, size, depth, winlen, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    a.x = x, a.lengths = lengths, a.y = y, a.saved = saved;
    a.P = (int)P, a.N = (int)N, a.depth = (int)depth, a.R = p.R, a.tile = p.tile, a.tiles = p.tiles, a.items = (int)p.items;
    return sn_dispatch(false, size, winlen, a, p.fwd_grid, stream);
}

int squiggle_net_backward(const float *dy, const float *x, const float *saved, void **params, const int *lengths,
                          size_t P, size_t N, size_t size, size_t depth, size_t winlen, int cu_count, float *dx,
                          void **grads, void *ws, size_t wsb, hipStream_t stream) {
    if (!sn_shape_ok(size, depth, winlen)) return TK_ERR_UNSUPPORTED;
    SnArgs a = {};
    SnGrads g = {};
    if (!dy || !x || !saved || !grads || !ws || !sn_take_params(params, depth, &a.p)) return TK_ERR_BAD_ARG;
    if (!sn_is4(dy) || !sn_is4(x) || !sn_is4(dx) || !sn_is4(lengths) || !sn_is16(saved) || !sn_is16(ws))
        return TK_ERR_BAD_ARG;
    for (size_t l = 0; l < depth + 2; ++l) {
        if (!grads[2 * l] || !grads[2 * l + 1] || !sn_is4(grads[2 * l]) || !sn_is4(grads[2 * l + 1]))
            return TK_ERR_BAD_ARG;
        g.w[l] = static_cast<float *>(grads[2 * l]), g.b[l] = static_cast<float *>(grads[2 * l + 1]);
    }
    SnPlan p;
    if (!sn_plan(P, N, size, depth, winlen, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    if (wsb < p.bytes) return TK_ERR_WORKSPACE;
    a.dy = dy, a.x = x, a.lengths = lengths, a.dx = dx, a.saved = const_cast<float *>(saved);
    a.ws = static_cast<float *>(ws), a.slab_floats = (unsigned)p.slab_floats;
    a.P = (int)P, a.N = (int)N, a.depth = (int)depth, a.R = p.R, a.tile = p.tile, a.tiles = p.tiles, a.items = (int)p.items;
    const int rc = sn_dispatch(true, size, winlen, a, p.bwd_grid, stream);
    if (rc != TK_OK) return rc;
    hipLaunchKernelGGL(sn_reduce_kernel, dim3((a.slab_floats + 255) / 256), dim3(256), 0, stream,
                       static_cast<const float *>(a.ws), a.slab_floats, p.bwd_grid, (int)size, (int)winlen, (int)depth, g);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // namespace tk

extern "C" {

int tk_squiggle_net_supported(size_t size, size_t depth, size_t winlen) { return tk::sn_shape_ok(size, depth, winlen); }

size_t tk_squiggle_net_workspace_bytes(size_t P, size_t N, size_t size, size_t depth, size_t winlen, int cu_count) {
    tk::SnPlan p;
    return tk::sn_plan(P, N, size, depth, winlen, cu_count, &p) ? p.bytes : 0;
}

int tk_squiggle_net_forward_dev(const float *x, void **params, const int *lengths, size_t P, size_t N, size_t size,
                                size_t depth, size_t winlen, int cu_count, float *saved, float *y, void *stream) {
    return tk::squiggle_net_forward(x, params, lengths, P, N, size, depth, winlen, cu_count, saved, y,
                                    static_cast<hipStream_t>(stream));
}

int tk_squiggle_net_backward_dev(const float *dy, const float *x, const float *saved, void **params,
                                 const int *lengths, size_t P, size_t N, size_t size, size_t depth, size_t winlen,
                                 int cu_count, float *dx, void **grads, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    return tk::squiggle_net_backward(dy, x, saved, params, lengths, P, N, size, depth, winlen, cu_count, dx, grads,
                                     workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
int tk_lab_squiggle_net_plan(size_t P, size_t N, size_t size, size_t depth, size_t winlen, int cu_count, size_t *out) {
    tk::SnPlan p;
    if (!tk::sn_plan(P, N, size, depth, winlen, cu_count, &p)) return 0;
    const size_t v[8] = {(size_t)p.tile, (size_t)p.R, (size_t)p.R, (size_t)p.tiles, (size_t)p.fwd_grid,
                         (size_t)p.bwd_grid, p.slab_floats, p.bytes};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return 1;
}
#endif

}  // extern "C"

// optim.hip -- the optimiser step on the device (gfx950): include/taiyaki_amd_optim.h.
//
// The tail of a train step -- arena.finish's mul_, the gradient maxima and the clamp (clip_kernels.hip), the L2-norm cap
// of bin/train_abinitio.py:219, AdamW and the zero fill of the next step -- as two launches over a tile table.
//
// Why not a library optimiser: torch.optim.AdamW(capturable=True) is about a dozen _foreach passes over 28 to 34 tensors,
// it takes beta1 as a host float (a replayed graph keeps the beta1 of its capture, and the reference's OneCycleLR changes
// beta1 every iteration), it knows nothing of the arena (scale, clamp, cap and fill stay launches of their own), and a host
// without PyTorch has none.  The update is seven float32 streams (g, m, v, p read; g, m, v, p written -- g's write is the
// fill): one pass is all the HBM traffic there has to be.
//
//   launch 1  optim_stats_kernel   per tile: max |g * scale| (NaN if the tile holds one) and the float64 sum of the
//                                  clamped g^2 -> workspace; thread 0 of workgroup 0: the update's scalars from the
//                                  hyper block (float64 arithmetic, one rounding), STEP_NOW = step, step += 1.
//                                  Without maxima and norm: that thread alone.
//   launch 2  optim_update_kernel  per workgroup: the tile sums added in one fixed order (thread j takes tiles j, j + 256,
//                                  ...; then a tree over the 256) -> the cap's factor; per tile: the update; the workgroup
//                                  that owns a segment's first tile folds that segment's tile maxima into maxs[s].
// No workgroup reads a word another workgroup of the same launch writes; no atomics; nothing depends on the grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dispatch.h"
#include "../../include/taiyaki_amd_optim.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TILE = TK_OPTIM_TILE;
constexpr int PER_THREAD = TILE / THREADS;      // 16 elements: four 16-byte accesses per stream
static_assert(TILE % (4 * THREADS) == 0, "a tile is whole 16-byte accesses per thread");
// what launch 1 hands launch 2 (words of the hyper block from TK_OPTIM_STEP_NOW on)
constexpr int D_DECAY = 10, D_W1 = 11, D_B2 = 12, D_W2 = 13, D_STEP_SIZE = 14, D_BC2_SQRT = 15;
static_assert(D_BC2_SQRT < TK_OPTIM_HYPER_WORDS && TK_OPTIM_STEP_NOW < D_DECAY, "hyper block layout");

struct Tile {
    uint32_t seg, first, count, local;
};
static_assert(sizeof(Tile) == 4 * TK_OPTIM_TILE_WORDS, "tile table layout");

struct Partial {        // one per tile, 16 bytes
    double sq;
    float mx;
    float pad;
};

__device__ __forceinline__ bool clamps(float th) { return th >= 0.f && th < __builtin_huge_valf(); }

// steps 1 and 3: the scaled gradient, clamped by tk_grad_maxabs_clip_dev's rule
__device__ __forceinline__ float scaled_clamped(float g, float scale, float th, bool on) {
    const float s = g * scale;
    return on ? fminf(fmaxf(s, -th), th) : s;
}

// (the kernels' own test: dispatch.h's aligned16 is the host's)
__device__ __forceinline__ bool vec16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = fmaxf(x, __shfl_xor(x, d));
    return x;
}

// max over the workgroup of non-negative values, NaN if any thread says `bad`; the result in thread 0
__device__ __forceinline__ float block_max_nan(float m, bool bad, float *part, int *anybad) {
    m = wave_max(m);
    const bool wbad = __any(bad);
    __syncthreads();            // the previous use of part / anybad is over
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6] = m;
        anybad[threadIdx.x >> 6] = wbad;
    }
    __syncthreads();
    float r = part[0];
    int b = anybad[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        r = fmaxf(r, part[w]);
        b |= anybad[w];
    }
    return b ? __builtin_nanf("") : r;
}

__global__ __launch_bounds__(THREADS) void optim_stats_kernel(const float *__restrict__ g, const Tile *__restrict__ tiles,
                                                              unsigned ntiles, float *hyper,
                                                              const float *__restrict__ thresh,
                                                              Partial *__restrict__ part) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double lr = hyper[TK_OPTIM_LR], b1 = hyper[TK_OPTIM_BETA1], b2 = hyper[TK_OPTIM_BETA2];
        const double wd = hyper[TK_OPTIM_WEIGHT_DECAY];
        const float step = hyper[TK_OPTIM_STEP];
        const float t = step + 1.f;
        hyper[D_DECAY] = (float)(1.0 - lr * wd);
        hyper[D_W1] = (float)(1.0 - b1);
        hyper[D_B2] = (float)b2;
        hyper[D_W2] = (float)(1.0 - b2);
        hyper[D_STEP_SIZE] = (float)(lr / (1.0 - pow(b1, (double)t)));
        hyper[D_BC2_SQRT] = (float)sqrt(1.0 - pow(b2, (double)t));
        hyper[TK_OPTIM_STEP_NOW] = step;
        hyper[TK_OPTIM_STEP] = t;
    }
    if (ntiles == 0) return;    // no maxima, no clamp, no norm: that thread was the launch
    __shared__ double sq_s[WAVES];
    __shared__ float mx_s[WAVES];
    __shared__ int bad_s[WAVES];
    const float scale = hyper[TK_OPTIM_GRAD_SCALE];
    const int tid = threadIdx.x;
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const Tile tl = tiles[t];
        const float th = thresh ? thresh[tl.seg] : 0.f;
        const bool on = thresh && clamps(th);
        const float *gp = g + tl.first;
        const int count = (int)tl.count;
        float m = 0.f;
        bool bad = false;
        double sq = 0.0;
        auto take = [&](float x) {
            const float s = x * scale;
            m = fmaxf(m, fabsf(s));
            bad |= !(s == s);
            const float c = on ? fminf(fmaxf(s, -th), th) : s;
            sq += (double)c * (double)c;
        };
        if (vec16(gp)) {
#pragma unroll
            for (int k = 0; k < PER_THREAD / 4; ++k) {
                const int i = (k * THREADS + tid) * 4;
                if (i + 4 <= count) {
                    const float4 x = *reinterpret_cast<const float4 *>(gp + i);
                    take(x.x), take(x.y), take(x.z), take(x.w);
                } else {
                    for (int j = i; j < count; ++j) take(gp[j]);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                const int i = k * THREADS + tid;
                if (i < count) take(gp[i]);
            }
        }
        const float r = block_max_nan(m, bad, mx_s, bad_s);
        sq = wave_sum(sq);
        if ((tid & 63) == 0) sq_s[tid >> 6] = sq;
        __syncthreads();
        if (tid == 0) {
            double total = sq_s[0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) total += sq_s[w];
            Partial p;
            p.sq = total;
            p.mx = r;
            p.pad = 0.f;
            part[t] = p;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void optim_update_kernel(float *__restrict__ g, float *__restrict__ m_all,
                                                               float *__restrict__ v_all, float *const *__restrict__ params,
                                                               const Tile *__restrict__ tiles, unsigned ntiles, float *hyper,
                                                               const float *__restrict__ thresh, float *__restrict__ maxs,
                                                               const Partial *__restrict__ part, int with_norm,
                                                               int zero_grads) {
    __shared__ double red[THREADS];
    __shared__ float mx_s[WAVES];
    __shared__ int bad_s[WAVES];
    const int tid = threadIdx.x;
    const float scale = hyper[TK_OPTIM_GRAD_SCALE], eps = hyper[TK_OPTIM_EPS];
    const float decay = hyper[D_DECAY], w1 = hyper[D_W1], b2 = hyper[D_B2], w2 = hyper[D_W2];
    const float step_size = hyper[D_STEP_SIZE], bc2_sqrt = hyper[D_BC2_SQRT];
    bool cap = false;
    float coef = 1.f;
    if (with_norm) {
        double acc = 0.0;
        for (unsigned t = tid; t < ntiles; t += THREADS) acc += part[t].sq;
        red[tid] = acc;
        __syncthreads();
        for (int s = THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        const float norm = (float)sqrt(red[0]);
        const float max_norm = hyper[TK_OPTIM_MAX_NORM];
        if (max_norm < __builtin_huge_valf()) {          // clip_grad_norm_: a NaN norm makes the factor NaN
            cap = true;
            coef = max_norm / (norm + 1e-6f);
            coef = coef > 1.f ? 1.f : coef;
        }
        if (blockIdx.x == 0 && tid == 0) hyper[TK_OPTIM_GRAD_NORM] = norm;
    }
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const Tile tl = tiles[t];
        if (maxs != nullptr && tl.local == 0) {
            // this segment's tiles follow each other in the table
            float mm = 0.f;
            bool bad = false;
            for (unsigned u = t + tid; u < ntiles && tiles[u].seg == tl.seg; u += THREADS) {
                const float x = part[u].mx;
                bad |= !(x == x);
                mm = fmaxf(mm, x);
            }
            const float r = block_max_nan(mm, bad, mx_s, bad_s);
            if (tid == 0) maxs[tl.seg] = r;
        }
        const float th = thresh ? thresh[tl.seg] : 0.f;
        const bool on = thresh && clamps(th);
        float *gp = g + tl.first, *mp = m_all + tl.first, *vp = v_all + tl.first, *pp = params[tl.seg] + tl.local;
        const int count = (int)tl.count;
        auto one = [&](float &gx, float &mx, float &vx, float &px) {
            float c = scaled_clamped(gx, scale, th, on);
            if (cap) c *= coef;
            float p = px * decay;
            const float mn = fmaf(w1, c - mx, mx);
            const float vn = fmaf(w2 * c, c, b2 * vx);
            const float denom = sqrtf(vn) / bc2_sqrt + eps;
            p = p - step_size * (mn / denom);
            gx = zero_grads ? 0.f : c;
            mx = mn;
            vx = vn;
            px = p;
        };
        if (vec16(gp) && vec16(mp) && vec16(vp) && vec16(pp)) {
#pragma unroll
            for (int k = 0; k < PER_THREAD / 4; ++k) {
                const int i = (k * THREADS + tid) * 4;
                if (i + 4 <= count) {
                    float4 gx = *reinterpret_cast<const float4 *>(gp + i), mx = *reinterpret_cast<const float4 *>(mp + i);
                    float4 vx = *reinterpret_cast<const float4 *>(vp + i), px = *reinterpret_cast<const float4 *>(pp + i);
                    one(gx.x, mx.x, vx.x, px.x), one(gx.y, mx.y, vx.y, px.y);
                    one(gx.z, mx.z, vx.z, px.z), one(gx.w, mx.w, vx.w, px.w);
                    *reinterpret_cast<float4 *>(gp + i) = gx, *reinterpret_cast<float4 *>(mp + i) = mx;
                    *reinterpret_cast<float4 *>(vp + i) = vx, *reinterpret_cast<float4 *>(pp + i) = px;
                } else {
                    for (int j = i; j < count; ++j) one(gp[j], mp[j], vp[j], pp[j]);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                const int i = k * THREADS + tid;
                if (i < count) one(gp[i], mp[i], vp[i], pp[i]);
            }
        }
    }
}

// tiles of the layout, or 0 where it is refused
size_t tile_count(const int64_t *seg_off, size_t nseg) {
    if (seg_off == nullptr || nseg == 0 || seg_off[0] != 0) return 0;
    size_t n = 0;
    for (size_t s = 0; s < nseg; ++s) {
        if (seg_off[s + 1] < seg_off[s]) return 0;
        const uint64_t len = (uint64_t)(seg_off[s + 1] - seg_off[s]);
        if ((uint64_t)seg_off[s + 1] > (1ull << 31)) return 0;
        n += len == 0 ? 1 : (size_t)((len + TILE - 1) / TILE);
    }
    return n;
}

}  // namespace

extern "C" {

size_t tk_optim_tile_count(const int64_t *seg_off, size_t nseg) { return tile_count(seg_off, nseg); }

size_t tk_optim_workspace_bytes(const int64_t *seg_off, size_t nseg) {
    return tile_count(seg_off, nseg) * sizeof(Partial);
}

int tk_optim_tiles(const int64_t *seg_off, size_t nseg, uint32_t *tiles, size_t capacity) {
    const size_t n = tile_count(seg_off, nseg);
    if (n == 0 || tiles == nullptr || capacity < n) return TK_ERR_BAD_ARG;
    Tile *out = reinterpret_cast<Tile *>(tiles);
    for (size_t s = 0; s < nseg; ++s) {
        const uint64_t lo = (uint64_t)seg_off[s], hi = (uint64_t)seg_off[s + 1];
        uint64_t at = lo;
        do {
            const uint64_t cnt = hi - at < (uint64_t)TILE ? hi - at : (uint64_t)TILE;
            *out++ = Tile{(uint32_t)s, (uint32_t)at, (uint32_t)cnt, (uint32_t)(at - lo)};
            at += cnt;
        } while (at < hi);
    }
    return TK_OK;
}

int tk_adamw_step_dev(float *grads, float *exp_avg, float *exp_avg_sq, const void *params, const uint32_t *tiles,
                      size_t ntiles, size_t nseg, size_t total, float *hyper, const float *thresh, float *maxs,
                      void *workspace, size_t workspace_bytes, int with_norm, int zero_grads, int cu_count, void *stream) {
    if (grads == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr || params == nullptr || tiles == nullptr ||
        hyper == nullptr || workspace == nullptr)
        return TK_ERR_BAD_ARG;
    // (a tile table of this layout has between nseg and nseg + total / TILE tiles)
    if (nseg == 0 || ntiles < nseg || total > ((size_t)1 << 31) || ntiles > nseg + total / TILE || cu_count <= 0)
        return TK_ERR_BAD_ARG;
    if (!tk::aligned16(workspace)) return TK_ERR_BAD_ARG;
    if (workspace_bytes < ntiles * sizeof(Partial)) return TK_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // thresholds alone need no statistics: the update clamps by itself, and nothing would read the tile results
    const bool stats = maxs != nullptr || with_norm != 0;
    const size_t cap = (size_t)cu_count * 8;
    const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
    const Tile *tl = reinterpret_cast<const Tile *>(tiles);
    Partial *part = static_cast<Partial *>(workspace);
    hipLaunchKernelGGL(optim_stats_kernel, dim3(stats ? grid : 1), dim3(THREADS), 0, st, grads, tl,
                       stats ? (unsigned)ntiles : 0u, hyper, thresh, part);
    hipLaunchKernelGGL(optim_update_kernel, dim3(grid), dim3(THREADS), 0, st, grads, exp_avg, exp_avg_sq,
                       static_cast<float *const *>(params), tl, (unsigned)ntiles, hyper, thresh, maxs, part,
                       with_norm != 0, zero_grads != 0);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // extern "C"

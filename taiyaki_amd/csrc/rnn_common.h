// rnn_common.h -- what the persistent recurrences (lstm_kernels.hip, gru_kernels.hip) share: the granule hand-off
// between the workgroups of a group, the block placement, the register and LDS helpers of the step schedule and
// the kernel that zeroes the granule buffers in front of every launch.
//
// Hand-off.  8-byte granules {value, tag} written by ONE sc1 store and read by sc1 loads until every tag matches
// (cdna_hip_programming.md Guideline 16, R2: the data is the flag, no fence).  Tag = step + 1, two slots by step
// parity: no member can publish step s + 2 before every member has read step s.  The granule buffers are zeroed by
// a kernel in front of every launch.  Every spin is bounded by a clock budget; on expiry TK_STATUS_RNN_TIMEOUT is
// OR-ed into *status and the whole grid leaves (the other spins see the bit).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/taiyaki_amd_flipflop.h"

namespace tk {
namespace {

constexpr uint64_t kSpinTicks = 200000000ull;   // 2 s of s_memrealtime (100 MHz) per wait

// The columns of a launch: n of them, in tensors that hold ld >= n columns per time step (row (t, column) is row
// t * ld + column of a tensor; the pointers, `lengths` among them, stand at the launch's first column).  ld != n is a
// window of columns of a wider batch (DESIGN.md "Batches wider than one launch"), which the -DTK_RNN_WIDE build and the
// -DTK_LSTM_LARGE build of lstm_kernels.hip alone launch (TK_RNN_SLABS): there ld is a kernel argument.  In every other
// build ld is n itself, as a kernel argument this is one int, and the kernels are instruction for instruction what they
// were when they took n alone.
#if defined(TK_RNN_WIDE) || defined(TK_LSTM_LARGE)
#define TK_RNN_SLABS 1
#endif

struct Cols {
    int n;
#ifdef TK_RNN_SLABS
    int pitch;
    __host__ __device__ int ld() const { return pitch; }
#else
    __host__ __device__ int ld() const { return n; }
#endif
};

inline Cols make_cols(size_t n, size_t ld) {
#ifdef TK_RNN_SLABS
    return Cols{(int)n, (int)ld};
#else
    return Cols{(int)n};
#endif
}

// p advanced to column `first` of a tensor with `width` floats per column (lengths: width 1); NULL stays NULL
template <class P>
P *at_column(P *p, size_t first, size_t width) {
    return p ? p + first * width : p;
}

// The slab rule (DESIGN.md "Batches wider than one launch").  A batch wider than one launch admits runs as slabs of S
// columns, slab k being columns [k S, min((k + 1) S, N)), one launch after the other on the caller's stream.  S is the
// widest batch the cell's admission rule admits at (size, cu_count); that rule is monotone in N, so S is found from the
// rule itself, by bisection, and is never restated.  0: the rule admits no batch; INT32_MAX: it admits every batch.
template <class Admits>
size_t widest_admitted(Admits admits) {
    size_t lo = 1, hi = (size_t)INT32_MAX;
    if (!admits(lo)) return 0;
    if (admits(hi)) return hi;
    while (hi - lo > 1) {                              // admits(lo) && !admits(hi)
        const size_t mid = lo + (hi - lo) / 2;
        (admits(mid) ? lo : hi) = mid;
    }
    return lo;
}

typedef unsigned long long u64;
typedef __attribute__((address_space(1))) u64 gu64;
typedef __attribute__((address_space(1))) uint32_t gu32;

__device__ __forceinline__ void store_granule(u64 *g, unsigned tag, float v) {
    __hip_atomic_store((gu64 *)g, ((u64)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// This lane's NG granules g[e0 + q * stride] that lie below `end` until every lane of the wave sees `tag` in all
// of its own; false when the clock budget runs out or another workgroup has already given up.  Every pass issues
// all NG loads before it waits (a granule at or past `end` is read at g[0] and ignored: no branch per load).
template <int NG>
__device__ __forceinline__ bool sweep(const u64 *g, int e0, int stride, int end, unsigned tag, float (&v)[NG],
                                      uint32_t *status) {
    const uint64_t start = __builtin_amdgcn_s_memrealtime();
    for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            const int e = e0 + q * stride;
            const bool in = e < end;
            const u64 x = __hip_atomic_load((gu64 *)(g + (in ? e : 0)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v[q] = __uint_as_float((unsigned)x);
            ok &= !in || (unsigned)(x >> 32) == tag;
        }
        if (__all(ok)) return true;
        if ((spins & 31) == 31) {
            const uint32_t st = __hip_atomic_load((gu32 *)status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((st & TK_STATUS_RNN_TIMEOUT) || __builtin_amdgcn_s_memrealtime() - start > kSpinTicks) {
                __hip_atomic_fetch_or((gu32 *)status, TK_STATUS_RNN_TIMEOUT, __ATOMIC_RELAXED,
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

// Values loaded from HBM, pinned as ready here: the compiler waits for their loads at this point, not at their first
// use after a later prefetch (vmcnt is in order, so that wait would also wait for the prefetch).
template <int M>
__device__ __forceinline__ void settle(float (&v)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) asm volatile("" : "+v"(v[i]));
}
template <int M, int K>
__device__ __forceinline__ void settle(float (&v)[M][K]) {
#pragma unroll
    for (int i = 0; i < M; ++i) settle(v[i]);
}

// A running pointer of the step schedule, advanced at the top of a step: pinned as advanced there, in front of the poll
// (left alone, the compiler sinks the addition to the pointer's first use, behind the barrier).  Typed as a pointer to
// global memory: behind the pin the compiler no longer sees where the pointer came from, and a plain one would be read
// through flat instructions.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float gcfloat;

template <class P>
__device__ __forceinline__ void settle_ptr(P *&p) {        // P: gfloat, gcfloat, gu64
    asm volatile("" : "+v"(p));
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// C consecutive floats of LDS (16-byte aligned where C is a multiple of 4)
template <int C>
__device__ __forceinline__ void lds_row(const float *p, float (&v)[C]) {
    if constexpr (C % 4 == 0) {
#pragma unroll
        for (int c4 = 0; c4 < C / 4; ++c4) {
            const float4 q = reinterpret_cast<const float4 *>(p)[c4];
            v[4 * c4 + 0] = q.x;
            v[4 * c4 + 1] = q.y;
            v[4 * c4 + 2] = q.z;
            v[4 * c4 + 3] = q.w;
        }
    } else if constexpr (C == 2) {
        const float2 q = *reinterpret_cast<const float2 *>(p);
        v[0] = q.x;
        v[1] = q.y;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = p[c];
    }
}

// Row staging.  The cell lanes of a forward step are a few lanes of every wave, so a store of theirs reaches global
// memory as 32-byte pieces.  They write a step's bulk outputs into an LDS block of rows of U floats instead (U a
// multiple of 4, the block 16-byte aligned), and behind the next barrier the block leaves as whole rows: lane tid of nt
// moves the 16-byte chunks tid + i * nt, i < NQ, chunk q being floats [4 (q % (U / 4)), + 4) of row q / (U / 4).
// dst[i] is where chunk i goes at time 0 (NULL: a chunk past the block or of a column past N, not stored), pitch[i]
// its tensor's floats per time step.  One dwordx4 per chunk; the tensors need no more than a float's alignment.
typedef float row_chunk __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) row_chunk grow_chunk;          // ... through a running pointer (settle_ptr)

template <int NQ>
__device__ __forceinline__ void rows_to_global(const float *blk, int tid, int nt, float *const (&dst)[NQ],
                                               const size_t (&pitch)[NQ], size_t t) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        if (!dst[i]) continue;
        const float4 v = reinterpret_cast<const float4 *>(blk)[tid + i * nt];
        *reinterpret_cast<row_chunk *>(dst[i] + t * pitch[i]) = row_chunk{v.x, v.y, v.z, v.w};
    }
}

__global__ void zero_u64x2_kernel(uint4 *p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// Zeroes the granule buffers (`bytes` a multiple of 16) on `stream`, in front of the launch that polls them.
int zero_ws(void *ws, size_t bytes, hipStream_t stream) {
    // (a kernel, not hipMemsetAsync: see clip_kernels.hip on memset nodes replayed from a hipGraph)
    const size_t n = bytes / 16;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(zero_u64x2_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<uint4 *>(ws), n);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // namespace
}  // namespace tk

// basecall_mods.hip -- the modified-base weights of every read's call (include/taiyaki_amd_basecall.h, (f);
// flipflopfings.py:100-143 extract_mod_weights on the stitched path and the stitched categorical columns): one
// workgroup per read, the tail's walk over the stitched rows (basecall_walk.h), so a read's row count is its call length.
//
// A pure selection: 32-bit words are copied, never computed with; the columns of the other bases get the quiet NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/taiyaki_amd_basecall.h"
#include "basecall_walk.h"
#include "dispatch.h"

namespace tk {

constexpr uint32_t QUIET_NAN = 0x7fc00000u;

// Lane mapping.  A weight row is ncat adjacent floats (24 bytes at ACGT + 2 mods), the next stitched row's sits
// nchunks * ncat floats further on: whatever the mapping, a move's row costs one 64-byte segment of its own, so the
// reads cannot be made contiguous across rows and are left to the cache.  The WRITES can: the walk leaves one word per
// move of the tile in LDS -- where its weight row starts and which base it moved into, 9 bytes, not the row -- and the
// tile's output, (moves of the tile) x nmod words at consecutive addresses, is then written flat, lane e -> (move e /
// nmod, column e % nmod): consecutive lanes write consecutive words and read adjacent floats of one weight row.
__global__ __launch_bounds__(BC_THREADS) void mod_weights_kernel(WalkArgs walk, const uint32_t *__restrict__ weights,
                                                                 uint32_t ncat, uint32_t nbase, uint32_t nmod,
                                                                 ModColumns cols, const int64_t *__restrict__ out_off,
                                                                 uint32_t *__restrict__ mods,
                                                                 int32_t *__restrict__ seqlen,
                                                                 uint32_t *__restrict__ status) {
    __shared__ WalkShared ws;
    __shared__ int64_t move_src[BC_THREADS];        // first word of the move's weight row; < 0: there is none
    __shared__ uint8_t move_base[BC_THREADS];
    __shared__ uint8_t col_base[TK_BASECALL_MAX_NMOD], col_src[TK_BASECALL_MAX_NMOD];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid < (int)nmod) {
        col_base[tid] = cols.base[tid];
        col_src[tid] = cols.src[tid];
    }
    int64_t obeg = out_off[r], room = out_off[r + 1] - obeg;
    if (obeg < 0) room = 0;                         // (nothing is written in front of the buffer)
    const int64_t nblk = walk.nrow - 1, nchunks = walk.nchunks;
    bool overflow = false;
    __syncthreads();
    const int64_t count = walk_moves(
        walk, r, room, ws, &overflow,
        [&](int64_t at, int64_t st, int64_t, int64_t, int64_t prow, int64_t pc) {
            // (`at` minus the tile's first position is below BC_THREADS: a tile has at most that many moves)
            const int slot = (int)(at & (BC_THREADS - 1));
            // the weights have one row fewer than the path: a stitched row k - 1 that is its chunk's row nblk (cuts
            // that run past a chunk's blocks) has no weight row, and the move gets NaNs
            move_src[slot] = prow < nblk ? (prow * nchunks + pc) * (int64_t)ncat : -1;
            move_base[slot] = (uint8_t)((uint64_t)st % nbase);
        },
        [&](int64_t first, int64_t n) {
            uint32_t *dst = mods + (obeg + first) * (int64_t)nmod;
            for (int64_t e = tid; e < n * nmod; e += BC_THREADS) {
                const int64_t i = e / nmod;
                const uint32_t j = (uint32_t)(e - i * nmod);
                const int slot = (int)((first + i) & (BC_THREADS - 1));
                const int64_t src = move_src[slot];
                dst[e] = (src >= 0 && col_base[j] == move_base[slot]) ? weights[src + col_src[j]] : QUIET_NAN;
            }
        });
    if (overflow && status) atomicOr(status, TK_STATUS_CHUNK_PLAN);
    if (tid == 0) seqlen[r] = call_length(count, room);
}

int mod_weights_dispatch(const int64_t *path, const float *mod_weights, size_t nblk, size_t nchunks, size_t ncat,
                         const int64_t *chunk_starts, const int64_t *chunk_ends, const int64_t *read_chunk_off,
                         const float *read_scale, size_t nread, size_t stride, size_t nbase, size_t nmod,
                         const ModColumns &cols, const int64_t *out_off, float *mods, int32_t *seqlen,
                         uint32_t *status, hipStream_t stream) {
    const WalkArgs walk = {path, (int64_t)nblk + 1, (int64_t)nchunks, chunk_starts, chunk_ends, read_chunk_off,
                           read_scale, (int64_t)stride};
    hipLaunchKernelGGL(mod_weights_kernel, dim3((unsigned)nread), dim3(BC_THREADS), 0, stream, walk,
                       reinterpret_cast<const uint32_t *>(mod_weights), (uint32_t)ncat, (uint32_t)nbase, (uint32_t)nmod,
                       cols, out_off, reinterpret_cast<uint32_t *>(mods), seqlen, status);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // namespace tk

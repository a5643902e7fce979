// basecall_walk.h -- what the basecaller's per-read kernels share (basecall_kernels.hip: the tail and the stitched
// scores; basecall_mods.hip: the modified-base weights): the stitching cuts, and the walk over a read's stitched rows
// that finds its moves.  ONE copy of each, so the kernels agree on every cut and on every read's call length by
// construction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tk {

constexpr int BC_WAVE = 64;
constexpr int BC_THREADS = 256;
constexpr int BC_WAVES = BC_THREADS / BC_WAVE;

// basecall_helpers.py:64-94, path_stitching=False: the rows [lo, hi) that stitching keeps of chunk `c`, the i-th of its
// read's `nch` chunks of `nrow` rows -- the reference's integer floor divisions for the first, middle and last chunk;
// a read of one chunk keeps all its rows.  (hi < lo where the cuts cross: no rows.)
__device__ __forceinline__ void chunk_cut(const int64_t *__restrict__ starts, const int64_t *__restrict__ ends,
                                          int64_t c, int64_t i, int64_t nch, int64_t stride, int64_t nrow,
                                          int64_t *lo_out, int64_t *hi_out) {
    int64_t lo = 0, hi = nrow;
    if (nch > 1) {
        const int64_t s = starts[c], e = ends[c];
        if (i == 0) {
            lo = s / stride;
            hi = (e + starts[c + 1]) / (2 * stride);
        } else {
            lo = (ends[c - 1] - s) / (2 * stride);
            hi = i == nch - 1 ? (e - s) / stride : (e + starts[c + 1] - 2 * s) / (2 * stride);
        }
    }
    *lo_out = lo < 0 ? 0 : lo;
    *hi_out = hi > nrow ? nrow : hi;
}

// the per-chunk Viterbi paths of a launch and the geometry of its reads
struct WalkArgs {
    const int64_t *path;            // (nrow, nchunks) flip-flop states
    int64_t nrow, nchunks;
    const int64_t *starts, *ends;   // (nchunks)
    const int64_t *read_chunk_off;  // (nread + 1)
    const float *read_scale;        // (nread) or NULL: NaN = a refused read, no rows
    int64_t stride;
};

struct WalkShared {
    uint32_t wave_moves[BC_WAVES];
    int64_t last_state;             // state of the last stitched row so far
};

// The stitched rows of read `r`, one workgroup of BC_THREADS threads, tiles of BC_THREADS rows of one chunk: stitched
// row k >= 1 is a MOVE when its state differs from stitched row k - 1 (across a cut the two rows come from different
// chunks); a move's position in the call is the count carried between tiles + the moves of the lower waves + the lower
// lanes of its wave's ballot.  Per tile:
//   on_move(at, state, row, c, prow, pc)   in the thread of a move with at < room: `at` its position in the call,
//                                  (row, c) the row and chunk of `path` that hold stitched row k, (prow, pc) those
//                                  that hold stitched row k - 1;
//   a barrier;
//   on_tile(first, n)              in every thread: the tile held the moves first .. first + n - 1 of those that fit the
//                                  room.  What on_move left in shared memory may be read here; the next tile's on_move
//                                  calls come after a barrier that every thread reaches behind its on_tile.
// Returns the read's moves (the same in every thread); *overflow is set in the threads whose move did not fit `room`.
template <class OnMove, class OnTile>
__device__ __forceinline__ int64_t walk_moves(const WalkArgs &a, int r, int64_t room, WalkShared &s, bool *overflow,
                                              OnMove on_move, OnTile on_tile) {
    const int tid = threadIdx.x, wave = tid / BC_WAVE, lane = tid & (BC_WAVE - 1);
    int64_t cbeg = a.read_chunk_off[r], cend = a.read_chunk_off[r + 1];
    cbeg = cbeg < 0 ? 0 : cbeg;
    cend = cend > a.nchunks ? a.nchunks : cend;
    const bool refused = a.read_scale && a.read_scale[r] != a.read_scale[r];
    const int64_t nch = refused ? 0 : cend - cbeg;
    int64_t count = 0;                      // moves so far (the same in every thread)
    bool any_row = false;                   // a stitched row exists already (uniform)
    int64_t last_row = 0, last_chunk = 0;   // where the last stitched row so far sits in `path` (uniform)
    for (int64_t i = 0; i < nch; ++i) {
        const int64_t c = cbeg + i;
        int64_t lo, hi;
        chunk_cut(a.starts, a.ends, c, i, nch, a.stride, a.nrow, &lo, &hi);
        for (int64_t base = lo; base < hi; base += BC_THREADS) {
            const int64_t row = base + tid;
            const bool live = row < hi;
            int64_t st = 0, prev = 0;
            bool move = false;
            if (live) {
                st = a.path[row * a.nchunks + c];
                const bool has_prev = row > lo || any_row;
                prev = row > lo ? a.path[(row - 1) * a.nchunks + c] : s.last_state;
                move = has_prev && st != prev;
            }
            const uint64_t mask = __ballot(move);
            if (lane == 0) s.wave_moves[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            int64_t at = count, total = 0;
            for (int w = 0; w < BC_WAVES; ++w) {
                if (w < wave) at += s.wave_moves[w];
                total += s.wave_moves[w];
            }
            if (move) {
                at += __popcll(mask & ((1ull << lane) - 1ull));
                if (at < room)
                    on_move(at, st, row, c, row > lo ? row - 1 : last_row, row > lo ? c : last_chunk);
                else
                    *overflow = true;
            }
            if (live && row == hi - 1) s.last_state = st;
            any_row = true;
            __syncthreads();
            const int64_t fit = room - count;
            on_tile(count, fit < 0 ? 0 : (fit < total ? fit : total));
            count += total;
        }
        if (hi > lo) {
            last_row = hi - 1;
            last_chunk = c;
        }
    }
    return count;
}

// what a read reports as its call length: its moves, or its room where they did not fit
__device__ __forceinline__ int32_t call_length(int64_t count, int64_t room) {
    return (int32_t)(count < room ? count : (room < 0 ? 0 : room));
}

}  // namespace tk

// squiggle_match.h -- the launch arguments of the squiggle-match kernels (squiggle_kernels.hip),
// shared with the C ABI (c_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace tk {

struct SqArgs {
    const float *params;        // (npos, nbatch, 3): level, log-scale, move logit
    const float *signal;        // all reads back to back
    const int32_t *siglen;      // (nbatch)
    const int64_t *sig_off;     // (nbatch + 1) exclusive prefix sum of siglen
    int nbatch;
    int npos;
    int64_t nsignal;            // length of `signal`
    float prob_back;
    float localpen, minscore;   // Viterbi only
    float *cost;                // (nbatch) negated score (nullable for the backward sweep)
    float *grad;                // (npos, nbatch, 3) negated gradient
    int32_t *path;              // (nsignal) Viterbi path
    float *lattice;             // forward columns: read b's start at (sig_off[b] + b) * 2 * 64 R floats
    uint8_t *tb;                // Viterbi traceback: 64 R bytes per sample
    int32_t *endtb;             // Viterbi traceback of the end state: one per sample
    uint32_t *status;
};

// positions per lane the kernels use for npos (0: beyond the build's limit)
int sq_positions_per_lane(size_t npos);
size_t sq_lattice_bytes(size_t npos, size_t nbatch, size_t nsignal);
size_t sq_path_bytes(size_t npos, size_t nsignal);
// which: 0 cost, 1 cost + stored lattice, 2 backward over a stored lattice, 3 Viterbi
int squiggle_dispatch(int which, const SqArgs &a, hipStream_t stream);

}  // namespace tk

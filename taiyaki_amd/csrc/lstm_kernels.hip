// lstm_kernels.hip -- the recurrence of layers.Lstm (one nn.LSTM layer, gate order i, f, g, o; h0 = c0 = 0)
// as one persistent, weight-stationary launch per layer and direction of the pass.
//
// Geometry.  A workgroup owns U hidden units (their 4 U gate rows of W_hh, held in VGPRs for the whole launch) and
// C batch columns.  The G = H / U workgroups that share C columns form a group; a group needs nothing from another
// group.  The admission rule and the workspace size are those of U = 16 with 8 or 16 columns (lstm_geometry); a
// launch at U = 32 or 64 takes C * 16 / U columns per workgroup, so its grid and its granule buffers are never
// larger than the admitted ones (lstm_plan).  H = 192 and 384 are not multiples of 64: there a workgroup owns U = 48
// units and 4 (H 192: or 8) columns, and the admission geometry is the launch's own (lstm_geometry).
//
// Hand-off.  Inside a group every step is an all-to-all: forward, each member needs the whole h_{t-1} of its
// columns; backward, each member needs the sum over members of W_hh[rows(m), J]^T dG_{t+1}[rows(m)] for its units J
// (a reduce-scatter, summed in producer order: bit-reproducible).  Both go through the tagged granules of
// rnn_common.h (its header has the protocol, the zeroing in front of every launch and the bounded spin).
//
// Step schedule.  vmcnt is one in-order counter per wave for loads and stores, so every wait of a poll also waits
// for whatever the wave issued before it.  Nothing bound for HBM is issued ahead of a poll in the same step: the
// inputs of step s + 1 (forward: gx; backward: dy, c_{t-1}, the gates) are loaded right after step s's poll, and
// the bulk outputs of step s (forward: y, c, gates; backward: dG) are held back and stored right after step s + 1's
// poll.  Both drain under the matvec; the granule publish is the last memory operation of a step.  The backward
// holds them in registers (its cell lanes are (column, unit), unit contiguous: whole rows as they are).  The
// forward's cell lanes are kp < C of every KP lanes, 32-byte pieces of a row per store, so they stage the six values
// in LDS and the workgroup stores the block as whole rows, 16 bytes per lane (rows_to_global, rnn_common.h): 3 store
// instructions per workgroup and step at H 256, U 64, C 2 where the cell lanes issued 48.
// What a step computes without the hand-off stands in front of its poll, where the wave would only wait (the forward at
// H 256, U 64, C 2 and every backward): the addresses, as running pointers advanced once per step, and in the backward
// tanh(c_t) and the factors of the gate derivatives; behind the barrier stand the memory instructions alone and what
// needs the gathered values.  give_up is read behind the barrier by every wave and tested once, in front of the
// publish: no wait for it stands on the chain (DESIGN.md "Step schedule" has the argument for the path it guards).
//
// Columns.  A launch works on `cols.n` columns of tensors that hold `cols.ld()` columns per time step (rnn_common.h:
// Cols).  The two are one number everywhere but in the -DTK_RNN_WIDE build, which runs a batch wider than the admission
// rule takes as slabs of columns, one admitted launch after the other, in place (`checked`; lstm_slab).
//
// Four builds of this one source.  -DTK_RNN_WIDE (libtaiyaki_amd_rnn_wide.so) takes the three VL forms, the saving
// forward, the forward with nothing saved and the backward, with the tensors' columns per time step as a kernel argument
// of its own (DESIGN.md "Batches wider than one launch").  The flip-flop library takes the training pair: the forward that saves the gates
// and c, and the backward.  -DTK_RNN_VARLEN (libtaiyaki_amd_rnn_varlen.so) takes the forward alone in its VL form with
// nothing saved: per-column lengths, y the only output (DESIGN.md "Variable-length recurrences").
// -DTK_RNN_VARLEN_TRAIN (libtaiyaki_amd_rnn_varlen_train.so) takes the training pair in its VL form: the saving forward
// and the backward with per-column lengths (DESIGN.md "Training through variable-length batches").
// A fifth, -DTK_LSTM_LARGE (libtaiyaki_amd_lstm_large.so), is hidden size 512 and nothing else: the three VL forms at
// (512, 32, 4) and (512, 32, 8), 512 lanes per workgroup, with a geometry of its own and the slabs of the -DTK_RNN_WIDE
// build (DESIGN.md "LSTM at size 512").  What it needs stands under its #ifdef or is a template argument that no other
// build instantiates: the other builds' objects do not change with it.
#include "dispatch.h"
#include "ff_common.h"
#include "lstm_bwd_layout.h"
#include "lstm_fwd_layout.h"
#include "rnn_common.h"

namespace tk {
namespace {

// threads per workgroup at U units: 4 U H / threads W_hh floats per lane, <= 128 at H = 256; U = 48 (H 192, 384): the
// forward's lanes (u, kp) at KP = 8, 192 floats per lane at H = 384
template <int U>
constexpr int threads_for() { return U == 48 ? 384 : U <= 32 ? 256 : 512; }
// ... of the forward at (H, U): H = 512 (-DTK_LSTM_LARGE alone instantiates it) takes 512 lanes at U = 32, lanes (u, kp)
// at KP = 16, so that a lane holds the 128 floats of (256, 64) and not 256
template <int H, int U>
constexpr int fwd_threads_for() { return H == 512 ? 512 : threads_for<U>(); }
// ... of the backward: two lanes per column of W_hh at U = 48, 96 floats per lane at either size; H = 512: one lane per
// column (RP 1), 4 U = 128 floats per lane
template <int H, int U>
constexpr int bwd_threads_for() { return U == 48 ? 2 * H : fwd_threads_for<H, U>(); }

// The value of lane (lane ^ M) of the wave.  M = 1 and 2 are one quad permutation, M = 4 a mirror of the half row and a
// reversal of the quad (i -> 7 - i -> i ^ 4): DPP operands of the VALU, which the compiler folds into the add that uses
// them where it can.  They stay off the LDS crossbar, where a ds_bpermute_b32 takes its turn behind the matvec's reads.
template <int M>
__device__ __forceinline__ float xor_lane(float v) {
    static_assert(M == 1 || M == 2 || M == 4, "a partner inside the lane's group of 8");
    const int x = __float_as_int(v);
    if constexpr (M == 1) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));      // quad_perm:[1,0,3,2]
    } else if constexpr (M == 2) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));      // quad_perm:[2,3,0,1]
    } else {
        const int y = __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true);              // row_half_mirror
        return __int_as_float(__builtin_amdgcn_update_dpp(0, y, 0x1B, 0xF, 0xF, true));      // quad_perm:[3,2,1,0]
    }
}

// Recursive halving over the lanes rq ^ M, M = M0, 2 M0, ... < RQ (lstm_bwd_layout.h): each round a lane keeps the
// half of its remaining accumulators that its bit of rq names, and adds its partner's partial sums of that half.
template <int M, int RQ, int NA>
__device__ __forceinline__ void halve_rounds(float (&acc)[NA], int rq) {
    if constexpr (M < RQ) {
        constexpr int n = NA / (2 * M);
        const bool up = (rq & M) != 0;
#pragma unroll
        for (int a = 0; a < n; ++a) {
            const float send = up ? acc[a] : acc[a + n];
            const float keep = up ? acc[a + n] : acc[a];
            acc[a] = keep + xor_lane<M>(send);
        }
        halve_rounds<2 * M, RQ>(acc, rq);
    }
}

// Two floats in one aligned 64-bit register pair, and the matvec's fused multiply-add on both halves at once.  At C 2 the
// two batch columns of a group are the halves: acc(c0, c1) += w * d(c0, c1), one v_pk_fma_f32 where two v_fma_f32 stood.
// Each half rounds as fmaf does and no sum changes its operands or their order, so every bit stays.  The weight is one
// half of a pair of two consecutive weights, broadcast to both halves of the product by the instruction's op_sel bits:
// pk_fma_lo takes w[0], pk_fma_hi w[1].  Written as asm, one statement per instruction, because a splat of the weight
// (__builtin_elementwise_fma) costs a register pair per weight, which 128 weights per lane do not have; not volatile, so
// the compiler schedules them and places the waits for the LDS reads as for plain FMAs.  The backward's block path at C 2
// takes it (0.09 us per step); the forward at (256, 64, 2) gave the same bits 0.48 us per step slower and keeps its plain
// FMAs (DESIGN.md "Packed-FMA matvec", profiles/r50_lstm_packed.txt).
typedef float pair2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void pk_fma_lo(pair2 &acc, pair2 w, pair2 h) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(w), "v"(h));
}
__device__ __forceinline__ void pk_fma_hi(pair2 &acc, pair2 w, pair2 h) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(w), "v"(h));
}
// (as settle, rnn_common.h: the pairs formed once, in front of the step loop, and kept as pairs)
template <int M>
__device__ __forceinline__ void settle_pairs(pair2 (&v)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) asm volatile("" : "+v"(v[i]));
}

// The forward at H 256, U 64, C 2 (lstm_fwd_kernel below has the contract, the schedule of a step and the VL and SAVE
// forms; lstm_fwd_layout.h the arithmetic of this layout and the order of every sum, which is that of the plain body).
// Written over CK = C / 2 columns per lane; at C 4 (CK 2) it gives the plain body's bits too but measured slower than
// it (lstm_fwd_layout.h), so only C 2 comes here.  Three things differ from the plain body, all on a step's serial chain:
//   * h in LDS: two rows of a lane side by side at C 2, so the matvec reads 16 bytes at a time, 16 ds_read_b128 per lane
//     and step where it issued 16 ds_read2_b64 (8 LDS-array cycles each, against 4);
//   * the KP = 8 partial sums meet by recursive halving over xor 1, 2, 4, DPP operands of the adds (halve_rounds, as in
//     the backward), where 12 (C 4: 16) ds_bpermute_b32 queued behind the matvec's reads; a lane is left with the sums
//     of ONE gate in CK = C / 2 columns;
//   * every lane adds its own gx to those sums and applies its gate's function, so a wave issues one sigmoidf body and,
//     for the lanes of gate g, one tanhf body where the cell lanes issued three and one; the lane of gate i takes the
//     other three activations of its columns from the lanes kp ^ 4 (f), kp ^ 2 (g) and kp ^ 6 (o) by DPP moves and
//     runs the cell update, the publish and the staging as the plain body's cell lane does.
// And the step's schedule keeps off the chain what does not depend on the hand-off (the file's header): running pointers
// advanced in front of the poll, give_up and the staged rows read behind the matvec's leading reads, the rows stored
// behind the first group of FMAs, give_up tested once in front of the cell update.
template <int H, int C, int U, bool VL, bool SAVE>
__device__ __forceinline__ void lstm_fwd_lanes_body(const float *__restrict__ gx, const float *__restrict__ whh, int T,
                                                    Cols cols, int reverse, int ngroups, float *__restrict__ y,
                                                    float *__restrict__ gates, float *__restrict__ cell, u64 *hbuf,
                                                    uint32_t *status, const int32_t *__restrict__ lengths) {
    constexpr int NT = threads_for<U>();
    const int N = cols.n, LD = cols.ld();               // the launch's columns; the tensors' columns per time step
    constexpr int G = H / U;
    constexpr LstmFwdLanes FL(NT, H, U, C);
    constexpr int KP = FL.KP, KS = FL.KS, PR = FL.PR, CK = FL.CK;
    constexpr int NG = H * C / NT;
    static_assert(FL.ok() && KP == 8 && NG * NT == H * C && FL.gate_lane_xor(1) == 4 && FL.gate_lane_xor(2) == 2 &&
                      FL.gate_lane_xor(3) == 6,
                  "whole rows in 16-byte reads; the partial sums and the four gates of a column inside 8 lanes of a wave");
    constexpr int U4 = U / 4;
    constexpr int NQ = SAVE ? (6 * C * U4 + NT - 1) / NT : 1;        // 16-byte chunks of a staging block per lane
    static_assert(U % 4 == 0, "a row of the staging block is whole 16-byte chunks");
    __shared__ __attribute__((aligned(16))) float hs[2][H * C];      // h_{t-1} at FL.hs_index(k, c), by step parity
    // a step's h, c, i, f, g, o as [value][column][unit], by step parity (as in the plain body)
    __shared__ __attribute__((aligned(16))) float stg[SAVE ? 2 : 1][SAVE ? 6 * C * U : 4];
    __shared__ int give_up;

    int group, member;
    place(G, group, member);
    const int tid = threadIdx.x;
    const int j0 = member * U, n0 = group * C;
    const int u = tid / KP, kp = tid % KP;

    float w[4][KS];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < KS; ++i) w[g][i] = whh[((size_t)g * H + j0 + u) * H + FL.k(kp, i)];
    settle(w);

    const int gate = FL.gate(kp), col = FL.col(kp, 0);  // this lane keeps the sums of `gate` in columns col + v, v < CK
    const bool cell_lane = gate == 0;
    const int n = n0 + col;
    bool fetch[CK], valid[CK];                         // a column of the batch: its gx is loaded; ... and this is its cell lane
    float cst[CK], held[CK];                           // held: not SAVE, h of the previous step, stored one step late
    int len[CK];                                       // VL: the steps of this lane's columns
#pragma unroll
    for (int v = 0; v < CK; ++v) {
        fetch[v] = n + v < N;
        valid[v] = cell_lane && fetch[v];
        cst[v] = held[v] = 0.f;
        len[v] = 0;
        if constexpr (VL) len[v] = !valid[v] ? 0 : lengths ? lengths[n + v] : T;
    }

    for (int i = tid; i < H * C; i += NT) hs[0][i] = 0.f;
    if (tid == 0) give_up = 0;

    const size_t H4 = 4 * (size_t)H;
    // Running pointers, each advanced by one recurrence step at the top of every step, in front of the poll, so that
    // behind the barrier stand the loads and stores alone.  With t(s) the time index of step s, in step s they stand at
    // t(s + 1) (gxp: the prefetch) and at t(s - 1) (rp, yp: the outputs held back); one is read only where that is a
    // time index of the tensor (s + 1 < T; s > 0).
    const ptrdiff_t dir = reverse ? -1 : 1, t0 = reverse ? T - 1 : 0;
    // the chunks of the staging block this lane stores: rows (value, column) of y, cell and the gates' four slabs
    gfloat *rp[NQ];
    ptrdiff_t rstep[NQ];
    bool rok[NQ];                                      // a chunk of the block and of a column of the batch
    if constexpr (SAVE) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = tid + i * NT, row = q / U4, v = row / C, nn = n0 + row % C;
            const size_t w = v < 2 ? (size_t)H : H4;
            float *base = v == 0 ? y : v == 1 ? cell : gates + (size_t)(v - 2) * H;
            rstep[i] = dir * (ptrdiff_t)((size_t)LD * w);
            rok[i] = q < 6 * C * U4 && nn < N;
            rp[i] = (gfloat *)base + (size_t)nn * w + j0 + 4 * (q % U4) + (t0 - 2 * dir) * (ptrdiff_t)((size_t)LD * w);
        }
    }
    const float4 *stg4 = reinterpret_cast<const float4 *>(&stg[0][0]);       // the two blocks as 16-byte chunks
    // not SAVE: y of this lane's columns
    gfloat *yp = (gfloat *)y + ((t0 - 2 * dir) * LD + n) * (ptrdiff_t)H + j0 + u;
    const ptrdiff_t ystep = dir * (ptrdiff_t)LD * H;
    // gx of this lane's gate in its columns, at time 0 (the next column is H4 floats on)
    const float *gx0 = gx + (size_t)n * H4 + (size_t)gate * H + j0 + u;
    const ptrdiff_t gstep = dir * (ptrdiff_t)((size_t)LD * H4);
    gcfloat *gxp = (gcfloat *)gx0 + t0 * (ptrdiff_t)((size_t)LD * H4);
    float gq[CK];                                      // ... of this step (loaded one step ahead)
#pragma unroll
    for (int v = 0; v < CK; ++v) gq[v] = fetch[v] ? gxp[v * H4] : 0.f;
    // the granule this lane publishes, by step parity
    u64 *const pub0 = hbuf + (size_t)group * (H * C) + col * H + j0 + u;
    const size_t pubpitch = (size_t)ngroups * (H * C);
    __syncthreads();

    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        float *hb = hs[s & 1];
        settle(gq);
        gxp += gstep;
        settle_ptr(gxp);
        if constexpr (SAVE) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                rp[i] += rstep[i];
                settle_ptr(rp[i]);
            }
        } else {
            yp += ystep;
            settle_ptr(yp);
        }
        gu64 *pub = (gu64 *)pub0 + (s & 1) * pubpitch;
        settle_ptr(pub);
        int blk[NQ];                                     // SAVE: this lane's chunks of the step before's block (none: chunk 0)
        if constexpr (SAVE) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                blk[i] = rok[i] ? ((s - 1) & 1) * (6 * C * U4) + tid + i * NT : 0;
                asm volatile("" : "+v"(blk[i]));
            }
        }
        if (s > 0) {
            const u64 *src = hbuf + ((size_t)((s - 1) & 1) * ngroups + group) * (H * C);
            float v[NG];
            if (!sweep<NG>(src, tid, NT, H * C, (unsigned)s, v, status)) give_up = 1;
            // granule e = c * H + k.  The 64 lanes of a wave write 64 floats two apart, as the [k][c] image has them: two
            // lanes per bank of a ds_write_b32's group of 32, which costs that write nothing (its cycles are those of
            // moving address and data to the LDS)
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                const int e = tid + q * NT;
                hb[FL.hs_index(e % H, e / H)] = v[q];
            }
            __syncthreads();
            if constexpr (!SAVE) {                       // (from a register: nothing to wait for)
#pragma unroll
                for (int v = 0; v < CK; ++v)
                    if (valid[v]) yp[v * H] = held[v];
            }
        }
        float gn[CK];
#pragma unroll
        for (int v = 0; v < CK; ++v) gn[v] = fetch[v] && s + 1 < T ? gxp[v * H4] : 0.f;
        asm volatile("" ::: "memory");                   // the prefetch stays here

        float acc[4 * C];                                // (gate, c) at FL.flat(gate, c): the order the rounds halve
#pragma unroll
        for (int a = 0; a < 4 * C; ++a) acc[a] = 0.f;
        // read j: rows PR j ... PR j + PR - 1 of this lane, one 16-byte read; AHEAD of them in flight in front of the FMAs
        // that use the first
        constexpr int NR = KS / PR, AHEAD = 4;
        float hv[NR][PR * C];
#pragma unroll
        for (int j = 0; j < AHEAD; ++j) lds_row<PR * C>(hb + FL.chunk(kp, j), hv[j]);
        // Behind them, so that no wait for either stands in front of the first FMA: give_up, read by every wave behind
        // the same barrier and tested once, in front of the cell update (a workgroup that has given up runs the matvec
        // out on an h it does not know, and neither publishes nor stages); and this lane's chunks of the step before's
        // block, which leave behind the first group of FMAs (LDS answers in order: they have come when read 1 has).
        // Both reads stand in step 0 as well, which has no poll: give_up is 0 there, and the chunks are not stored.
        const int gu = give_up;
        float4 out[NQ];
        if constexpr (SAVE) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) out[i] = stg4[blk[i]];
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (j + AHEAD < NR) lds_row<PR * C>(hb + FL.chunk(kp, j + AHEAD), hv[j + AHEAD]);
            __builtin_amdgcn_sched_barrier(0);           // (left alone, the scheduler sinks the read to its first use)
#pragma unroll
            for (int e = 0; e < PR; ++e)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        acc[FL.flat(g, c)] = fmaf(w[g][PR * j + e], hv[j][e * C + c], acc[FL.flat(g, c)]);
            if constexpr (SAVE) {
                if (j == 0) {                            // behind the step's poll, in front of its cell update
#pragma unroll
                    for (int i = 0; i < NQ; ++i) {
                        // (a chunk made to wait for the sums as they stand: left alone, the FMAs above sink below its store)
#pragma unroll
                        for (int a = 0; a < 4 * C; ++a) asm volatile("" : "+v"(out[i].x) : "v"(acc[a]));
                        if (rok[i] && s > 0) *(grow_chunk *)rp[i] = row_chunk{out[i].x, out[i].y, out[i].z, out[i].w};
                    }
                    asm volatile("" ::: "memory");       // the deferred stores stay here
                }
            }
        }
        halve_rounds<1, KP>(acc, kp);                    // acc[v]: `gate` of column col + v, summed over the 8 lanes
        if (gu) return;

        float ig[CK], fg[CK], gg[CK], og[CK];
#pragma unroll
        for (int v = 0; v < CK; ++v) {
            const float x = acc[v] + gq[v];
            float a;
            if (gate == 2)
                a = tanhf(x);
            else
                a = sigmoidf(x);
            ig[v] = a;                                   // (what the cell lane, of gate i, reads)
            gg[v] = xor_lane<2>(a);
            fg[v] = xor_lane<4>(a);
            og[v] = xor_lane<2>(fg[v]);
        }

        if (cell_lane) {
            float h[CK];
#pragma unroll
            for (int v = 0; v < CK; ++v) {
                // (the contraction written out, as in the plain body: the builds must not differ in which product the fma takes)
                cst[v] = fmaf(ig[v], gg[v], fg[v] * cst[v]);
                h[v] = og[v] * tanhf(cst[v]);
                if constexpr (VL) {
                    if (t >= len[v]) {
                        cst[v] = h[v] = 0.f;
                        if constexpr (SAVE) ig[v] = fg[v] = gg[v] = og[v] = 0.f;
                    }
                }
            }
            if (s + 1 < T) {                             // the publish: the step's last operation on global memory
#pragma unroll
                for (int v = 0; v < CK; ++v) store_granule((u64 *)(pub + v * H), (unsigned)(s + 1), h[v]);
            }
#pragma unroll
            for (int v = 0; v < CK; ++v) {
                if constexpr (!SAVE) {
                    held[v] = h[v];
                } else {
                    float *sp = stg[s & 1] + (col + v) * U + u;
                    sp[0 * C * U] = h[v];
                    sp[1 * C * U] = cst[v];
                    sp[2 * C * U] = ig[v];
                    sp[3 * C * U] = fg[v];
                    sp[4 * C * U] = gg[v];
                    sp[5 * C * U] = og[v];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < CK; ++v) gq[v] = gn[v];
    }
    if (T > 0) {                                         // the last step's outputs: one step on from where the pointers stand
        if constexpr (!SAVE) {
#pragma unroll
            for (int v = 0; v < CK; ++v)
                if (valid[v]) yp[ystep + v * H] = held[v];
        } else {
            __syncthreads();                             // the last step's block: no poll, so no barrier, is behind it
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                if (!rok[i]) continue;
                const float4 o = stg4[((T - 1) & 1) * (6 * C * U4) + tid + i * NT];
                *(grow_chunk *)(rp[i] + rstep[i]) = row_chunk{o.x, o.y, o.z, o.w};
            }
        }
    }
}

// Forward.  gx (T, N, 4H) = x W_ih^T + b_ih + b_hh.  Writes y = h (T, N, H), the gate activations (T, N, 4H) and
// c (T, N, H).  Recurrence step s runs time t = s (reverse: T - 1 - s).  hbuf: [2][ngroups][C][H] granules.
//
// Lane (u, kp), kp < KP = threads / U: the 4 gate rows of unit u over the columns k = i KP + kp (i < KS = H / KP)
// in VGPRs, so each h value read from LDS feeds 4 rows (KS C-wide LDS reads per lane per step).  The KP partial
// sums are combined by xor shuffles: the first log2(C) rounds halve the columns a lane keeps, the rest add the 4
// gates of its one column; lane kp < C then holds the 4 pre-activations of column col(kp) and runs its cell update.
// It leaves h, c and the activations in the staging block of the step's parity; behind the next step's barrier (after
// the loop: one barrier of its own) lane tid stores the 16-byte chunks tid + i NT of that block.  No second barrier
// per step: a block is written again two steps on, behind the barrier that every wave reaches after its stores.
// ((256, 64, 2) runs lstm_fwd_lanes_body above: the same lanes, weights and sums, another h image, reduction and split
// of the activations, and the deferred stores and give_up's test further down the step.)
//
// VL: column n has lengths[n] steps (NULL: T).  A step at t >= lengths[n] leaves h = c = 0, writes y = 0 and
// publishes h = 0 like any other step: every workgroup runs all T steps, so the hand-off is that of a full batch.
// SAVE: gates and cell are written, through the staging block (with VL: 0 on a step at or beyond the length).  Not SAVE:
// they are not written (the pointers are not read); y goes out from the cell lane's register, one step late.
template <int H, int C, int U, bool VL = false, bool SAVE = !VL>
__global__ __launch_bounds__((fwd_threads_for<H, U>()), 1) void lstm_fwd_kernel(const float *__restrict__ gx,
                                                                       const float *__restrict__ whh, int T, Cols cols,
                                                                       int reverse, int ngroups,
                                                                       float *__restrict__ y,
                                                                       float *__restrict__ gates,
                                                                       float *__restrict__ cell, u64 *hbuf,
                                                                       uint32_t *status,
                                                                       const int32_t *__restrict__ lengths) {
    if constexpr (lstm_fwd_lanes(H, U, C)) {           // (256, 64, 2): one activation per lane (above); nothing below runs
        lstm_fwd_lanes_body<H, C, U, VL, SAVE>(gx, whh, T, cols, reverse, ngroups, y, gates, cell, hbuf, status, lengths);
        return;
    }
    constexpr int NT = fwd_threads_for<H, U>();
    const int N = cols.n, LD = cols.ld();               // the launch's columns; the tensors' columns per time step
    constexpr int G = H / U;
    constexpr int KP = NT / U;
    constexpr int KS = H / KP;
    constexpr int NG = (H * C + NT - 1) / NT;
    static_assert(KS >= 1 && KP <= 64 && C <= KP, "lane (u, kp) inside one wave; one cell lane per (u, column)");
    constexpr int U4 = U / 4;
    constexpr int NQ = SAVE ? (6 * C * U4 + NT - 1) / NT : 1;        // 16-byte chunks of a staging block per lane
    static_assert(U % 4 == 0, "a row of the staging block is whole 16-byte chunks");
    __shared__ __attribute__((aligned(16))) float hs[2][H * C];      // h_{t-1} as [k][c], by step parity
    // a step's h, c, i, f, g, o as [value][column][unit], by step parity: written by the cell lanes at the end of step
    // s, read behind step s + 1's barrier, written again behind step s + 2's
    __shared__ __attribute__((aligned(16))) float stg[SAVE ? 2 : 1][SAVE ? 6 * C * U : 4];
    __shared__ int give_up;

    int group, member;
    place(G, group, member);
    const int tid = threadIdx.x;
    const int j0 = member * U, n0 = group * C;
    const int u = tid / KP, kp = tid % KP;

    float w[4][KS];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < KS; ++i) w[g][i] = whh[((size_t)g * H + j0 + u) * H + i * KP + kp];
    settle(w);

    int col = 0;                                       // the column this lane keeps through the reduction
#pragma unroll
    for (int m = 1, width = C; width > 1; m <<= 1, width >>= 1)
        if (kp & m) col += width / 2;
    const bool cell_lane = kp < C;
    const int n = n0 + col;
    const bool valid = cell_lane && n < N;
    float cst = 0.f;
    int len = 0;                                       // VL: the steps of this lane's column
    if constexpr (VL) len = !valid ? 0 : lengths ? lengths[n] : T;

    for (int i = tid; i < H * C; i += NT) hs[0][i] = 0.f;
    if (tid == 0) give_up = 0;

    const size_t H4 = 4 * (size_t)H;
    // the chunks of the staging block this lane stores: rows (value, column) of y, cell and the gates' four slabs
    float *rp[NQ];
    size_t rpitch[NQ];
    if constexpr (SAVE) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = tid + i * NT, row = q / U4, v = row / C, nn = n0 + row % C;
            const size_t w = v < 2 ? (size_t)H : H4;
            float *base = v == 0 ? y : v == 1 ? cell : gates + (size_t)(v - 2) * H;
            rpitch[i] = (size_t)LD * w;
            rp[i] = q < 6 * C * U4 && nn < N ? base + (size_t)nn * w + j0 + 4 * (q % U4) : nullptr;
        }
    }
    float gq[4] = {0.f, 0.f, 0.f, 0.f};              // gx of this step (loaded one step ahead)
    if (valid) {
        const float *p = gx + ((size_t)(reverse ? T - 1 : 0) * LD + n) * H4 + j0 + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) gq[g] = p[(size_t)g * H];
    }
    float held = 0.f;                                  // not SAVE: h of the previous step, stored one step late
    __syncthreads();

    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        float *hb = hs[s & 1];
        settle(gq);
        if (s > 0) {
            const u64 *src = hbuf + ((size_t)((s - 1) & 1) * ngroups + group) * (H * C);
            float v[NG];
            if (!sweep<NG>(src, tid, NT, H * C, (unsigned)s, v, status)) give_up = 1;
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                const int e = tid + q * NT;              // granule e = c * H + k
                if (e < H * C) hb[(e % H) * C + e / H] = v[q];
            }
            __syncthreads();
            if (give_up) return;
            const int tl = reverse ? t + 1 : t - 1;
            if constexpr (!SAVE) {
                if (valid) y[((size_t)tl * LD + n) * H + j0 + u] = held;
            } else {
                rows_to_global<NQ>(stg[(s - 1) & 1], tid, NT, rp, rpitch, (size_t)tl);
            }
        }
        float gn[4] = {0.f, 0.f, 0.f, 0.f};
        if (valid && s + 1 < T) {
            const float *p = gx + ((size_t)(reverse ? t - 1 : t + 1) * LD + n) * H4 + j0 + u;
#pragma unroll
            for (int g = 0; g < 4; ++g) gn[g] = p[(size_t)g * H];
        }
        asm volatile("" ::: "memory");                   // the deferred stores and the prefetch stay here

        float acc[4][C];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[g][c] = 0.f;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            float hv[C];
            lds_row<C>(hb + (i * KP + kp) * C, hv);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[g][c] = fmaf(w[g][i], hv[c], acc[g][c]);
        }
#pragma unroll
        for (int m = 1; m < KP; m <<= 1) {
            const int half = C / (2 * m);                // 0 once a lane keeps one column
            const bool up = (kp & m) != 0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (half == 0) acc[g][0] += __shfl_xor(acc[g][0], m);
#pragma unroll
                for (int c = 0; c < C / 2; ++c) {        // (constant trip count: unrolled before the rounds are)
                    if (c < half) {
                        const float send = up ? acc[g][c] : acc[g][c + half];
                        const float keep = up ? acc[g][c + half] : acc[g][c];
                        acc[g][c] = keep + __shfl_xor(send, m);
                    }
                }
            }
        }

        if (cell_lane) {
            float ig = sigmoidf(acc[0][0] + gq[0]), fg = sigmoidf(acc[1][0] + gq[1]);
            float gg = tanhf(acc[2][0] + gq[2]), og = sigmoidf(acc[3][0] + gq[3]);
            // (the contraction written out: left to the compiler, which product the fma takes depends on the code around
            // it -- the VL mask's select, the staging stores -- and a column's rows then differ in the last bit between
            // the builds)
            cst = fmaf(ig, gg, fg * cst);
            float h = og * tanhf(cst);
            if constexpr (VL) {
                if (t >= len) {
                    cst = h = 0.f;
                    if constexpr (SAVE) ig = fg = gg = og = 0.f;
                }
            }
            if (s + 1 < T)
                store_granule(hbuf + ((size_t)(s & 1) * ngroups + group) * (H * C) + col * H + j0 + u,
                              (unsigned)(s + 1), h);
            if constexpr (!SAVE) {
                held = h;
            } else {
                float *sp = stg[s & 1] + col * U + u;
                sp[0 * C * U] = h;
                sp[1 * C * U] = cst;
                sp[2 * C * U] = ig;
                sp[3 * C * U] = fg;
                sp[4 * C * U] = gg;
                sp[5 * C * U] = og;
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) gq[g] = gn[g];
    }
    if (T > 0) {
        const int tl = reverse ? 0 : T - 1;
        if constexpr (!SAVE) {
            if (valid) y[((size_t)tl * LD + n) * H + j0 + u] = held;
        } else {
            __syncthreads();                             // the last step's block: no poll, so no barrier, is behind it
            rows_to_global<NQ>(stg[(T - 1) & 1], tid, NT, rp, rpitch, (size_t)tl);
        }
    }
}

#ifndef TK_RNN_VARLEN
// Backward.  From the saved gate activations and c, and dy = dL/dy (T, N, H), writes dgates = dL/d(pre-activation)
// (T, N, 4H) walking the recurrence from its last step.  pbuf: [2][ngroups][G producers][C][H] granules.
//
// VL: column n has lengths[n] steps (NULL: T).  A step at t >= lengths[n] writes dgates = 0 and hands on dh = 0 and
// dc = 0 (its dG rows in LDS are 0, so is what it publishes; dc_next = f_next = 0), like any other step.  The mask is a
// select behind the cell update, as in the forward: dy, the gates and c beyond the length are loaded and never used.
// (With reverse != 0 the walk reaches the padding after the column's real steps, with a dh and a dc f that are not 0.)
//
// Lane (k, rp), rp < RP = threads / H, holds column k of R = 4 U / RP owned rows of W_hh: rows rp R + i (i < R); at
// U = 48 rows i RP + rp, as the GRU backward takes them.  RP divides U, so row i RP + rp is unit (i RP) % U + rp of gate
// (i RP) / U, a compile-time offset from the lane's first weight: with U and H no powers of two, r / U and r % U of a
// run-time row keep an address per weight live, and the kernel spills.
//
// Block layout (H 256, U 64: lstm_bwd_layout.h has the arithmetic and the order of summation).  In the column layout
// every lane of a wave reads the same dG row, and a value read from LDS feeds one weight: at C 2 a wave issues 64
// ds_read_b128 for its 256 v_fmac per step, 64 x 4 LDS-array cycles x 8 waves = 2048 per step and CU against
// 2 x 256 x 2 = 1024 VALU cycles per SIMD -- the matvec waits for the LDS array (measured: 2192 LDS-array cycles per
// step and CU, SQ_LDS_IDX_ACTIVE, profiles/r35_lstm_bwd_layout.txt).  Here lane (kb, rq) = (tid / 8, tid % 8) holds
// the 4 columns k = 4 kb + q of 32 rows, the row pairs p = rq + 8 i: a pair is one read of 2 C floats, the 8 lanes rq
// read 8 adjacent chunks (the other lanes of the wave the same 8: no conflict), and each value feeds 4 weights: 16
// ds_read_b128 per wave and step at C 2, 592 LDS-array cycles per step and CU measured.  The 8 partial sums of a
// (k, c) meet inside the wave by recursive halving over xor 1, 2, 4 (DPP operands of the adds, no LDS), after which a
// lane holds C H / threads sums of distinct (k, c) and publishes exactly those: no `red`, no third barrier, no strided
// publish loop.  The order of a sum depends on (H, U) alone, so a column's dgates are the same bits at C 2 and C 4;
// for that the gather of these instantiations also adds the G producers one by one in producer order at either C
// (APART below: at C 4 the column layout's two planes each added two producers first).
template <int H, int C, int U, bool VL = false>
__global__ __launch_bounds__((bwd_threads_for<H, U>()), 1) void lstm_bwd_kernel(const float *__restrict__ whh,
                                                                       const float *__restrict__ gates,
                                                                       const float *__restrict__ cell,
                                                                       const float *__restrict__ dy, int T, Cols cols,
                                                                       int reverse, int ngroups,
                                                                       float *__restrict__ dgates, u64 *pbuf,
                                                                       uint32_t *status,
                                                                       const int32_t *__restrict__ lengths) {
    constexpr int NT = bwd_threads_for<H, U>();
    const int N = cols.n, LD = cols.ld();               // the launch's columns; the tensors' columns per time step
    constexpr int G = H / U;
    constexpr bool STRIDED = U == 48;                 // a lane's rows: every RP-th, not R in a run
    constexpr int RP = NT / H;                        // row partitions: lane (k, rp) holds W_hh[rows of rp, k]
    constexpr int R = 4 * U / RP;                     // floats per lane
    constexpr LstmBwdBlock LB(NT, H, U, C);           // the block layout (lstm_bwd_layout.h) ...
    constexpr bool BLOCK = LB.KQ > 0;                 // ... where the instantiation takes it
    constexpr int KQ = BLOCK ? LB.KQ : 1, RQ = BLOCK ? LB.RQ : 1, RR = BLOCK ? LB.RR : 1, KEEP = BLOCK ? LB.KEEP : 1;
    constexpr int PAIRS = U * C;                      // (c, u) pairs of the cell update
    constexpr int PL = NT / PAIRS;                    // producer planes of the gather
    constexpr int NP = (G + PL - 1) / PL;
    // BLOCK: a plane that polls NP > 1 producers leaves them apart in `gath`, and the cell lane adds all G in producer
    // order, as the launch with one producer per plane does: a column's dh is the same bits whatever C
    constexpr bool APART = BLOCK && NP > 1;
    static_assert(!APART || NP * PL == G, "every plane polls NP producers");
    static_assert(RP >= 1 && R >= 1 && PL >= 1 && PL * PAIRS == NT, "every lane polls; one cell lane per pair");
    static_assert(!STRIDED || (RP * H == NT && R * RP == 4 * U && U % RP == 0),
                  "a lane's rows keep their gate index at compile time");
    static_assert(!BLOCK || (LB.ok() && KQ * RR * NT == 4 * U * H && RQ <= 64 && (RQ & (RQ - 1)) == 0 &&
                             KEEP * NT == C * H && KQ * RR == R),
                  "every owned weight in one lane; the RQ partial sums inside one wave; one granule per held sum");
    __shared__ __attribute__((aligned(16))) float dgs[4 * U * C];      // dG_t of the owned rows as [row][c]
    __shared__ float gath[(APART ? G : PL) * PAIRS];
    __shared__ __attribute__((aligned(16))) float red[RP > 1 && !BLOCK ? RP * C * H : 1];
    __shared__ int give_up;

    int group, member;
    place(G, group, member);
    const int tid = threadIdx.x;
    const int j0 = member * U, n0 = group * C;

    const int k = tid % H, rp = tid / H;
    const int kb = tid / RQ, rq = tid % RQ;            // BLOCK: lane (kb, rq)
    float w[R];                                        // BLOCK: as [q][j], the weight of column KQ kb + q in row(rq, j)
    if constexpr (BLOCK) {
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            const int r = LB.row(rq, j);
#pragma unroll
            for (int q = 0; q < KQ; ++q) w[q * RR + j] = whh[((size_t)(r / U) * H + j0 + (r % U)) * H + KQ * kb + q];
        }
    } else if constexpr (STRIDED) {
        const float *wbase = whh + (size_t)(j0 + rp) * H + k;
#pragma unroll
        for (int i = 0; i < R; ++i) w[i] = wbase[(unsigned)((((i * RP) / U) * H + (i * RP) % U) * H)];
    } else {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int r = rp * R + i;
            w[i] = whh[((size_t)(r / U) * H + j0 + (r % U)) * H + k];
        }
    }
    settle(w);
    // PACKED (BLOCK at C 2): the matvec as packed FMAs over the two columns (pk_fma_lo above).  wq[q RR / 2 + i] =
    // {w[q RR + 2 i], w[q RR + 2 i + 1]}, column KQ kb + q of the row pair i, one register pair for the whole launch; w is
    // not read behind this
    constexpr bool PACKED = BLOCK && C == 2;
    pair2 wq[PACKED ? R / 2 : 1];
    if constexpr (PACKED) {
#pragma unroll
        for (int m = 0; m < R / 2; ++m) wq[m] = pair2{w[2 * m], w[2 * m + 1]};
        settle_pairs(wq);
    }

    const bool cell_lane = tid < PAIRS;
    const int pair = tid % PAIRS, plane = tid / PAIRS;
    const int cc = pair / U, u = pair % U;
    const int n = n0 + cc;
    const bool valid = cell_lane && n < N;
    float dc_next = 0.f, f_next = 0.f;
    int len = 0;                                       // VL: the steps of this lane's column
    if constexpr (VL) len = !valid ? 0 : lengths ? lengths[n] : T;
    if (tid == 0) give_up = 0;

    // this step's inputs, loaded one step ahead: dy, c_t, c_{t-1}, the four gates (c_t of a step is the c_{t-1}
    // of the step before)
    const size_t H4 = 4 * (size_t)H;
    float in[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const int t = reverse ? 0 : T - 1;
        const size_t o = ((size_t)t * LD + n) * H + j0 + u;
        in[0] = dy[o];
        in[1] = cell[o];
        if (T > 1) in[2] = cell[((size_t)(reverse ? t + 1 : t - 1) * LD + n) * H + j0 + u];
        const float *gp = gates + ((size_t)t * LD + n) * H4 + j0 + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) in[3 + g] = gp[(size_t)g * H];
    }
    float held[4] = {0.f, 0.f, 0.f, 0.f};             // dG of the previous step, stored one step late
    // Running pointers, each advanced by one recurrence step at the top of every step, in front of the poll, so that
    // behind the gather's barrier stand the loads and stores alone.  With t(s) the time index of step s, in step s they
    // stand at: dyp, gp: dy and the gates of t(s + 1); cnp: c of t(s + 2); dgp: dgates of t(s - 1).  A pointer is read
    // only where its time index is one of the tensor's (valid lanes; the guards on tt below; s > 0).
    const ptrdiff_t step1 = (reverse ? 1 : -1) * (ptrdiff_t)LD * H, step4 = 4 * step1;
    const ptrdiff_t row0 = ((ptrdiff_t)(reverse ? 0 : T - 1) * LD + n) * H;      // row (t(0), n) of a (T, N, H) tensor
    gcfloat *dyp = (gcfloat *)dy + row0 + j0 + u, *cnp = (gcfloat *)cell + row0 + step1 + j0 + u;
    gcfloat *gp = (gcfloat *)gates + 4 * row0 + j0 + u;
    gfloat *dgp = (gfloat *)dgates + 4 * row0 - 2 * step4 + j0 + u;
    __syncthreads();

    const u64 *mine = pbuf + (size_t)group * G * C * H + cc * H + j0 + u;
    // BLOCK: the first of the KEEP sums this lane publishes is granule (c, k) = (a0 % C, KQ kb + a0 / C); the others are
    // the columns c + 1, ... of the same k
    const int a0 = LB.kept_first(rq), pub = (a0 % C) * H + KQ * kb + a0 / C;
    for (int s = 0; s < T; ++s) {
        const int tt = T - 1 - s;                         // recurrence position
        const int t = reverse ? T - 1 - tt : tt;          // time index
        const int tp = reverse ? t + 1 : t - 1;           // time index of the recurrence's previous step
        settle(in);
        // What the cell update takes from in[] alone, computed here, where the wave would otherwise only wait for the
        // poll: tanh(c_t) and the factors of the gate derivatives, each the operation the update always was (fac[0] one
        // fma; fac[3] a product, then a difference).  Pinned in front of the poll like the loads.
        float fac[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (cell_lane) {
#pragma clang fp contract(off)
            const float tc = tanhf(in[1]);
            fac[0] = fmaf(-tc, tc, 1.f);
            fac[1] = 1.f - in[3];
            fac[2] = 1.f - in[4];
            const float g2 = in[5] * in[5];
            fac[3] = 1.f - g2;
            fac[4] = 1.f - in[6];
            fac[5] = tc;
        }
        settle(fac);
        dyp += step1;
        cnp += step1;
        gp += step4;
        dgp += step4;
        settle_ptr(dyp);
        settle_ptr(cnp);
        settle_ptr(gp);
        settle_ptr(dgp);
        float dhr = 0.f;
        int gu = 0;                                       // give_up as read behind the gather's barrier
        if (s > 0) {
            float v[NP];
            const int nvalid = plane < G ? (G - plane + PL - 1) / PL : 0;
            const u64 *src = mine + (size_t)((s - 1) & 1) * ngroups * G * C * H;
            if (!sweep<NP>(src, plane * C * H, PL * C * H, G * C * H, (unsigned)s, v, status)) give_up = 1;
            if constexpr (APART) {
#pragma unroll
                for (int q = 0; q < NP; ++q) gath[(plane + q * PL) * PAIRS + pair] = v[q];
            } else {
                float sum = 0.f;
#pragma unroll
                for (int q = 0; q < NP; ++q)
                    if (q < nvalid) sum += v[q];
                gath[plane * PAIRS + pair] = sum;
            }
            __syncthreads();
            // read here, by every wave behind the same barrier, and tested once, behind the dgs barrier: no wait for it
            // stands on the chain, and a workgroup that has given up runs the step out (on a dh it does not know, into
            // registers and LDS only: the stores below are the step before's) but does not publish
            gu = give_up;
            if (cell_lane) {
#pragma unroll
                for (int p = 0; p < (APART ? G : PL); ++p) dhr += gath[p * PAIRS + pair];
            }
            if (valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g) dgp[(size_t)g * H] = held[g];
            }
        }
        float nx[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (valid && tt > 0) {
            nx[0] = *dyp;
            nx[1] = in[2];
            if (tt > 1) nx[2] = *cnp;
#pragma unroll
            for (int g = 0; g < 4; ++g) nx[3 + g] = gp[(size_t)g * H];
        }
        asm volatile("" ::: "memory");                   // the deferred stores and the prefetch stay here

        if (cell_lane) {
#pragma clang fp contract(off)
            float cp = in[2];
            if constexpr (VL) {
                if (tp >= len) cp = 0.f;                  // (reverse: the column's first step starts from c = 0)
            }
            const float ig = in[3], gg = in[5], og = in[6];
            float fg = in[4];
            const float dh = in[0] + dhr;
            const float tc = fac[5];
            // (the one contraction written out: dc_next f_next is the product the fma takes, as it always was)
            float dc = fmaf(dc_next, f_next, dh * og * fac[0]);
            float di = dc * gg * ig * fac[1];
            float df = dc * cp * fg * fac[2];
            float dg = dc * ig * fac[3];
            float dout = dh * tc * og * fac[4];
            if constexpr (VL) {
                if (t >= len) dc = fg = di = df = dg = dout = 0.f;
            }
            dc_next = dc;
            f_next = fg;
            held[0] = di;
            held[1] = df;
            held[2] = dg;
            held[3] = dout;
            dgs[(0 * U + u) * C + cc] = valid ? di : 0.f;
            dgs[(1 * U + u) * C + cc] = valid ? df : 0.f;
            dgs[(2 * U + u) * C + cc] = valid ? dg : 0.f;
            dgs[(3 * U + u) * C + cc] = valid ? dout : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) in[q] = nx[q];
        // every wave holds the same gu; in front of the barrier the waves without cell lanes test it while they would
        // wait for the others (and in front of the last step's stores: the dG of a step that gave up is not one)
        if (gu) return;
        __syncthreads();
        if (s + 1 == T) break;                           // the first step has no predecessor to feed

        if constexpr (BLOCK) {
            u64 *dst = pbuf + (((size_t)(s & 1) * ngroups + group) * G + member) * C * H;
            float acc[KQ * C];
#pragma unroll
            for (int a = 0; a < KQ * C; ++a) acc[a] = 0.f;
            pair2 accp[KQ];                               // PACKED: one per column k of the lane, the halves the two batch columns
#pragma unroll
            for (int q = 0; q < KQ; ++q) accp[q] = pair2{0.f, 0.f};
#pragma unroll
            for (int i = 0; i < RR / 2; ++i) {
                float d[2 * C];                           // rows 2 p and 2 p + 1 of the pair p = rq + RQ i
                lds_row<2 * C>(dgs + (rq + RQ * i) * 2 * C, d);
                if constexpr (PACKED) {
                    const pair2 d0 = {d[0], d[1]}, d1 = {d[2], d[3]};        // the read's two aligned halves: a row each
#pragma unroll
                    for (int q = 0; q < KQ; ++q) pk_fma_lo(accp[q], wq[q * RR / 2 + i], d0);
#pragma unroll
                    for (int q = 0; q < KQ; ++q) pk_fma_hi(accp[q], wq[q * RR / 2 + i], d1);
                } else {
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int q = 0; q < KQ; ++q)
#pragma unroll
                            for (int c = 0; c < C; ++c)
                                acc[q * C + c] = fmaf(w[q * RR + 2 * i + e], d[e * C + c], acc[q * C + c]);
                }
            }
            if constexpr (PACKED) {
#pragma unroll
                for (int q = 0; q < KQ; ++q)
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[q * C + c] = accp[q][c];
            }
            halve_rounds<1, RQ>(acc, rq);
#pragma unroll
            for (int v = 0; v < KEEP; ++v) store_granule(dst + pub + v * H, (unsigned)(s + 1), acc[v]);
            continue;
        }
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            float d[C];
            lds_row<C>(dgs + (STRIDED ? i * RP + rp : rp * R + i) * C, d);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = fmaf(w[i], d[c], acc[c]);
        }
        u64 *dst = pbuf + (((size_t)(s & 1) * ngroups + group) * G + member) * C * H;
        if constexpr (RP == 1) {
#pragma unroll
            for (int c = 0; c < C; ++c) store_granule(dst + c * H + k, (unsigned)(s + 1), acc[c]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) red[(rp * C + c) * H + k] = acc[c];
            __syncthreads();
            for (int e = tid; e < C * H; e += NT) {
                float v = 0.f;
#pragma unroll
                for (int q = 0; q < RP; ++q) v += red[q * C * H + e];
                store_granule(dst + e, (unsigned)(s + 1), v);
            }
        }
    }
    if (valid && T > 0) {
        const int tl = reverse ? T - 1 : 0;
        float *dp = dgates + ((size_t)tl * LD + n) * H4 + j0 + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) dp[(size_t)g * H] = held[g];
    }
}

#endif  // TK_RNN_VARLEN: no backward

int g_lab_cols = 0;     // lab build: force the admitted batch columns, 8 or 16; H = 192: 4 or 8 (0 = the rule below)
int g_lab_units = 0;    // lab build: force the hidden units per workgroup, 16, 32 or 64 (0 = the rule in lstm_plan)

// units per workgroup of the sizes that are no power of two (0: a power of two, planned from U = 16)
int units48(size_t H) { return H == 192 || H == 384 ? 48 : 0; }

// The admission geometry: batch columns C per group and the number of groups; false where the kernels do not run.  It
// fixes the workspace (tk_lstm_workspace_bytes) and bounds every launch plan.  H = 16 ... 256, powers of two: groups of
// H / 16 workgroups with 8 columns where they fit one workgroup per CU, else with 16.  H = 192 and 384: groups of H / 48
// workgroups with 4 columns where they fit, else, at H = 192 only, with 8 (at H = 384 the forward at 8 columns does not
// fit its registers); this is the launch itself.  Every kernel waits on the other members of its group, so a grid
// larger than the CU count is never admitted.
#ifdef TK_LSTM_LARGE
// -DTK_LSTM_LARGE (libtaiyaki_amd_lstm_large.so): H = 512 alone.  Groups of 512 / 32 = 16 workgroups with 4 columns
// where they fit one workgroup per CU, else with 8; this is the launch itself, as at H = 192 and 384.
constexpr int kLargeUnits = 32;

bool lstm_geometry(size_t N, size_t H, int cu_count, int *C_out, int *groups_out) {
    if (H != 512 || N == 0 || cu_count <= 0) return false;
    const size_t G = H / kLargeUnits;
    for (int C = 4; C <= 8; C *= 2) {
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
#else
bool lstm_geometry(size_t N, size_t H, int cu_count, int *C_out, int *groups_out) {
    const int U48 = units48(H);
    if (!(U48 || H == 16 || H == 32 || H == 64 || H == 128 || H == 256) || N == 0 || cu_count <= 0) return false;
    const size_t G = H / (U48 ? U48 : 16);
    const int first = U48 ? 4 : 8, last = H == 384 ? 4 : 2 * first;
    for (int C = first; C <= last; C *= 2) {
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
#endif  // TK_LSTM_LARGE

size_t ws_bytes(size_t H, int C, int groups, int U, bool backward) {
    return 2 * (size_t)groups * (backward ? H / U : 1) * C * H * sizeof(u64);
}

// A launch: U units and C = C_admitted * 16 / U columns per workgroup, groups of H / U workgroups.  Release rule:
// U = 64, or H where H < 64 (config 2's layer when the rule was set: 2.85 / 2.54 us per forward / backward step at U = 64, 2.84 / 3.58 at
// U = 32, 3.44 / 4.02 at U = 16; tools/lstmbench.py).  C divides the admitted column count, so the grid and both granule buffers are never
// larger than those of the admission geometry.  H = 192 and 384: U = 48 and the admitted columns and groups as they are
// (the lab's forced units do not apply).
struct Plan {
    int U, C, groups;
    unsigned grid;
};

bool lstm_plan(size_t N, size_t H, int cu_count, Plan *p) {
    int C16 = 0, groups16 = 0;
    if (!lstm_geometry(N, H, cu_count, &C16, &groups16)) return false;
#ifdef TK_LSTM_LARGE
    *p = Plan{kLargeUnits, C16, groups16, (unsigned)(groups16 * (H / kLargeUnits))};
    return true;
#endif
    if (const int U48 = units48(H)) {
        *p = Plan{U48, C16, groups16, (unsigned)(groups16 * (H / U48))};
        return true;
    }
    int U = g_lab_units != 0 ? g_lab_units : 64;
    if ((size_t)U > H) U = (int)H;
    if (U != 16 && U != 32 && U != 64) return false;
    p->U = U;
    p->C = C16 * 16 / U;
    p->groups = (int)((N + p->C - 1) / p->C);
    p->grid = (unsigned)(p->groups * (H / U));
    return true;
}

// (H, U, C) -> one instantiation: U = 16 takes 8 or 16 columns, U = 32 4 or 8, U = 64 2 or 4; U <= H; U = 48 takes 4,
// and 8 at H = 192.  -DTK_LSTM_LARGE: (512, 32, 4) and (512, 32, 8) and no other
#ifdef TK_LSTM_LARGE
#define TK_LSTM_SWITCH(LAUNCH)                                                                                    \
    switch ((int)H * 100000 + p.U * 1000 + p.C) {                                                                 \
        LAUNCH(512, 32, 4) LAUNCH(512, 32, 8)                                                                     \
        default: return TK_ERR_UNSUPPORTED;                                                                       \
    }
#else
#define TK_LSTM_SWITCH(LAUNCH)                                                                                   \
    switch ((int)H * 100000 + p.U * 1000 + p.C) {                                                                 \
        LAUNCH(16, 16, 8) LAUNCH(16, 16, 16) LAUNCH(32, 16, 8) LAUNCH(32, 16, 16) LAUNCH(64, 16, 8)                \
        LAUNCH(64, 16, 16) LAUNCH(128, 16, 8) LAUNCH(128, 16, 16) LAUNCH(256, 16, 8) LAUNCH(256, 16, 16)          \
        LAUNCH(32, 32, 4) LAUNCH(32, 32, 8) LAUNCH(64, 32, 4) LAUNCH(64, 32, 8) LAUNCH(128, 32, 4)                 \
        LAUNCH(128, 32, 8) LAUNCH(256, 32, 4) LAUNCH(256, 32, 8)                                                  \
        LAUNCH(64, 64, 2) LAUNCH(64, 64, 4) LAUNCH(128, 64, 2) LAUNCH(128, 64, 4) LAUNCH(256, 64, 2)               \
        LAUNCH(256, 64, 4) LAUNCH(192, 48, 4) LAUNCH(192, 48, 8) LAUNCH(384, 48, 4)                               \
        default: return TK_ERR_UNSUPPORTED;                                                                       \
    }
#endif

template <bool VL, bool SAVE>
int launch_fwd(const Plan &p, size_t H, hipStream_t st, const float *gx, const float *whh, int T, Cols cols,
               int rev, float *y, float *gates, float *cell, u64 *ws, uint32_t *status, const int32_t *lengths) {
#define TK_LSTM_FWD(HH, UU, CC)                                                                                  \
    case HH * 100000 + UU * 1000 + CC:                                                                           \
        hipLaunchKernelGGL((lstm_fwd_kernel<HH, CC, UU, VL, SAVE>), dim3(p.grid), dim3(fwd_threads_for<HH, UU>()), 0,  \
                           st, gx, whh, T, cols, rev, p.groups, y, gates, cell, ws, status, lengths);            \
        break;
    TK_LSTM_SWITCH(TK_LSTM_FWD)
#undef TK_LSTM_FWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

#ifndef TK_RNN_VARLEN
template <bool VL>
int launch_bwd(const Plan &p, size_t H, hipStream_t st, const float *whh, const float *gates, const float *cell,
               const float *dy, int T, Cols cols, int rev, float *dg, u64 *ws, uint32_t *status,
               const int32_t *lengths) {
#define TK_LSTM_BWD(HH, UU, CC)                                                                                   \
    case HH * 100000 + UU * 1000 + CC:                                                                            \
        hipLaunchKernelGGL((lstm_bwd_kernel<HH, CC, UU, VL>), dim3(p.grid), dim3(bwd_threads_for<HH, UU>()), 0,   \
                           st, whh, gates, cell, dy, T, cols, rev, p.groups, dg, ws, status, lengths);            \
        break;
    TK_LSTM_SWITCH(TK_LSTM_BWD)
#undef TK_LSTM_BWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}
#endif  // TK_RNN_VARLEN
#undef TK_LSTM_SWITCH

// The slab width of a batch of N columns (rnn_common.h has the rule): the widest batch lstm_geometry admits at
// (H, cu_count), or N where one launch admits the batch; 0 where the kernels do not run.
size_t lstm_slab(size_t N, size_t H, int cu_count) {
    int C = 0, groups = 0;
    const size_t S = widest_admitted([&](size_t n) { return lstm_geometry(n, H, cu_count, &C, &groups); });
    return N == 0 ? 0 : N < S ? N : S;
}

// What every dispatcher below does around its launch, written once: the pointer and range checks (`pointers_ok`: the
// entry's own required pointers), then for every slab of the batch its plan, the workspace's size, nothing to do at
// T == 0, the granules zeroed, then `launch(plan, the slab's first column, its columns)`.  The -DTK_RNN_WIDE and
// -DTK_LSTM_LARGE builds alone cut a batch: everywhere else the one slab is the batch, and a batch that no launch admits is refused.  The slabs
// share the workspace and follow each other on `stream`: two persistent grids at once could together exceed the CUs
// and wait on each other for ever.  The first slab is the widest, so it has the largest plan: a later slab cannot fail
// a check that the first passed, and a launch error returns at once, with no further slab started.
template <class Launch>
int checked(bool pointers_ok, size_t T, size_t N, size_t H, int cu_count, void *ws, size_t wsb, uint32_t *status,
            hipStream_t stream, bool backward, Launch launch) {
    if (!pointers_ok || !ws || !status || !aligned16(ws) || T > (size_t)INT32_MAX || N > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
#ifdef TK_RNN_SLABS
    const size_t S = lstm_slab(N, H, cu_count);
#else
    const size_t S = N;
#endif
    if (S == 0) return TK_ERR_UNSUPPORTED;
    for (size_t first = 0; first < N; first += S) {
        const size_t n = N - first < S ? N - first : S;
        Plan p;
        if (!lstm_plan(n, H, cu_count, &p)) return TK_ERR_UNSUPPORTED;
        const size_t need = ws_bytes(H, p.C, p.groups, p.U, backward);
        if (wsb < need) return TK_ERR_WORKSPACE;
        if (T == 0) continue;
        int rc = zero_ws(ws, need, stream);
        if (rc != TK_OK) return rc;
        rc = launch(p, first, make_cols(n, N));
        if (rc != TK_OK) return rc;
    }
    return TK_OK;
}

// the backward's granule bytes at U = 16 (H = 192, 384: at the launch's U = 48): they bound every plan's, forward and
// backward
size_t train_workspace_bytes(size_t N, size_t H, int cu_count) {
    int C = 0, groups = 0;
    if (!lstm_geometry(N, H, cu_count, &C, &groups)) return 0;
#ifdef TK_LSTM_LARGE
    return ws_bytes(H, C, groups, kLargeUnits, true);
#endif
    const int U48 = units48(H);
    return ws_bytes(H, C, groups, U48 ? U48 : 16, true);
}

// The forward and the backward of every dispatcher below: `checked`, whose launch of a slab takes the tensors, and
// `lengths`, advanced to the slab's first column.
template <bool VL, bool SAVE>
int forward(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N, size_t H, int reverse,
            int cu_count, float *y, float *gates, float *cell, void *ws, size_t wsb, uint32_t *status,
            hipStream_t stream) {
    auto launch = [&](const Plan &p, size_t first, Cols cols) {
        return launch_fwd<VL, SAVE>(p, H, stream, at_column(gx, first, 4 * H), whh, (int)T, cols, reverse,
                                    at_column(y, first, H), at_column(gates, first, 4 * H), at_column(cell, first, H),
                                    static_cast<u64 *>(ws), status, at_column(lengths, first, 1));
    };
    return checked(gx && whh && y && (!SAVE || (gates && cell)), T, N, H, cu_count, ws, wsb, status, stream, false,
                   launch);
}

#ifndef TK_RNN_VARLEN
template <bool VL>
int backward(const float *whh, const float *gates, const float *cell, const float *dy, const int32_t *lengths,
             size_t T, size_t N, size_t H, int reverse, int cu_count, float *dgates, void *ws, size_t wsb,
             uint32_t *status, hipStream_t stream) {
    auto launch = [&](const Plan &p, size_t first, Cols cols) {
        return launch_bwd<VL>(p, H, stream, whh, at_column(gates, first, 4 * H), at_column(cell, first, H),
                              at_column(dy, first, H), (int)T, cols, reverse, at_column(dgates, first, 4 * H),
                              static_cast<u64 *>(ws), status, at_column(lengths, first, 1));
    };
    return checked(whh && gates && cell && dy && dgates, T, N, H, cu_count, ws, wsb, status, stream, true, launch);
}
#endif

}  // namespace

#ifdef TK_RNN_VARLEN
// The forward-only launch with per-column lengths (include/taiyaki_amd_rnn_varlen.h): the plan, and so the grid and
// the granule buffers, of lstm_forward_dispatch at the same (N, H, cu_count).
size_t lstm_varlen_workspace_bytes(size_t N, size_t H, int cu_count) {
    Plan p;
    if (!lstm_plan(N, H, cu_count, &p)) return 0;
    return ws_bytes(H, p.C, p.groups, p.U, false);
}

int lstm_forward_varlen_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N,
                                 size_t H, int reverse, int cu_count, float *y, void *ws, size_t wsb,
                                 uint32_t *status, hipStream_t stream) {
    return forward<true, false>(gx, whh, lengths, T, N, H, reverse, cu_count, y, nullptr, nullptr, ws, wsb, status,
                                stream);
}
#elif defined(TK_RNN_VARLEN_TRAIN)
// The training pair with per-column lengths (include/taiyaki_amd_rnn_varlen_train.h): the plans, grids and granule
// buffers of lstm_forward_dispatch / lstm_backward_dispatch at the same (N, H, cu_count); the workspace is the
// backward's bound, as tk_lstm_workspace_bytes is.
size_t lstm_varlen_train_workspace_bytes(size_t N, size_t H, int cu_count) {
    return train_workspace_bytes(N, H, cu_count);
}

int lstm_forward_varlen_save_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N,
                                      size_t H, int reverse, int cu_count, float *y, float *gates, float *cell,
                                      void *ws, size_t wsb, uint32_t *status, hipStream_t stream) {
    return forward<true, true>(gx, whh, lengths, T, N, H, reverse, cu_count, y, gates, cell, ws, wsb, status, stream);
}

int lstm_backward_varlen_dispatch(const float *whh, const float *gates, const float *cell, const float *dy,
                                  const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                                  float *dgates, void *ws, size_t wsb, uint32_t *status, hipStream_t stream) {
    return backward<true>(whh, gates, cell, dy, lengths, T, N, H, reverse, cu_count, dgates, ws, wsb, status, stream);
}
#elif defined(TK_LSTM_LARGE)
// Hidden size 512 (include/taiyaki_amd_lstm_large.h): the VL forms at every batch width, on one slab of lstm_slab
// columns after the other, as the -DTK_RNN_WIDE build runs the sizes it covers.
int lstm_large_supported(size_t H) { return H == 512; }

size_t lstm_large_slab(size_t N, size_t H, int cu_count) { return lstm_slab(N, H, cu_count); }

// the training pair's workspace at the widest slab, the first
size_t lstm_large_workspace_bytes(size_t N, size_t H, int cu_count) {
    return train_workspace_bytes(lstm_slab(N, H, cu_count), H, cu_count);
}

// gates and cell may both be NULL: nothing is saved
int lstm_forward_large_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N,
                                size_t H, int reverse, int cu_count, float *y, float *gates, float *cell, void *ws,
                                size_t wsb, uint32_t *status, hipStream_t stream) {
    if (!gates != !cell) return TK_ERR_BAD_ARG;
    return gates ? forward<true, true>(gx, whh, lengths, T, N, H, reverse, cu_count, y, gates, cell, ws, wsb, status,
                                       stream)
                 : forward<true, false>(gx, whh, lengths, T, N, H, reverse, cu_count, y, nullptr, nullptr, ws, wsb,
                                        status, stream);
}

int lstm_backward_large_dispatch(const float *whh, const float *gates, const float *cell, const float *dy,
                                 const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                                 float *dgates, void *ws, size_t wsb, uint32_t *status, hipStream_t stream) {
    return backward<true>(whh, gates, cell, dy, lengths, T, N, H, reverse, cu_count, dgates, ws, wsb, status, stream);
}

#ifdef TK_LAB
void lstm_large_lab_cols(int cols) { g_lab_cols = cols; }

// the eight numbers of lstm_lab_geometry (the admission geometry is the launch's own)
bool lstm_large_lab_geometry(size_t N, size_t H, int cu_count, size_t *out) {
    int C = 0, groups = 0;
    Plan p;
    if (!lstm_geometry(N, H, cu_count, &C, &groups) || !lstm_plan(N, H, cu_count, &p)) return false;
    const size_t v[8] = {(size_t)C, (size_t)groups, (size_t)p.U, (size_t)p.C, (size_t)p.groups, p.grid,
                         ws_bytes(H, p.C, p.groups, p.U, false), ws_bytes(H, p.C, p.groups, p.U, true)};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return true;
}
#endif
#elif defined(TK_RNN_WIDE)
// Every batch width at the sizes the kernels cover (include/taiyaki_amd_rnn_wide.h): the VL forms, on one slab of
// lstm_slab columns after the other.  A batch that one launch admits is one slab: the call of the training pair with
// per-column lengths, or of the forward that saves nothing, at the same (N, H, cu_count).
size_t lstm_wide_slab(size_t N, size_t H, int cu_count) { return lstm_slab(N, H, cu_count); }

// the training pair's workspace at the widest slab, the first
size_t lstm_wide_workspace_bytes(size_t N, size_t H, int cu_count) {
    return train_workspace_bytes(lstm_slab(N, H, cu_count), H, cu_count);
}

// gates and cell may both be NULL: nothing is saved
int lstm_forward_wide_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N,
                               size_t H, int reverse, int cu_count, float *y, float *gates, float *cell, void *ws,
                               size_t wsb, uint32_t *status, hipStream_t stream) {
    if (!gates != !cell) return TK_ERR_BAD_ARG;
    return gates ? forward<true, true>(gx, whh, lengths, T, N, H, reverse, cu_count, y, gates, cell, ws, wsb, status,
                                       stream)
                 : forward<true, false>(gx, whh, lengths, T, N, H, reverse, cu_count, y, nullptr, nullptr, ws, wsb,
                                        status, stream);
}

int lstm_backward_wide_dispatch(const float *whh, const float *gates, const float *cell, const float *dy,
                                const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                                float *dgates, void *ws, size_t wsb, uint32_t *status, hipStream_t stream) {
    return backward<true>(whh, gates, cell, dy, lengths, T, N, H, reverse, cu_count, dgates, ws, wsb, status, stream);
}
#else
size_t lstm_workspace_bytes(size_t N, size_t H, int cu_count) { return train_workspace_bytes(N, H, cu_count); }

int lstm_forward_dispatch(const float *gx, const float *whh, size_t T, size_t N, size_t H, int reverse,
                          int cu_count, float *y, float *gates, float *cell, void *ws, size_t wsb,
                          uint32_t *status, hipStream_t stream) {
    return forward<false, true>(gx, whh, nullptr, T, N, H, reverse, cu_count, y, gates, cell, ws, wsb, status, stream);
}

int lstm_backward_dispatch(const float *whh, const float *gates, const float *cell, const float *dy, size_t T,
                           size_t N, size_t H, int reverse, int cu_count, float *dgates, void *ws, size_t wsb,
                           uint32_t *status, hipStream_t stream) {
    return backward<false>(whh, gates, cell, dy, nullptr, T, N, H, reverse, cu_count, dgates, ws, wsb, status, stream);
}

#ifdef TK_LAB
void lstm_lab_cols(int cols) { g_lab_cols = cols; }
void lstm_lab_units(int units) { g_lab_units = units; }

// out[0..7] = the admitted C and groups, then the launch plan's U, C, groups, grid and its forward and backward
// granule bytes; false where the kernels do not run
bool lstm_lab_geometry(size_t N, size_t H, int cu_count, size_t *out) {
    int C16 = 0, groups16 = 0;
    Plan p;
    if (!lstm_geometry(N, H, cu_count, &C16, &groups16) || !lstm_plan(N, H, cu_count, &p)) return false;
    const size_t v[8] = {(size_t)C16, (size_t)groups16, (size_t)p.U, (size_t)p.C, (size_t)p.groups, p.grid,
                         ws_bytes(H, p.C, p.groups, p.U, false), ws_bytes(H, p.C, p.groups, p.U, true)};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return true;
}
#endif
#endif  // TK_RNN_VARLEN

}  // namespace tk

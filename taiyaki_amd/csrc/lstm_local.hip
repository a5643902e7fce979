// lstm_local.hip -- the recurrence of layers.Lstm (gate order i, f, g, o; h0 = c0 = 0) at a hidden size whose whole
// W_hh fits the registers of ONE workgroup: H = 96, 4 H H floats = 147 456 bytes, 96 floats per lane at 4 H = 384 lanes
// (include/taiyaki_amd_lstm_local.h; libtaiyaki_amd_lstm_local.so).  The cell, the tensors and the VL contract are those
// of lstm_kernels.hip; the geometry is that of gru_kernels.hip at H <= 128 (U = H, G = 1): a workgroup owns every unit
// of its C batch columns, h moves through LDS only, nothing is handed between workgroups.  So there are no granules, no
// workspace, no status word and no bounded spin, the grid may exceed the CU count, and any batch is one launch.
//
// Step schedule (lstm_kernels.hip's rule).  One __syncthreads per step.  Nothing bound for HBM is issued ahead of the
// barrier's wait in the same step: the inputs of the next step are loaded right behind a step's barrier, and a step's
// bulk outputs wait in an LDS block of the step's parity and leave behind the next barrier the workgroup passes, as
// whole rows, 16 bytes per lane (rows_to_global, rnn_common.h).  Both drain under the matvec.
//
// Order of the sums.  A lane adds its products in the order of its k (forward) or rows (backward), which is the same
// at C = 1 and C = 2 (a 16-byte LDS read is 4 rows at C = 1 and 2 rows x 2 columns at C = 2, and a lane's rows come in
// runs of 4); the partial sums of the lanes then meet pairwise over xor 1, 2 (, 4), where an addition commutes.  So a
// column's y, gates, cell and dgates depend on H alone: not on N, not on the other columns, not on C.
//
// Every kernel is the VL form: column n has lengths[n] steps (NULL: T), and a step at t >= lengths[n] writes 0 and hands
// on h = c = 0 (backward: dh = dc = 0) through a select behind the cell update, so what gx and dy hold there is loaded
// and never used.
#include "dispatch.h"
#include "rnn_common.h"

#include "../../include/taiyaki_amd_lstm_local.h"

namespace tk {
namespace {

// The value of lane (lane ^ M) of the wave, as DPP operands of the VALU (lstm_kernels.hip: xor_lane): M = 1, 2 one quad
// permutation, 3 the quad reversed, 4 a mirror of the half row and a reversal of the quad.
template <int M>
__device__ __forceinline__ float xor_lane(float v) {
    static_assert(M >= 1 && M <= 4, "a partner inside the lane's group of 8");
    const int x = __float_as_int(v);
    if constexpr (M == 1) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));      // quad_perm:[1,0,3,2]
    } else if constexpr (M == 2) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));      // quad_perm:[2,3,0,1]
    } else if constexpr (M == 3) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x1B, 0xF, 0xF, true));      // quad_perm:[3,2,1,0]
    } else {
        const int y = __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true);              // row_half_mirror
        return __int_as_float(__builtin_amdgcn_update_dpp(0, y, 0x1B, 0xF, 0xF, true));
    }
}

// The partial sums of the P lanes p ^ M, M = M0, 2 M0, ... < P, meet (lstm_kernels.hip: halve_rounds).  While a lane
// holds REM > 1 accumulators a round halves them: the lane keeps the half that its bit of p names and adds its
// partner's partial sums of that half.  Once it holds one, a round adds the partner's.  A lane ends with accumulator
// index sum over the halving rounds of (bit of p) * REM / 2.
template <int M, int P, int REM, int NA>
__device__ __forceinline__ void meet(float (&acc)[NA], int p) {
    if constexpr (M < P) {
        if constexpr (REM > 1) {
            constexpr int n = REM / 2;
            const bool up = (p & M) != 0;
#pragma unroll
            for (int a = 0; a < n; ++a) {
                const float send = up ? acc[a] : acc[a + n];
                const float keep = up ? acc[a + n] : acc[a];
                acc[a] = keep + xor_lane<M>(send);
            }
            meet<2 * M, P, n>(acc, p);
        } else {
            acc[0] += xor_lane<M>(acc[0]);
            meet<2 * M, P, 1>(acc, p);
        }
    }
}

// Two floats in a register pair, and a fused multiply-add on both halves: one v_pk_fma_f32, each half rounded as fmaf
// rounds (so a sum is the same bits whether its products pair up over gates, at C = 1, or over columns, at C = 2)
typedef float pair2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ pair2 fma2(pair2 a, pair2 b, pair2 c) { return __builtin_elementwise_fma(a, b, c); }

template <int M, int K>
__device__ __forceinline__ void settle(pair2 (&v)[M][K]) {
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) asm volatile("" : "+v"(v[i][k]));
}

// What a lane stores of a staging block of NV values x C columns x H units, [value][column][unit]: the 16-byte chunk
// `tid` (one per lane: NV C H / 4 <= threads), bound for row (value, column) of `base(value)`
template <int H, int C, int NV, class Base>
__device__ __forceinline__ void chunk_target(int tid, int n0, int N, int LD, Base base, float *(&dst)[1],
                                             size_t (&pitch)[1]) {
    constexpr int H4 = H / 4;
    const int row = tid / H4, v = row / C, nn = n0 + row % C;
    size_t width;
    float *b = base(v, width);
    pitch[0] = (size_t)LD * width;
    dst[0] = tid < NV * C * H4 && nn < N ? b + (size_t)nn * width + 4 * (tid % H4) : nullptr;
}

// Forward.  Writes y = h (T, N, H) and, SAVE, the gate activations (T, N, 4H) and c (T, N, H).  Recurrence step s runs
// time t = s (reverse: T - 1 - s).
//
// Lane (u, kp) = (tid / 4, tid % 4): the 4 gate rows of unit u over the columns k = 4 (kp + 4 j) + e (j < H / 16,
// e < 4) of W_hh in VGPRs, so a 16-byte read of h feeds 16 (C 2: 8) weights.  The four partial sums of a (gate, column)
// sit in one quad: they meet by two halving rounds, DPP operands of the adds, after which lane kp holds the sums of ONE
// gate -- i, g, f, o at kp 0, 1, 2, 3 -- in its C columns, adds its own gx and applies that gate's function, as
// lstm_fwd_lanes_body does at (256, 64, 2).  The lane of gate i takes the other three by DPP moves and runs the cell
// update; it leaves h for the next step in hs of the other parity and the step's outputs in the staging block.
template <int H, int C, bool SAVE>
__global__ __launch_bounds__(4 * H, 1) void lstm_local_fwd_kernel(const float *__restrict__ gx,
                                                                  const float *__restrict__ whh, int T, int N,
                                                                  int reverse, float *__restrict__ y,
                                                                  float *__restrict__ gates, float *__restrict__ cell,
                                                                  const int32_t *__restrict__ lengths) {
    constexpr int NT = 4 * H, KP = 4, KS = H / KP, NR = KS / 4;
    constexpr int NV = SAVE ? 6 : 1;                   // staged values: h (, c, i, f, g, o)
    static_assert(H % 16 == 0 && (C == 1 || C == 2) && NV * C * (H / 4) <= NT,
                  "a lane's k in runs of 4; one 16-byte chunk of the staging block per lane");
    __shared__ __attribute__((aligned(16))) float hs[2][H * C];          // h_{t-1} as [k][c], by step parity
    __shared__ __attribute__((aligned(16))) float stg[2][NV * C * H];    // a step's outputs, by step parity

    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * C;
    const int u = tid / KP, kp = tid % KP;
    const int gate = (kp & 1) * 2 + (kp >> 1);         // what the two halving rounds leave in this lane
    const bool cell_lane = kp == 0;

    pair2 w[2][KS];                                    // gates (i, f) and (g, o) of unit u at the lane's k
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) w[g / 2][4 * j + e][g % 2] = whh[((size_t)g * H + u) * H + 4 * (kp + KP * j) + e];
    settle(w);

    bool fetch[C];                                     // a column of the batch: its gx is loaded
    float cst[C];
    int len[C];
#pragma unroll
    for (int v = 0; v < C; ++v) {
        fetch[v] = n0 + v < N;
        cst[v] = 0.f;
        len[v] = !fetch[v] ? 0 : lengths ? lengths[n0 + v] : T;
    }
    for (int i = tid; i < H * C; i += NT) hs[0][i] = 0.f;

    const size_t H4 = 4 * (size_t)H;
    float *rp[1];
    size_t rpitch[1];
    chunk_target<H, C, NV>(tid, n0, N, N, [&](int v, size_t &width) {
        width = v < 2 ? (size_t)H : H4;
        return v == 0 ? y : v == 1 ? cell : gates + (size_t)(v - 2) * H;
    }, rp, rpitch);
    // gx of this lane's gate in its columns, at time 0 (the next column is H4 floats on)
    const float *gx0 = gx + (size_t)n0 * H4 + (size_t)gate * H + u;
    float gq[C];                                       // ... of this step (loaded one step ahead)
#pragma unroll
    for (int v = 0; v < C; ++v) gq[v] = fetch[v] && T > 0 ? gx0[(size_t)(reverse ? T - 1 : 0) * N * H4 + v * H4] : 0.f;
    __syncthreads();

    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        const float *hb = hs[s & 1];
        settle(gq);
        if (s > 0) {
            __syncthreads();                             // hb and the staging block: written by the cell lanes of step s - 1
            rows_to_global<1>(stg[(s - 1) & 1], tid, NT, rp, rpitch, (size_t)(reverse ? t + 1 : t - 1));
        }
        float gn[C];
#pragma unroll
        for (int v = 0; v < C; ++v)
            gn[v] = fetch[v] && s + 1 < T ? gx0[(size_t)(reverse ? t - 1 : t + 1) * N * H4 + v * H4] : 0.f;
        asm volatile("" ::: "memory");                   // the deferred stores and the prefetch stay here

        // C 1: packed FMAs on the gate pairs (i, f) and (g, o) of the column, 48 v_pk_fma_f32 per step where the plain
        // form issues 96 v_fmac_f32: 0.81 us per step against 0.86 (profiles/r39_lstm_local.txt).  C 2: plain FMAs
        // (paired over the two columns the compiler splats every weight into a register pair of its own: 234 VGPRs,
        // and two workgroups no longer share a CU)
        float acc[4 * C];                                // (gate, c) at gate * C + c
        pair2 acc2[2] = {pair2{0.f, 0.f}, pair2{0.f, 0.f}};
#pragma unroll
        for (int a = 0; a < 4 * C; ++a) acc[a] = 0.f;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            float hv[4 * C];                             // h of k = 4 (kp + 4 j) + e as [e][c]
            lds_row<4 * C>(hb + 4 * C * (kp + KP * j), hv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (C == 1) {
#pragma unroll
                    for (int p = 0; p < 2; ++p) acc2[p] = fma2(w[p][4 * j + e], pair2{hv[e], hv[e]}, acc2[p]);
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int c = 0; c < C; ++c)
                            acc[g * C + c] = fmaf(w[g / 2][4 * j + e][g % 2], hv[e * C + c], acc[g * C + c]);
                }
            }
        }
        if constexpr (C == 1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = acc2[g / 2][g % 2];
        }
        meet<1, KP, 4 * C>(acc, kp);                     // acc[v]: `gate` of column n0 + v, summed over the quad

        float ig[C], fg[C], gg[C], og[C];
#pragma unroll
        for (int v = 0; v < C; ++v) {
            const float x = acc[v] + gq[v];
            float a;
            if (gate == 2)
                a = tanhf(x);
            else
                a = sigmoidf(x);
            ig[v] = a;                                   // (what the cell lane, of gate i, reads)
            gg[v] = xor_lane<1>(a);
            fg[v] = xor_lane<2>(a);
            og[v] = xor_lane<3>(a);
        }

        if (cell_lane) {
#pragma unroll
            for (int v = 0; v < C; ++v) {
                // (the contraction written out, as in lstm_kernels.hip: the instantiations must not differ in which
                // product the fma takes)
                cst[v] = fmaf(ig[v], gg[v], fg[v] * cst[v]);
                float h = og[v] * tanhf(cst[v]);
                if (t >= len[v]) {
                    cst[v] = h = 0.f;
                    ig[v] = fg[v] = gg[v] = og[v] = 0.f;
                }
                hs[(s + 1) & 1][u * C + v] = h;
                float *sp = stg[s & 1] + v * H + u;
                sp[0] = h;
                if constexpr (SAVE) {
                    sp[1 * C * H] = cst[v];
                    sp[2 * C * H] = ig[v];
                    sp[3 * C * H] = fg[v];
                    sp[4 * C * H] = gg[v];
                    sp[5 * C * H] = og[v];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < C; ++v) gq[v] = gn[v];
    }
    if (T > 0) {
        __syncthreads();                                 // the last step's block
        rows_to_global<1>(stg[(T - 1) & 1], tid, NT, rp, rpitch, (size_t)(reverse ? 0 : T - 1));
    }
}

// Backward.  From the saved gate activations and c, and dy = dL/dy (T, N, H), writes dgates = dL/d(pre-activation)
// (T, N, 4H), walking the recurrence from its last step:
//   dh = dy + W_hh^T dG of the step behind;  dc = dh o (1 - tanh^2 c) + dc_next f_next;  dG = [dc g i (1 - i),
//   dc c_prev f (1 - f), dc i (1 - g^2), dh tanh(c) o (1 - o)]
//
// Lane (kb, rq) = (tid / 8, tid % 8) holds the 2 columns k = 2 kb + q of the 4 H / 8 rows r = 4 (rq + 8 j) + e
// (j < H / 8, e < 4) of W_hh, so a value of dG read from LDS feeds 2 weights and the 8 lanes rq read 8 adjacent
// 16-byte chunks.  The 8 partial sums of a (k, c) meet inside the wave over xor 1, 2, 4 (DPP operands of the adds, no
// LDS): the rounds halve while a lane holds more than one sum, then add.  Lane rq < 2 C is left with dh of
// k = 2 kb + (rq & 1) in column rq >> 1 and IS the cell lane of that (column, unit): dh never goes through LDS, and a
// step has one barrier, between the cell update that writes dG (by step parity) and the matvec that reads it.  The
// cell lanes leave dG in the staging block too; it goes out as whole rows behind that barrier.
template <int H, int C>
__global__ __launch_bounds__(4 * H, 1) void lstm_local_bwd_kernel(const float *__restrict__ whh,
                                                                  const float *__restrict__ gates,
                                                                  const float *__restrict__ cell,
                                                                  const float *__restrict__ dy, int T, int N,
                                                                  int reverse, float *__restrict__ dgates,
                                                                  const int32_t *__restrict__ lengths) {
    constexpr int NT = 4 * H, RQ = 8, KQ = 2, RR = 4 * H / RQ, NR = RR / 4;
    static_assert(H % 8 == 0 && (C == 1 || C == 2) && (H / KQ) * RQ == NT && 4 * C * (H / 4) <= NT,
                  "a lane's rows in runs of 4; every weight in one lane; one 16-byte chunk of the staging block per lane");
    __shared__ __attribute__((aligned(16))) float dgs[2][4 * H * C];     // dG of a step as [row][c], by step parity
    __shared__ __attribute__((aligned(16))) float stg[2][4 * C * H];     // ... as [gate][column][unit], bound for dgates

    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * C;
    const int kb = tid / RQ, rq = tid % RQ;

    float w[KQ][RR];
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < KQ; ++q) w[q][4 * j + e] = whh[(size_t)(4 * (rq + RQ * j) + e) * H + KQ * kb + q];
    settle(w);

    const bool cell_lane = rq < 2 * C;
    const int u = KQ * kb + (rq & 1), cc = cell_lane ? rq >> 1 : 0;
    const int n = n0 + cc;
    const bool valid = cell_lane && n < N;
    float dc_next = 0.f, f_next = 0.f;
    const int len = !valid ? 0 : lengths ? lengths[n] : T;

    const size_t H4 = 4 * (size_t)H;
    float *rp[1];
    size_t rpitch[1];
    chunk_target<H, C, 4>(tid, n0, N, N, [&](int v, size_t &width) {
        width = H4;
        return dgates + (size_t)v * H;
    }, rp, rpitch);

    // this step's inputs, loaded one step ahead: dy, c_t, c_{t-1}, the four gates (c_t of a step is the c_{t-1} of the
    // step before)
    float in[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid && T > 0) {
        const int t = reverse ? 0 : T - 1;
        const size_t o = ((size_t)t * N + n) * H + u;
        in[0] = dy[o];
        in[1] = cell[o];
        if (T > 1) in[2] = cell[((size_t)(reverse ? t + 1 : t - 1) * N + n) * H + u];
        const float *gp = gates + ((size_t)t * N + n) * H4 + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) in[3 + g] = gp[(size_t)g * H];
    }
    float dhr = 0.f;                                     // W_hh^T dG of the step behind, this lane's (column, unit)

    for (int s = 0; s < T; ++s) {
        const int tt = T - 1 - s;                         // recurrence position
        const int t = reverse ? T - 1 - tt : tt;          // time index
        const int tp = reverse ? t + 1 : t - 1;           // time index of the recurrence's previous step
        settle(in);
        float *db = dgs[s & 1];
        if (cell_lane) {
            const float ct = in[1];
            float cp = in[2];
            if (tp >= len) cp = 0.f;                      // (reverse: the column's first step starts from c = 0)
            const float ig = in[3], gg = in[5], og = in[6];
            float fg = in[4];
            const float dh = in[0] + dhr;
            const float tc = tanhf(ct);
            float dc = dh * og * (1.f - tc * tc) + dc_next * f_next;
            float di = dc * gg * ig * (1.f - ig);
            float df = dc * cp * fg * (1.f - fg);
            float dg = dc * ig * (1.f - gg * gg);
            float dout = dh * tc * og * (1.f - og);
            if (t >= len) dc = fg = di = df = dg = dout = 0.f;       // (also a column past N: len 0)
            dc_next = dc;
            f_next = fg;
            db[(0 * H + u) * C + cc] = di;
            db[(1 * H + u) * C + cc] = df;
            db[(2 * H + u) * C + cc] = dg;
            db[(3 * H + u) * C + cc] = dout;
            float *sp = stg[s & 1] + cc * H + u;
            sp[0 * C * H] = di;
            sp[1 * C * H] = df;
            sp[2 * C * H] = dg;
            sp[3 * C * H] = dout;
        }
        __syncthreads();
        // behind the barrier: the next step's inputs, then this step's dG as whole rows; both drain under the matvec
        float nx[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (valid && tt > 0) {
            const size_t o = ((size_t)tp * N + n) * H + u;
            nx[0] = dy[o];
            nx[1] = in[2];
            if (tt > 1) nx[2] = cell[((size_t)(reverse ? tp + 1 : tp - 1) * N + n) * H + u];
            const float *gp = gates + ((size_t)tp * N + n) * H4 + u;
#pragma unroll
            for (int g = 0; g < 4; ++g) nx[3 + g] = gp[(size_t)g * H];
        }
        rows_to_global<1>(stg[s & 1], tid, NT, rp, rpitch, (size_t)t);
        asm volatile("" ::: "memory");                   // the stores and the prefetch stay here
#pragma unroll
        for (int q = 0; q < 7; ++q) in[q] = nx[q];
        if (s + 1 == T) break;                            // the first step has no predecessor to feed

        // (plain FMAs at either C: at C 1 the packed form over the lane's two columns k, 48 v_pk_fma_f32 per step,
        // measured 1.17 us per step against 0.86, profiles/r39_lstm_local.txt)
        float acc[KQ * C];                               // (q, c) at q * C + c
#pragma unroll
        for (int a = 0; a < KQ * C; ++a) acc[a] = 0.f;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            float d[4 * C];                              // dG of rows 4 (rq + 8 j) + e as [e][c]
            lds_row<4 * C>(db + 4 * C * (rq + RQ * j), d);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < KQ; ++q)
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[q * C + c] = fmaf(w[q][4 * j + e], d[e * C + c], acc[q * C + c]);
        }
        meet<1, RQ, KQ * C>(acc, rq);                    // rq < 2 C: dh of (k, c) = (2 kb + (rq & 1), rq >> 1)
        dhr = acc[0];
    }
}

int g_lab_cols = 0;     // lab build: force the batch columns per workgroup, 1 or 2 (0 = the rule below)

constexpr bool size_built(size_t H) { return H == 96; }

// The batch columns per workgroup; 0 where the kernels do not run.  gru_plan's rule: 1 column where every column gets a
// CU of its own, else 2 (tools/lstmlocalbench.py on 256 CUs, us per forward / backward step, profiles/r39_lstm_local.txt:
// T 800 N 128 0.81 / 0.87 at 1 column, 1.37 / 1.14 at 2; T 400 N 256 0.84 / 0.90, 1.38 / 1.16; T 200 N 512 1.30 / 1.85,
// 1.41 / 1.21 -- above the CU count the forward alone is 8 % faster at 1 column, the pair 17 % slower).
int local_columns(size_t N, size_t H, int cu_count) {
    if (!size_built(H) || N == 0 || N > (size_t)INT32_MAX || cu_count <= 0) return 0;
    if (g_lab_cols == 1 || g_lab_cols == 2) return g_lab_cols;
    return N <= (size_t)cu_count ? 1 : 2;
}

// what both dispatchers do in front of their launch: TK_OK where there is something to launch, `done` set where not
int checked(bool pointers_ok, size_t T, size_t N, size_t H, int cu_count, int *C, bool *done) {
    *done = true;
    if (!pointers_ok || T > (size_t)INT32_MAX || N > (size_t)INT32_MAX) return TK_ERR_BAD_ARG;
    *C = local_columns(N, H, cu_count);
    if (*C == 0) return TK_ERR_UNSUPPORTED;
    *done = T == 0;
    return TK_OK;
}

#define TK_LSTM_LOCAL_SWITCH(LAUNCH)                                                                              \
    switch ((int)H * 10 + C) {                                                                                    \
        LAUNCH(96, 1) LAUNCH(96, 2)                                                                               \
        default: return TK_ERR_UNSUPPORTED;                                                                       \
    }

}  // namespace

int lstm_local_supported(size_t H) { return size_built(H) ? 1 : 0; }

int lstm_local_columns(size_t N, size_t H, int cu_count) { return local_columns(N, H, cu_count); }

int lstm_local_forward_dispatch(const float *gx, const float *whh, const int32_t *lengths, size_t T, size_t N, size_t H,
                                int reverse, int cu_count, float *y, float *gates, float *cell, hipStream_t stream) {
    if (!gates != !cell) return TK_ERR_BAD_ARG;
    int C;
    bool done;
    const int rc = checked(gx && whh && y && aligned16(gx) && aligned16(y) && aligned16(gates) && aligned16(cell), T, N,
                           H, cu_count, &C, &done);
    if (done) return rc;
    const unsigned grid = (unsigned)((N + C - 1) / C);
#define TK_LSTM_LOCAL_FWD(HH, CC)                                                                                 \
    case HH * 10 + CC:                                                                                            \
        if (gates)                                                                                                \
            hipLaunchKernelGGL((lstm_local_fwd_kernel<HH, CC, true>), dim3(grid), dim3(4 * HH), 0, stream, gx, whh,     \
                               (int)T, (int)N, reverse, y, gates, cell, lengths);                                 \
        else                                                                                                      \
            hipLaunchKernelGGL((lstm_local_fwd_kernel<HH, CC, false>), dim3(grid), dim3(4 * HH), 0, stream, gx, whh,    \
                               (int)T, (int)N, reverse, y, gates, cell, lengths);                                 \
        break;
    TK_LSTM_LOCAL_SWITCH(TK_LSTM_LOCAL_FWD)
#undef TK_LSTM_LOCAL_FWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

int lstm_local_backward_dispatch(const float *whh, const float *gates, const float *cell, const float *dy,
                                 const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                                 float *dgates, hipStream_t stream) {
    int C;
    bool done;
    const int rc = checked(whh && gates && cell && dy && dgates && aligned16(gates) && aligned16(cell) && aligned16(dy) &&
                               aligned16(dgates),
                           T, N, H, cu_count, &C, &done);
    if (done) return rc;
    const unsigned grid = (unsigned)((N + C - 1) / C);
#define TK_LSTM_LOCAL_BWD(HH, CC)                                                                                 \
    case HH * 10 + CC:                                                                                            \
        hipLaunchKernelGGL((lstm_local_bwd_kernel<HH, CC>), dim3(grid), dim3(4 * HH), 0, stream, whh, gates, cell, dy,  \
                           (int)T, (int)N, reverse, dgates, lengths);                                             \
        break;
    TK_LSTM_LOCAL_SWITCH(TK_LSTM_LOCAL_BWD)
#undef TK_LSTM_LOCAL_BWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}
#undef TK_LSTM_LOCAL_SWITCH

#ifdef TK_LAB
void lstm_local_lab_cols(int cols) { g_lab_cols = cols; }
#endif

}  // namespace tk

extern "C" {

int tk_lstm_local_supported(size_t size) { return tk::lstm_local_supported(size); }

int tk_lstm_local_columns(size_t nbatch, size_t size, int cu_count) {
    return tk::lstm_local_columns(nbatch, size, cu_count);
}

int tk_lstm_local_forward_dev(const float *gx, const float *w_hh, const int32_t *lengths, size_t nblk, size_t nbatch,
                              size_t size, int reverse, int cu_count, float *y, float *gates, float *cell,
                              void *stream) {
    return tk::lstm_local_forward_dispatch(gx, w_hh, lengths, nblk, nbatch, size, reverse, cu_count, y, gates, cell,
                                           static_cast<hipStream_t>(stream));
}

int tk_lstm_local_backward_dev(const float *w_hh, const float *gates, const float *cell, const float *dy,
                               const int32_t *lengths, size_t nblk, size_t nbatch, size_t size, int reverse,
                               int cu_count, float *dgates, void *stream) {
    return tk::lstm_local_backward_dispatch(w_hh, gates, cell, dy, lengths, nblk, nbatch, size, reverse, cu_count, dgates,
                                            static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
void tk_lab_lstm_local_cols(int cols) { tk::lstm_local_lab_cols(cols); }
#endif

}  // extern "C"

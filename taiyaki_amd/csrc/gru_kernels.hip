// gru_kernels.hip -- the recurrence of layers.GruMod (one nn.GRU layer, gate order r, z, n; h0 = 0) as one
// persistent, weight-stationary launch per layer and direction of the pass.
//
//   a = W_hh h_prev;  r = sigmoid(gx_r + a_r + bhh_r);  z = sigmoid(gx_z + a_z + bhh_z);  q = a_n + bhh_n;
//   n = tanh(gx_n + r q);  h = (1 - z) n + z h_prev                       (gx = x W_ih^T + b_ih, the caller's GEMM)
//
// Geometry.  A workgroup owns U hidden units (their 3 U gate rows of W_hh, held in VGPRs for the whole launch) and
// C batch columns; the G = H / U workgroups that share the columns form a group.
//   H <= 128: U = H, G = 1.  One workgroup of 4 H lanes holds the whole W_hh (3 H / 4 floats per lane: 72 at
//     H = 96), h moves through LDS only, nothing is handed between workgroups: no co-residency requirement, any N.
//     C = 1 where N <= the CU count, else 2 (gru_plan has the measurements).
//   H = 256: U = 64, G = 4, C = 4, 512 lanes with 96 weight floats each.  Every step is an all-to-all inside the group, as
//     in lstm_kernels.hip: forward each member needs the whole h_{t-1} of its columns, backward the sum over members
//     of W_hh[rows(m), J]^T dG[rows(m)] for its units J (summed in producer order: bit-reproducible).  Both go
//     through the tagged granules of rnn_common.h.  Such a grid is co-resident by construction: it is admitted
//     only where groups * G <= cu_count, at one workgroup per CU (__launch_bounds__(threads, 1)).
//   H = 192, 384: U = 48, G = H / 48 (4, 8), as in lstm_kernels.hip, handed on through the granules like H = 256.
//     C = 4 where ceil(N / 4) * G <= cu_count, else 8 where ceil(N / 8) * G <= cu_count, else the batch is refused.
//     Forward 384 lanes (u, kp) at KP = 8: 72 weight floats per lane at H = 192, 144 at 384.  Backward 2 H lanes
//     (384, 768), two per column of W_hh, 72 floats each at either size.
//
// Step schedule (lstm_kernels.hip's rule).  Nothing bound for HBM is issued ahead of a poll in the same step: the
// inputs of step s + 1 are loaded right after step s's poll (G = 1: barrier), the bulk outputs of step s are held
// in registers and stored right after step s + 1's.  Both drain under the matvec; the granule publish is the last
// memory operation of a step.  Every sum runs in a fixed order: a launch is bit-reproducible.
//
// Columns: `cols.n` of them in tensors of `cols.ld()` per time step, as in lstm_kernels.hip.
//
// Four builds of this one source, as for lstm_kernels.hip: -DTK_RNN_WIDE (libtaiyaki_amd_rnn_wide.so) takes the three VL
// forms on slabs of a batch's columns (`checked`; gru_slab), the flip-flop library takes the forward and the backward,
// -DTK_RNN_VARLEN (libtaiyaki_amd_rnn_varlen.so) the forward alone in its VL form with nothing saved,
// -DTK_RNN_VARLEN_TRAIN (libtaiyaki_amd_rnn_varlen_train.so) the saving forward and the backward in their VL form.
#include "dispatch.h"
#include "ff_common.h"
#include "rnn_common.h"

namespace tk {
namespace {

constexpr int kCols = 4;        // batch columns per workgroup at H = 256, and where they fit at H = 192 and 384

// threads per workgroup: 4 per unit where one workgroup owns every unit, 8 per unit at U = 64 of H = 256 and at U = 48
// of H = 192 and 384
template <int H, int U>
constexpr int gru_threads() { return U == H ? 4 * U : U == 48 ? 384 : 512; }
// ... of the backward: two lanes per column of W_hh at U = 48, 72 floats per lane at either size
template <int H, int U>
constexpr int bwd_threads_for() { return U == 48 ? 2 * H : gru_threads<H, U>(); }

// Forward.  Writes y = h (T, N, H) and, where the pointers are not NULL, the activations r, z, n as gates (T, N, 3H)
// and q (T, N, H).  Recurrence step s runs time t = s (reverse: T - 1 - s).  hbuf (G > 1): [2][ngroups][C][H]
// granules.
//
// Lane (u, kp), kp < KP = threads / U: the 3 gate rows of unit u over the columns k = i KP + kp (i < KS = H / KP)
// in VGPRs, so each h value read from LDS feeds 3 rows.  The KP partial sums are combined by xor shuffles: the first
// log2(C) rounds halve the columns a lane keeps, the rest add the gates of its one column; lane kp < C then holds
// the 3 hidden-side sums of column col(kp) and runs its cell update.
//
// VL: column n has lengths[n] steps (NULL: T).  A step at t >= lengths[n] leaves h = 0, writes y = 0 and hands h = 0
// on like any other step.  SAVE: gates and qout are written where they are not NULL (with VL: 0 on a step at or beyond
// the length); not SAVE: they are not written (the pointers are not read).
template <int H, int U, int C, bool VL = false, bool SAVE = !VL>
__global__ __launch_bounds__((gru_threads<H, U>()), 1) void gru_fwd_kernel(
    const float *__restrict__ gx, const float *__restrict__ whh, const float *__restrict__ bhh, int T, Cols cols,
    int reverse, int ngroups, float *__restrict__ y, float *__restrict__ gates, float *__restrict__ qout, u64 *hbuf,
    uint32_t *status, const int32_t *__restrict__ lengths) {
    constexpr int NT = gru_threads<H, U>();
    const int N = cols.n, LD = cols.ld();               // the launch's columns; the tensors' columns per time step
    constexpr int G = H / U;
    constexpr int KP = NT / U;
    constexpr int KS = H / KP;
    constexpr int NG = (H * C + NT - 1) / NT;
    static_assert(KP * U == NT && KS * KP == H && KP <= 64 && 64 % KP == 0 && C <= KP,
                  "lane (u, kp) inside one wave; one cell lane per (u, column)");
    __shared__ __attribute__((aligned(16))) float hs[2][H * C];      // h_{t-1} as [k][c], by step parity
    __shared__ int give_up;

    int group = blockIdx.x, member = 0;
    if constexpr (G > 1) place(G, group, member);
    const int tid = threadIdx.x;
    const int j0 = member * U, n0 = group * C;
    const int u = tid / KP, kp = tid % KP;

    float w[3][KS];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i = 0; i < KS; ++i) w[g][i] = whh[((size_t)g * H + j0 + u) * H + i * KP + kp];
    settle(w);
    float bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) bh[g] = bhh[g * H + j0 + u];
    settle(bh);

    int col = 0;                                       // the column this lane keeps through the reduction
#pragma unroll
    for (int m = 1, width = C; width > 1; m <<= 1, width >>= 1)
        if (kp & m) col += width / 2;
    const bool cell_lane = kp < C;
    const int n = n0 + col;
    const bool valid = cell_lane && n < N;
    float hprev = 0.f;
    int len = 0;                                       // VL: the steps of this lane's column
    if constexpr (VL) len = !valid ? 0 : lengths ? lengths[n] : T;

    for (int i = tid; i < H * C; i += NT) hs[0][i] = 0.f;
    if (tid == 0) give_up = 0;

    const size_t H3 = 3 * (size_t)H;
    float gq[3] = {0.f, 0.f, 0.f};                    // gx of this step (loaded one step ahead)
    if (valid) {
        const float *p = gx + ((size_t)(reverse ? T - 1 : 0) * LD + n) * H3 + j0 + u;
#pragma unroll
        for (int g = 0; g < 3; ++g) gq[g] = p[(size_t)g * H];
    }
    float held[5] = {0.f, 0.f, 0.f, 0.f, 0.f};        // h, r, z, n, q of the previous step, stored one step late
    __syncthreads();

    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        float *hb = hs[s & 1];
        settle(gq);
        if (s > 0) {
            if constexpr (G > 1) {
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
            } else {
                __syncthreads();                             // hb: written by the cell lanes of step s - 1
            }
            if (valid) {
                const size_t row = (size_t)(reverse ? t + 1 : t - 1) * LD + n;
                y[row * H + j0 + u] = held[0];
                if constexpr (SAVE) {
                    if (gates) {
                        float *gp = gates + row * H3 + j0 + u;
#pragma unroll
                        for (int g = 0; g < 3; ++g) gp[(size_t)g * H] = held[1 + g];
                    }
                    if (qout) qout[row * H + j0 + u] = held[4];
                }
            }
        }
        float gn[3] = {0.f, 0.f, 0.f};
        if (valid && s + 1 < T) {
            const float *p = gx + ((size_t)(reverse ? t - 1 : t + 1) * LD + n) * H3 + j0 + u;
#pragma unroll
            for (int g = 0; g < 3; ++g) gn[g] = p[(size_t)g * H];
        }
        asm volatile("" ::: "memory");                   // the deferred stores and the prefetch stay here

        float acc[3][C];
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[g][c] = 0.f;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            float hv[C];
            lds_row<C>(hb + (i * KP + kp) * C, hv);
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[g][c] = fmaf(w[g][i], hv[c], acc[g][c]);
        }
#pragma unroll
        for (int m = 1; m < KP; m <<= 1) {
            const int half = C / (2 * m);                // 0 once a lane keeps one column
            const bool up = (kp & m) != 0;
#pragma unroll
            for (int g = 0; g < 3; ++g) {
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
            float rg = sigmoidf(gq[0] + acc[0][0] + bh[0]), zg = sigmoidf(gq[1] + acc[1][0] + bh[1]);
            float qv = acc[2][0] + bh[2];
            float ng = tanhf(gq[2] + rg * qv);
            // (two products and a sum, no contraction: left to the compiler, the saving kernel at H 32 and 64 took
            // fma(zg, hprev, (1 - zg) ng) where its VL twin, like every instantiation at H >= 96, multiplies the pair
            // with one v_pk_mul_f32 and adds -- lengths = NULL then differed from the saving forward in the last bit)
            float h;
            {
#pragma clang fp contract(off)
                h = (1.f - zg) * ng + zg * hprev;
            }
            if constexpr (VL) {
                if (t >= len) {
                    h = 0.f;
                    if constexpr (SAVE) rg = zg = ng = qv = 0.f;
                }
            }
            hprev = h;
            if (s + 1 < T) {
                if constexpr (G > 1)
                    store_granule(hbuf + ((size_t)(s & 1) * ngroups + group) * (H * C) + col * H + j0 + u,
                                  (unsigned)(s + 1), h);
                else
                    hs[(s + 1) & 1][u * C + col] = h;
            }
            held[0] = h;
            held[1] = rg;
            held[2] = zg;
            held[3] = ng;
            held[4] = qv;
        }
#pragma unroll
        for (int g = 0; g < 3; ++g) gq[g] = gn[g];
    }
    if (valid && T > 0) {
        const size_t row = (size_t)(reverse ? 0 : T - 1) * LD + n;
        y[row * H + j0 + u] = held[0];
        if constexpr (SAVE) {
            if (gates) {
                float *gp = gates + row * H3 + j0 + u;
#pragma unroll
                for (int g = 0; g < 3; ++g) gp[(size_t)g * H] = held[1 + g];
            }
            if (qout) qout[row * H + j0 + u] = held[4];
        }
    }
}

#ifndef TK_RNN_VARLEN
// Backward.  From y, the saved activations r, z, n and q, and dy = dL/dy (T, N, H), writes dgates = dL/d(gx) =
// [dr_pre, dz_pre, dn_pre] (T, N, 3H) and dq = dn_pre r (T, N, H), walking the recurrence from its last step:
//   dh = dy + dh_rec;  dn_pre = dh (1 - z)(1 - n^2);  dz_pre = dh (h_prev - n) z (1 - z);  dr_pre = dn_pre q r (1 - r)
//   dh_rec of the step before = dh z + W_hh^T [dr_pre, dz_pre, dq]
// Lane (k, rp), rp < RP = threads / H, holds W_hh[every RP-th owned row from rp, k] of the owned 3 U rows; the RP partial sums meet in
// LDS.  G = 1: the cell lane of (column, unit) adds them there.  G > 1: pbuf [2][ngroups][G producers][C][H] granules.
//
// VL: column n has lengths[n] steps (NULL: T).  A step at t >= lengths[n] writes dgates = 0 and dq = 0 and hands on
// dh = 0 (its rows in LDS are 0, so is what it publishes; the carried dh z is 0), like any other step.  The mask is a
// select behind the cell update: dy and the saved rows beyond the length are loaded and never used.
template <int H, int U, int C, bool VL = false>
__global__ __launch_bounds__((bwd_threads_for<H, U>()), 1) void gru_bwd_kernel(
    const float *__restrict__ whh, const float *__restrict__ y, const float *__restrict__ gates,
    const float *__restrict__ qin, const float *__restrict__ dy, int T, Cols cols, int reverse, int ngroups,
    float *__restrict__ dgates, float *__restrict__ dqout, u64 *pbuf, uint32_t *status,
    const int32_t *__restrict__ lengths) {
    constexpr int NT = bwd_threads_for<H, U>();
    const int N = cols.n, LD = cols.ld();               // the launch's columns; the tensors' columns per time step
    constexpr int G = H / U;
    constexpr int RP = NT / H;                        // row partitions
    constexpr int R = 3 * U / RP;                     // floats per lane
    constexpr int PAIRS = U * C;                      // (c, u) pairs of the cell update
    constexpr int PL = NT / PAIRS;                    // producer planes of the gather
    constexpr int NP = (G + PL - 1) / PL;
    static_assert(RP >= 1 && RP * H == NT && R * RP == 3 * U && PL >= 1 && PL * PAIRS == NT,
                  "every lane polls; one cell lane per pair");
    __shared__ __attribute__((aligned(16))) float dgs[3 * U * C];      // [dr, dz, dq] of the owned rows as [row][c]
    __shared__ float gath[G > 1 ? PL * PAIRS : 1];
    __shared__ __attribute__((aligned(16))) float red[RP * C * H];
    __shared__ int give_up;

    int group = blockIdx.x, member = 0;
    if constexpr (G > 1) place(G, group, member);
    const int tid = threadIdx.x;
    const int j0 = member * U, n0 = group * C;

    // lane (k, rp) takes the owned rows i RP + rp (i < R): RP divides U, so row i RP + rp is unit (i RP) % U + rp of
    // gate (i RP) / U, a constant offset from the lane's first weight
    static_assert(U % RP == 0, "a lane's rows keep their gate index at compile time");
    const int k = tid % H, rp = tid / H;
    float w[R];
    const float *wbase = whh + (size_t)(j0 + rp) * H + k;
#pragma unroll
    for (int i = 0; i < R; ++i) w[i] = wbase[(unsigned)((((i * RP) / U) * H + (i * RP) % U) * H)];
    settle(w);

    const bool cell_lane = tid < PAIRS;
    const int pair = tid % PAIRS, plane = tid / PAIRS;
    const int cc = pair / U, u = pair % U;
    const int n = n0 + cc;
    const bool valid = cell_lane && n < N;
    float carry = 0.f;                                // dh z of the step before
    int len = 0;                                       // VL: the steps of this lane's column
    if constexpr (VL) len = !valid ? 0 : lengths ? lengths[n] : T;
    if (tid == 0) give_up = 0;

    // this step's inputs, loaded one step ahead: dy, r, z, n, q and h_prev (y of the recurrence's previous step)
    const size_t H3 = 3 * (size_t)H;
    float in[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const int t = reverse ? 0 : T - 1;
        const size_t row = (size_t)t * LD + n;
        in[0] = dy[row * H + j0 + u];
        const float *gp = gates + row * H3 + j0 + u;
#pragma unroll
        for (int g = 0; g < 3; ++g) in[1 + g] = gp[(size_t)g * H];
        in[4] = qin[row * H + j0 + u];
        if (T > 1) in[5] = y[((size_t)(reverse ? t + 1 : t - 1) * LD + n) * H + j0 + u];
    }
    float held[4] = {0.f, 0.f, 0.f, 0.f};             // dr_pre, dz_pre, dn_pre, dq of the previous step, stored late
    __syncthreads();

    const u64 *mine = pbuf + (size_t)group * G * C * H + cc * H + j0 + u;
    for (int s = 0; s < T; ++s) {
        const int tt = T - 1 - s;                         // recurrence position
        const int t = reverse ? T - 1 - tt : tt;          // time index
        const int tp = reverse ? t + 1 : t - 1;           // time index of the recurrence's previous step
        settle(in);
        float dhr = 0.f;
        if (s > 0) {
            if constexpr (G > 1) {
                float v[NP];
                const int nvalid = plane < G ? (G - plane + PL - 1) / PL : 0;
                const u64 *src = mine + (size_t)((s - 1) & 1) * ngroups * G * C * H;
                if (!sweep<NP>(src, plane * C * H, PL * C * H, G * C * H, (unsigned)s, v, status)) give_up = 1;
                float sum = 0.f;
#pragma unroll
                for (int q = 0; q < NP; ++q)
                    if (q < nvalid) sum += v[q];
                gath[plane * PAIRS + pair] = sum;
                __syncthreads();
                if (give_up) return;
                if (cell_lane) {
#pragma unroll
                    for (int p = 0; p < PL; ++p) dhr += gath[p * PAIRS + pair];
                }
            } else {
                __syncthreads();                          // red: the partial sums of step s - 1
#pragma unroll
                for (int q = 0; q < RP; ++q) dhr += red[(q * C + cc) * H + u];
            }
            if (valid) {
                const size_t row = (size_t)(reverse ? t - 1 : t + 1) * LD + n;
                float *dp = dgates + row * H3 + j0 + u;
#pragma unroll
                for (int g = 0; g < 3; ++g) dp[(size_t)g * H] = held[g];
                dqout[row * H + j0 + u] = held[3];
            }
        }
        float nx[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (valid && tt > 0) {
            const size_t row = (size_t)tp * LD + n;
            nx[0] = dy[row * H + j0 + u];
            const float *gp = gates + row * H3 + j0 + u;
#pragma unroll
            for (int g = 0; g < 3; ++g) nx[1 + g] = gp[(size_t)g * H];
            nx[4] = qin[row * H + j0 + u];
            if (tt > 1) nx[5] = y[((size_t)(reverse ? tp + 1 : tp - 1) * LD + n) * H + j0 + u];
        }
        asm volatile("" ::: "memory");                   // the deferred stores and the prefetch stay here

        if (cell_lane) {
            const float rg = in[1], zg = in[2], ng = in[3], qv = in[4];
            float hp = in[5];
            if constexpr (VL) {
                if (tp >= len) hp = 0.f;                  // (reverse: the column's first step starts from h = 0)
            }
            const float dh = in[0] + dhr + carry;
            float dn = dh * (1.f - zg) * (1.f - ng * ng);
            float dz = dh * (hp - ng) * zg * (1.f - zg);
            float dq = dn * rg;
            float dr = dn * qv * rg * (1.f - rg);
            carry = dh * zg;
            if constexpr (VL) {
                if (t >= len) carry = dn = dz = dq = dr = 0.f;
            }
            held[0] = dr;
            held[1] = dz;
            held[2] = dn;
            held[3] = dq;
            dgs[(0 * U + u) * C + cc] = valid ? dr : 0.f;
            dgs[(1 * U + u) * C + cc] = valid ? dz : 0.f;
            dgs[(2 * U + u) * C + cc] = valid ? dq : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) in[q] = nx[q];
        __syncthreads();
        if (s + 1 == T) break;                            // the first step has no predecessor to feed

        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            float d[C];
            lds_row<C>(dgs + (i * RP + rp) * C, d);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = fmaf(w[i], d[c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) red[(rp * C + c) * H + k] = acc[c];
        if constexpr (G > 1) {
            u64 *dst = pbuf + (((size_t)(s & 1) * ngroups + group) * G + member) * C * H;
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
        const size_t row = (size_t)(reverse ? T - 1 : 0) * LD + n;
        float *dp = dgates + row * H3 + j0 + u;
#pragma unroll
        for (int g = 0; g < 3; ++g) dp[(size_t)g * H] = held[g];
        dqout[row * H + j0 + u] = held[3];
    }
}

#endif  // TK_RNN_VARLEN: no backward

// A launch: U units and C columns per workgroup, groups of G = H / U workgroups; false where the kernels do not
// run.  H <= 128 is one workgroup per group (any N); H = 256 hands h between the 4 members of a group, so its grid
// must be co-resident: groups * 4 <= cu_count at one workgroup per CU.  H = 192 and 384: groups of H / 48 members with
// 4 columns where such a grid is co-resident, else with 8, else refused.
struct Plan {
    int U, G, C, groups;
    unsigned grid;
};

int g_lab_cols = 0;     // lab build: force the batch columns per workgroup at H <= 128: 1 or 2 (0 = the rule below)

bool gru_plan(size_t N, size_t H, int cu_count, Plan *p) {
    const bool u48 = H == 192 || H == 384;
    if (!(u48 || H == 32 || H == 64 || H == 96 || H == 128 || H == 256) || N == 0 || N > (size_t)INT32_MAX ||
        cu_count <= 0)
        return false;
    p->U = u48 ? 48 : H == 256 ? 64 : (int)H;
    p->G = (int)H / p->U;
    // one workgroup per group: 1 column where every column gets a CU of its own, else 2 (tools/grubench.py, us per
    // forward / backward step at H = 96: N = 64 0.88 / 0.81 at 1 column, 1.08 / 1.15 at 2, 1.45 / 1.72 at 4;
    // N = 512 1.28 / 1.11, 1.17 / 1.17, 1.49 / 1.75; 4 columns lost everywhere and is not built)
    p->C = p->G > 1 ? kCols : N <= (size_t)cu_count ? 1 : 2;
    if (p->G == 1 && g_lab_cols != 0) {
        if (g_lab_cols != 1 && g_lab_cols != 2) return false;
        p->C = g_lab_cols;
    }
    if (u48 && (N + 3) / 4 * p->G > (size_t)cu_count) p->C = 8;
    const size_t groups = (N + p->C - 1) / p->C;
    if (p->G > 1 && groups * p->G > (size_t)cu_count) return false;
    p->groups = (int)groups;
    p->grid = (unsigned)(groups * p->G);
    return true;
}

// granule bytes of a launch (0 at G = 1: nothing is handed between workgroups)
size_t gru_ws_bytes(size_t H, const Plan &p, bool backward) {
    if (p.G == 1) return 0;
    return 2 * (size_t)p.groups * (backward ? p.G : 1) * p.C * H * sizeof(u64);
}

#define TK_GRU_SWITCH(LAUNCH)                                                                                     \
    switch ((int)H * 10 + p.C) {                                                                                  \
        LAUNCH(256, 64, 4) LAUNCH(192, 48, 4) LAUNCH(192, 48, 8) LAUNCH(384, 48, 4) LAUNCH(384, 48, 8)            \
        LAUNCH(32, 32, 2) LAUNCH(64, 64, 2) LAUNCH(96, 96, 2) LAUNCH(128, 128, 2)                                 \
        LAUNCH(32, 32, 1) LAUNCH(64, 64, 1) LAUNCH(96, 96, 1) LAUNCH(128, 128, 1)                                 \
        default: return TK_ERR_UNSUPPORTED;                                                                       \
    }

template <bool VL, bool SAVE>
int launch_fwd(const Plan &p, size_t H, hipStream_t st, const float *gx, const float *whh, const float *bhh, int T,
               Cols cols, int rev, float *y, float *gates, float *q, u64 *ws, uint32_t *status, const int32_t *lengths) {
#define TK_GRU_FWD(HH, UU, CC)                                                                                    \
    case HH * 10 + CC:                                                                                            \
        hipLaunchKernelGGL((gru_fwd_kernel<HH, UU, CC, VL, SAVE>), dim3(p.grid), dim3(gru_threads<HH, UU>()), 0, st,    \
                           gx, whh, bhh, T, cols, rev, p.groups, y, gates, q, ws, status, lengths);               \
        break;
    TK_GRU_SWITCH(TK_GRU_FWD)
#undef TK_GRU_FWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

#ifndef TK_RNN_VARLEN
template <bool VL>
int launch_bwd(const Plan &p, size_t H, hipStream_t st, const float *whh, const float *y, const float *gates,
               const float *q, const float *dy, int T, Cols cols, int rev, float *dg, float *dq, u64 *ws,
               uint32_t *status, const int32_t *lengths) {
#define TK_GRU_BWD(HH, UU, CC)                                                                                    \
    case HH * 10 + CC:                                                                                            \
        hipLaunchKernelGGL((gru_bwd_kernel<HH, UU, CC, VL>), dim3(p.grid), dim3(bwd_threads_for<HH, UU>()), 0,    \
                           st, whh, y, gates, q, dy, T, cols, rev, p.groups, dg, dq, ws, status, lengths);        \
        break;
    TK_GRU_SWITCH(TK_GRU_BWD)
#undef TK_GRU_BWD
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}
#endif  // TK_RNN_VARLEN
#undef TK_GRU_SWITCH

// The slab width of a batch of N columns (rnn_common.h has the rule): the widest batch gru_plan admits at
// (H, cu_count), or N where one launch admits the batch (H <= 128: always); 0 where the kernels do not run.
size_t gru_slab(size_t N, size_t H, int cu_count) {
    Plan p;
    const size_t S = widest_admitted([&](size_t n) { return gru_plan(n, H, cu_count, &p); });
    return N == 0 ? 0 : N < S ? N : S;
}

// What every dispatcher below does around its launch, written once: the pointer and range checks (`pointers_ok`: the
// entry's own required pointers), then for every slab of the batch its plan, the workspace's size, nothing to do at
// T == 0, the granules zeroed where there are any, then `launch(plan, the slab's first column, its columns)`.  The
// -DTK_RNN_WIDE build alone cuts a batch: everywhere else the one slab is the batch, and a batch that no launch admits
// is refused.  The slabs share the workspace and follow each other on `stream`, never side by side (lstm_kernels.hip:
// checked); the first is the widest and has the largest plan; a launch error returns at once.
template <class Launch>
int checked(bool pointers_ok, size_t T, size_t N, size_t H, int cu_count, void *ws, size_t wsb, uint32_t *status,
            hipStream_t stream, bool backward, Launch launch) {
    if (!pointers_ok || !ws || !status || !aligned16(ws) || T > (size_t)INT32_MAX || N > (size_t)INT32_MAX)
        return TK_ERR_BAD_ARG;
#ifdef TK_RNN_WIDE
    const size_t S = gru_slab(N, H, cu_count);
#else
    const size_t S = N;
#endif
    if (S == 0) return TK_ERR_UNSUPPORTED;
    for (size_t first = 0; first < N; first += S) {
        const size_t n = N - first < S ? N - first : S;
        Plan p;
        if (!gru_plan(n, H, cu_count, &p)) return TK_ERR_UNSUPPORTED;
        const size_t need = gru_ws_bytes(H, p, backward);
        if (wsb < (need ? need : 16)) return TK_ERR_WORKSPACE;
        if (T == 0) continue;
        if (need) {
            int rc = zero_ws(ws, need, stream);
            if (rc != TK_OK) return rc;
        }
        const int rc = launch(p, first, make_cols(n, N));
        if (rc != TK_OK) return rc;
    }
    return TK_OK;
}

// Never 0 where the kernels run (0 means "does not run here"): one granule pair at G = 1, which needs none.
size_t workspace_bytes(size_t N, size_t H, int cu_count, bool backward) {
    Plan p;
    if (!gru_plan(N, H, cu_count, &p)) return 0;
    const size_t need = gru_ws_bytes(H, p, backward);
    return need ? need : 16;
}

// The forward and the backward of every dispatcher below: `checked`, whose launch of a slab takes the tensors, and
// `lengths`, advanced to the slab's first column.  `saved`: gates and q are required (the plain forward takes NULL for
// them at run time; not SAVE: they are not read).
template <bool VL, bool SAVE>
int forward(bool saved, const float *gx, const float *whh, const float *bhh, const int32_t *lengths, size_t T, size_t N,
            size_t H, int reverse, int cu_count, float *y, float *gates, float *q, void *ws, size_t wsb,
            uint32_t *status, hipStream_t stream) {
    auto launch = [&](const Plan &p, size_t first, Cols cols) {
        return launch_fwd<VL, SAVE>(p, H, stream, at_column(gx, first, 3 * H), whh, bhh, (int)T, cols, reverse,
                                    at_column(y, first, H), at_column(gates, first, 3 * H), at_column(q, first, H),
                                    static_cast<u64 *>(ws), status, at_column(lengths, first, 1));
    };
    return checked(gx && whh && bhh && y && (!saved || (gates && q)), T, N, H, cu_count, ws, wsb, status, stream,
                   false, launch);
}

#ifndef TK_RNN_VARLEN
template <bool VL>
int backward(const float *whh, const float *y, const float *gates, const float *q, const float *dy,
             const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count, float *dgates, float *dq,
             void *ws, size_t wsb, uint32_t *status, hipStream_t stream) {
    auto launch = [&](const Plan &p, size_t first, Cols cols) {
        return launch_bwd<VL>(p, H, stream, whh, at_column(y, first, H), at_column(gates, first, 3 * H),
                              at_column(q, first, H), at_column(dy, first, H), (int)T, cols, reverse,
                              at_column(dgates, first, 3 * H), at_column(dq, first, H), static_cast<u64 *>(ws), status,
                              at_column(lengths, first, 1));
    };
    return checked(whh && y && gates && q && dy && dgates && dq, T, N, H, cu_count, ws, wsb, status, stream, true,
                   launch);
}
#endif

}  // namespace

#ifdef TK_RNN_VARLEN
// The forward-only launch with per-column lengths (include/taiyaki_amd_rnn_varlen.h): the plan, and so the grid and
// the granule buffers, of gru_forward_dispatch at the same (N, H, cu_count).
size_t gru_varlen_workspace_bytes(size_t N, size_t H, int cu_count) { return workspace_bytes(N, H, cu_count, false); }

int gru_forward_varlen_dispatch(const float *gx, const float *whh, const float *bhh, const int32_t *lengths, size_t T,
                                size_t N, size_t H, int reverse, int cu_count, float *y, void *ws, size_t wsb,
                                uint32_t *status, hipStream_t stream) {
    return forward<true, false>(false, gx, whh, bhh, lengths, T, N, H, reverse, cu_count, y, nullptr, nullptr, ws, wsb,
                                status, stream);
}
#elif defined(TK_RNN_VARLEN_TRAIN)
// The training pair with per-column lengths (include/taiyaki_amd_rnn_varlen_train.h): the plans, grids and granule
// buffers of gru_forward_dispatch / gru_backward_dispatch at the same (N, H, cu_count); the workspace is the
// backward's, as tk_gru_workspace_bytes is.
size_t gru_varlen_train_workspace_bytes(size_t N, size_t H, int cu_count) {
    return workspace_bytes(N, H, cu_count, true);
}

int gru_forward_varlen_save_dispatch(const float *gx, const float *whh, const float *bhh, const int32_t *lengths,
                                     size_t T, size_t N, size_t H, int reverse, int cu_count, float *y, float *gates,
                                     float *q, void *ws, size_t wsb, uint32_t *status, hipStream_t stream) {
    return forward<true, true>(true, gx, whh, bhh, lengths, T, N, H, reverse, cu_count, y, gates, q, ws, wsb, status,
                               stream);
}

int gru_backward_varlen_dispatch(const float *whh, const float *y, const float *gates, const float *q,
                                 const float *dy, const int32_t *lengths, size_t T, size_t N, size_t H, int reverse,
                                 int cu_count, float *dgates, float *dq, void *ws, size_t wsb, uint32_t *status,
                                 hipStream_t stream) {
    return backward<true>(whh, y, gates, q, dy, lengths, T, N, H, reverse, cu_count, dgates, dq, ws, wsb, status,
                          stream);
}
#elif defined(TK_RNN_WIDE)
// Every batch width at the sizes the kernels cover (include/taiyaki_amd_rnn_wide.h): the VL forms, on one slab of
// gru_slab columns after the other.  A batch that one launch admits is one slab: the call of the training pair with
// per-column lengths, or of the forward that saves nothing, at the same (N, H, cu_count).
size_t gru_wide_slab(size_t N, size_t H, int cu_count) { return gru_slab(N, H, cu_count); }

// the training pair's workspace at the widest slab, the first
size_t gru_wide_workspace_bytes(size_t N, size_t H, int cu_count) {
    return workspace_bytes(gru_slab(N, H, cu_count), H, cu_count, true);
}

// gates and q may both be NULL: nothing is saved
int gru_forward_wide_dispatch(const float *gx, const float *whh, const float *bhh, const int32_t *lengths, size_t T,
                              size_t N, size_t H, int reverse, int cu_count, float *y, float *gates, float *q, void *ws,
                              size_t wsb, uint32_t *status, hipStream_t stream) {
    if (!gates != !q) return TK_ERR_BAD_ARG;
    return gates ? forward<true, true>(true, gx, whh, bhh, lengths, T, N, H, reverse, cu_count, y, gates, q, ws, wsb,
                                       status, stream)
                 : forward<true, false>(false, gx, whh, bhh, lengths, T, N, H, reverse, cu_count, y, nullptr, nullptr,
                                        ws, wsb, status, stream);
}

int gru_backward_wide_dispatch(const float *whh, const float *y, const float *gates, const float *q, const float *dy,
                               const int32_t *lengths, size_t T, size_t N, size_t H, int reverse, int cu_count,
                               float *dgates, float *dq, void *ws, size_t wsb, uint32_t *status, hipStream_t stream) {
    return backward<true>(whh, y, gates, q, dy, lengths, T, N, H, reverse, cu_count, dgates, dq, ws, wsb, status,
                          stream);
}
#else
size_t gru_workspace_bytes(size_t N, size_t H, int cu_count) { return workspace_bytes(N, H, cu_count, true); }

// gates and q may be NULL: the activations are then not saved
int gru_forward_dispatch(const float *gx, const float *whh, const float *bhh, size_t T, size_t N, size_t H,
                         int reverse, int cu_count, float *y, float *gates, float *q, void *ws, size_t wsb,
                         uint32_t *status, hipStream_t stream) {
    return forward<false, true>(false, gx, whh, bhh, nullptr, T, N, H, reverse, cu_count, y, gates, q, ws, wsb, status,
                                stream);
}

int gru_backward_dispatch(const float *whh, const float *y, const float *gates, const float *q, const float *dy,
                          size_t T, size_t N, size_t H, int reverse, int cu_count, float *dgates, float *dq, void *ws,
                          size_t wsb, uint32_t *status, hipStream_t stream) {
    return backward<false>(whh, y, gates, q, dy, nullptr, T, N, H, reverse, cu_count, dgates, dq, ws, wsb, status,
                           stream);
}

#ifdef TK_LAB
void gru_lab_cols(int cols) { g_lab_cols = cols; }
#endif
#endif  // TK_RNN_VARLEN

}  // namespace tk

// lstm_bwd_layout.h -- the block layout of the LSTM backward's matvec (lstm_kernels.hip, lstm_bwd_kernel): which
// weights of W_hh a lane holds, in which order it adds them, and which sums it publishes.  Plain constexpr arithmetic,
// no device code: the kernel's static_asserts and tests/test_lstm_bwd_layout.py (which compiles this header for the
// host and enumerates it) read the same functions.
//
// A workgroup of NT lanes owns the 4 U gate rows r = gate * U + unit of its U units, all H columns.  Lane
// tid = kb * RQ + rq holds the KQ columns k = KQ * kb + q (q < KQ) of RR owned rows: the row pairs p = rq + RQ * i
// (i < RR / 2), rows 2 p and 2 p + 1, which lie side by side in the [row][column] image of dG in LDS, so a pair is one
// read of 2 C floats and each float of it feeds KQ weights.  The RQ lanes rq of one kb are neighbours in a wave; their
// partial sums meet by recursive halving over xor 1, 2, ... RQ / 2: of its n accumulators, flat index a = q * C + c, a
// lane whose bit of rq is set keeps the upper n / 2 and sends the lower, the other the reverse.  After log2(RQ) rounds
// lane rq holds the KQ * C / RQ accumulators a = kept_first(rq) + v, each the sum over all 4 U rows in the one order
//
//     ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)),   s_rq = the lane's rows in the order row(rq, 0), row(rq, 1), ...
//
// (RQ = 8; floating-point addition commutes, so which lane of a pair keeps a sum does not show in its bits).  Neither
// the rows of a lane nor the tree depend on C: a batch column's sums are the same bits in every launch that takes it.
#pragma once

namespace tk {

// columns of W_hh per lane at (H, U); 0: the instantiation keeps the column layout (one column, R rows in a run)
constexpr int lstm_bwd_kq(int H, int U) { return H == 256 && U == 64 ? 4 : 0; }

struct LstmBwdBlock {
    int NT, H, U, C;          // lanes of the workgroup, hidden size, owned units, batch columns
    int KQ, RQ, RR, KEEP;     // columns per lane, lanes per column block, rows per lane, sums a lane publishes

    constexpr LstmBwdBlock(int nt, int h, int u, int c)
        : NT(nt), H(h), U(u), C(c), KQ(lstm_bwd_kq(h, u)), RQ(KQ ? nt * KQ / h : 0),
          RR(KQ ? 4 * u * h / (nt * KQ) : 0), KEEP(RQ ? KQ * c / RQ : 0) {}

    constexpr bool ok() const {
        return KQ > 0 && KQ * RR * NT == 4 * U * H && RQ * H == NT * KQ && RQ >= 1 && RQ <= 64 &&
               (RQ & (RQ - 1)) == 0 && RR % 2 == 0 && RQ * RR == 4 * U && KEEP >= 1 && KEEP * RQ == KQ * C &&
               KEEP <= C && C % KEEP == 0 && KEEP * NT == C * H;
    }
    // the j-th owned row (j < RR) of lane rq, in the order the lane adds them
    constexpr int row(int rq, int j) const { return 2 * (rq + RQ * (j / 2)) + j % 2; }
    // flat index q * C + c of the first accumulator lane rq holds after the reduction (it holds KEEP in a run: one q,
    // columns c, c + 1, ...)
    constexpr int kept_first(int rq) const {
        int a = 0, n = KQ * C;
        for (int m = 1; m < RQ; m <<= 1) {
            n /= 2;
            if (rq & m) a += n;
        }
        return a;
    }
};

}  // namespace tk

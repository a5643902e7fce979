// lstm_fwd_layout.h -- the lane layout of the LSTM forward's step at H 256, U 64 (lstm_kernels.hip, lstm_fwd_kernel):
// where h_{t-1} lies in LDS, which partial sums a lane is left with after the reduction, and which lane applies which
// gate's function.  Plain constexpr arithmetic, no device code: the kernel's static_asserts and
// tests/test_lstm_fwd_lanes.py (which compiles this header for the host and enumerates it) read the same functions.
//
// A workgroup of NT lanes owns U units and C batch columns.  Lane tid = u * KP + kp holds the 4 gate rows of unit u over
// the columns k = i * KP + kp of W_hh (i < KS), and adds them in the order of i: that is the layout of every forward
// instantiation, and it does not change here.
//
// h in LDS.  PR = 4 / C rows of a lane (C < 4; else 1) lie side by side: value (k, c), k = i * KP + kp, is float
// ((i / PR) * KP + kp) * PR * C + (i % PR) * C + c, so rows PR j ... PR j + PR - 1 of lane kp are ONE aligned 16-byte
// chunk, and the KP lanes kp read KP adjacent chunks (the other lanes of the wave the same KP).  At C = 4 this is the
// plain [k][c] image.
//
// Reduction.  The 4 C accumulators of a lane, flat index a = flat(gate, c), meet those of the other KP - 1 lanes by
// recursive halving over xor 1, 2, ... KP / 2 (lstm_kernels.hip: halve_rounds): of its n remaining accumulators a lane
// whose bit of kp is set keeps the upper n / 2 and sends the lower, the other the reverse.  flat() orders them so that
// the last two rounds halve the gates and the rounds before them the columns: lane kp ends with the CK = 4 C / KP sums
// a = kept_first(kp) + v, which are columns col(kp, v), v < CK, of the ONE gate gate(kp).  Each sum is
//
//     ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)),   p_kp = lane kp's partial sum, its weights in the order of i
//
// (KP = 8; floating-point addition commutes, so which lane of a pair keeps a sum does not show in its bits).  Neither
// the weights of a lane nor the tree depend on C.
//
// Activations.  Lane kp adds its own gx to its CK sums and applies its gate's function, one each at C = 2.  The lanes
// kp ^ 2, kp ^ 4 and kp ^ 6 hold the other three gates of the same columns; the lane of gate 0 (cell_lane) takes them
// through DPP moves and runs the cell update of its CK columns.
#pragma once

namespace tk {

// the instantiation that takes this layout; every other (H, U, C) keeps the plain [k][c] image, the shuffles and the
// cell update in the lanes kp < C.  (256, 64, 4) too: there a lane has two activations and the cell lane two columns,
// it gave the same bits and measured 3.41-3.43 us per step against the plain body's 2.90-2.93
// (profiles/r36_lstm_fwd_lanes.txt): the arithmetic below holds at C = 4, and the kernel does not take it there.
constexpr bool lstm_fwd_lanes(int H, int U, int C) { return H == 256 && U == 64 && C == 2; }

struct LstmFwdLanes {
    int NT, H, U, C;          // lanes of the workgroup, hidden size, owned units, batch columns
    int KP, KS, PR, CK;       // lanes per unit, weights per lane and gate, rows of h per 16-byte read, columns a lane keeps

    constexpr LstmFwdLanes(int nt, int h, int u, int c)
        : NT(nt), H(h), U(u), C(c), KP(nt / u), KS(h * u / nt), PR(c < 4 ? 4 / c : 1), CK(4 * c * u / nt) {}

    constexpr bool ok() const {
        return KP * U == NT && KS * KP == H && KP >= 4 && KP <= 64 && (KP & (KP - 1)) == 0 && PR >= 1 &&
               (PR * C) % 4 == 0 && KS % PR == 0 && CK >= 1 && CK * KP == 4 * C && C % CK == 0;
    }
    // the column of W_hh of lane kp's i-th weight (of each of its four gate rows)
    constexpr int k(int kp, int i) const { return i * KP + kp; }
    // the float of the h image that holds h[k] of column c
    constexpr int hs_index(int k_, int c) const {
        return ((k_ / KP / PR) * KP + k_ % KP) * PR * C + (k_ / KP % PR) * C + c;
    }
    // the first float of lane kp's j-th read (j < KS / PR): rows i = PR j ... PR j + PR - 1, C floats each
    constexpr int chunk(int kp, int j) const { return (j * KP + kp) * PR * C; }
    // the flat index of accumulator (gate, c) in the array the rounds halve
    constexpr int flat(int gate, int c) const { return (c / CK) * 4 * CK + gate * CK + c % CK; }
    // the flat index of the first of the CK sums lane kp is left with
    constexpr int kept_first(int kp) const {
        int a = 0, n = 4 * C;
        for (int m = 1; m < KP; m <<= 1) {
            n /= 2;
            if (kp & m) a += n;
        }
        return a;
    }
    constexpr int gate(int kp) const { return kept_first(kp) % (4 * CK) / CK; }
    constexpr int col(int kp, int v) const { return kept_first(kp) / (4 * CK) * CK + v; }
    constexpr bool cell_lane(int kp) const { return gate(kp) == 0; }
    // the lane, as an xor of kp, that holds gate g of the cell lane's columns
    constexpr int gate_lane_xor(int g) const {
        for (int x = 0; x < KP; ++x)
            if (gate(x) == g && col(x, 0) == 0) return x;
        return -1;
    }
};

}  // namespace tk

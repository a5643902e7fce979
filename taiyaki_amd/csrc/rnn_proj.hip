// rnn_proj.hip -- a recurrent layer's two projection GEMMs, out = a B^T (+ bias) with B the layer's w_ih or its
// transpose, on the bf16 matrix cores, every float32 operand split into three bf16 parts
// (include/taiyaki_amd_rnn_proj.h; libtaiyaki_amd_rnn_proj.so).  The split and the six products are those of
// wgrad_common.h (split2, the order of the products, two accumulator sets); the layout differs because k is innermost in
// both operands here: an operand fragment of v_mfma_f32_32x32x16_bf16 is then 8 consecutive k of one row, a plain
// 16-byte LDS read, and no transposed read is needed.
//
// Two launches.  proj_prep_kernel writes the three bf16 parts of B (nout x k; for the input gradient B[n][k] =
// w_ih[k][n]) into the workspace as [column tile][k block][part][32 columns][lane][16 bytes]: exactly the bytes, in
// their order, of the MFMA operand fragments of one k block (a fragment = 64 lanes x 16 bytes), zeros beyond nout.
// proj_kernel: a workgroup of four waves owns a PJ_RT x PJ_NT = 128 x 128 output tile (each wave 64 x 64: 2 x 2
// accumulators of 32 x 32, twice) and walks k in blocks of PJ_KB = 16, one MFMA step.  Per block every thread loads
// two float4 of `a`; after the block's MFMAs it splits the float4s of the NEXT block and writes 8 bytes into each of
// the three images of `a` in the other LDS buffer; the block after that is already on its way from memory (two
// register sets).  The weights do not pass through LDS: each wave loads its six B fragments of the next block from
// the workspace (L2) straight into the registers the MFMAs read, one coalesced 1 KB load each, one block ahead (two
// register sets); the prep launch precedes this one on the stream, so they are plain loads.  One barrier per block.
// With 27 KB of LDS and at most 256 registers two workgroups share a CU: two waves per SIMD, so one's split, loads and
// final stores run beside the other's MFMAs.
// LDS images: a fragment (32 rows x 16 k) is 64 lanes x 16 bytes, lane = row + 32 (k / 8), read as one ds_read_b128 per
// lane, linear in the lane (conflict-free).  In the images of `a` the two halves of a fragment are 576 bytes apart: the
// 16 lanes of one ds_write_b64 group (4 rows x 4 float4) then cover a whole 128-byte bank row once.
// k order: blocks ascending, one chain per accumulator set, (leading + corrections) + bias at the end.  Nothing depends
// on the row's position or on rows: a row's bits are a function of that row and of B alone.
// blockIdx = (row tile / 8) (8 column tiles) + column tile 8 + row tile % 8: the column tiles of one row tile follow
// one another on one XCD, so `a` comes from HBM once and from that XCD's L2 afterwards.
#include "wgrad_common.h"

#include "../../include/taiyaki_amd_rnn_proj.h"

namespace tk {
namespace {

constexpr int PJ_RT = 128;          // output tile: rows ...
constexpr int PJ_NT = 128;          // ... and columns
constexpr int PJ_KB = 16;           // k per staged block: one MFMA step
constexpr int PJ_THREADS = 256;     // four waves, 2 x 2, two workgroups per CU: two waves per SIMD
constexpr int PJ_A_HALF = 576;      // images of `a`: bytes from k 0-7 to k 8-15 of a fragment,
constexpr int PJ_A_MB = 2 * PJ_A_HALF;              // from one block of 32 rows to the next,
constexpr int PJ_A_PART = (PJ_RT / 32) * PJ_A_MB;   // and of one part
constexpr int PJ_A_PASSES = PJ_RT * (PJ_KB / 4) / PJ_THREADS;   // float4s of `a` per thread and block
constexpr int PJ_B_PART = (PJ_NT / 32) * 1024;      // images of B: one part of one block,
constexpr int PJ_B_BLOCK = 3 * PJ_B_PART;           // one block
static_assert(PJ_A_PASSES * PJ_THREADS == PJ_RT * (PJ_KB / 4), "the block of `a` is staged in whole passes");

// The gradient form (k > nout: a long k walked by few workgroups) was measured slower than rocBLAS at 15 and 1600 rows
// and faster at 64000 and 102400 (profiles/r31_lstmbench.txt): tk_rnn_proj_workspace_bytes admits it from here on
constexpr size_t PJ_GRAD_MIN_ROWS = 64000;

struct ProjPlan {
    int tiles_m, tiles_n, nkb, grid;
    size_t bytes;
};

bool proj_width_ok(size_t lo, size_t hi) {
    const bool known = lo == 16 || lo == 32 || lo == 64 || lo == 96 || lo == 128 || lo == 192 || lo == 256 || lo == 384;
    return known && (hi == 3 * lo || hi == 4 * lo);
}

// The plan: a function of the shape only (cu_count is part of the signature for the neighbours' sake).  Every admitted
// k is a multiple of PJ_KB: no block is ragged in k.
bool proj_plan(size_t rows, size_t k, size_t nout, int cu_count, ProjPlan *p) {
    if (rows == 0 || k == 0 || nout == 0 || cu_count <= 0) return false;
    if (!proj_width_ok(k < nout ? k : nout, k < nout ? nout : k)) return false;
    if (rows >= (size_t(1) << 31) / (k < nout ? nout : k)) return false;
    const size_t tm = ceil_div(rows, PJ_RT), tn = ceil_div(nout, PJ_NT), nkb = k / PJ_KB;
    p->tiles_m = (int)tm, p->tiles_n = (int)tn, p->nkb = (int)nkb;
    p->grid = (int)(ceil_div(tm, 8) * 8 * tn);
    p->bytes = tn * nkb * PJ_B_BLOCK;
    return true;
}

// where the caller should run the kernel: where it runs (proj_plan) and was not measured slower than the GEMM
bool proj_admitted(size_t rows, size_t k, size_t nout, int cu_count, ProjPlan *p) {
    return proj_plan(rows, k, nout, cu_count, p) && (k < nout || rows >= PJ_GRAD_MIN_ROWS);
}

// the three bf16 parts of B, one 16-byte piece (8 consecutive k of one column n) per thread and part
__global__ __launch_bounds__(256) void proj_prep_kernel(const float *w, unsigned char *img, int K, int N, int nkb,
                                                        int transposed, unsigned pieces) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= pieces) return;
    const int lane = idx & 63, nb = (idx >> 6) & 3, blk = idx >> 8;     // blk = column tile * nkb + k block
    const int n = (blk / nkb) * PJ_NT + nb * 32 + (lane & 31);
    const int k0 = (blk % nkb) * PJ_KB + 8 * (lane >> 5);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        v[e] = 0.f;
        if (n < N) v[e] = transposed ? w[(size_t)k * N + n] : w[(size_t)n * K + k];
    }
    uint4 p1, p2, p3;
    split2(v[0], v[1], p1.x, p2.x, p3.x);
    split2(v[2], v[3], p1.y, p2.y, p3.y);
    split2(v[4], v[5], p1.z, p2.z, p3.z);
    split2(v[6], v[7], p1.w, p2.w, p3.w);
    unsigned char *at = img + (size_t)blk * PJ_B_BLOCK + (size_t)(idx & 255) * 16;
    *reinterpret_cast<uint4 *>(at) = p1;
    *reinterpret_cast<uint4 *>(at + PJ_B_PART) = p2;
    *reinterpret_cast<uint4 *>(at + 2 * PJ_B_PART) = p3;
}

struct ProjArgs {
    const float *a;
    const unsigned char *bimg;
    const float *bias;
    float *out;
    int M, K, N;
    int tiles_m, tiles_n, nkb;
};

// WIDE: `a` is 16-byte aligned (K is a multiple of 4 by the rule) and takes float4 loads
template <bool WIDE>
__global__ __launch_bounds__(PJ_THREADS, 2) void proj_kernel(const ProjArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char imga[2][3 * PJ_A_PART];   // [buffer][part]

    const float *asrc = p.a;
    const int M = p.M, K = p.K, nkb = p.nkb;
    const int grp = blockIdx.x / (8 * p.tiles_n), rem = blockIdx.x % (8 * p.tiles_n);
    const int nt = rem >> 3, mt = grp * 8 + (rem & 7);
    if (mt >= p.tiles_m) return;        // (the padding of the last group of eight)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhalf = lane >> 5;
    const int wmb = (wave >> 1) * 2, wnb = (wave & 1) * 2;      // the wave's first block of 32 rows / of 32 columns

    // staging `a`: float4 q of the block's four in row r + 64 j of the tile
    const int q = tid & 3, r = tid >> 2;
    const int awoff = (r >> 5) * PJ_A_MB + (q >> 1) * PJ_A_HALF + (r & 31) * 16 + 8 * (q & 1);
    const int m_first = mt * PJ_RT + r;
    // operand fragments: those of `a` from LDS, those of B from the workspace, where fragment (32-column block, part) of
    // a block is 64 lanes x 16 consecutive bytes
    const int aroff = wmb * PJ_A_MB + lhalf * PJ_A_HALF + l31 * 16;
    const unsigned char *bsrc = p.bimg + (size_t)nt * nkb * PJ_B_BLOCK + (wnb * 64 + lane) * 16;

    f32x16 acc[WG_ACC_SETS][2][2];
#pragma unroll
    for (int s = 0; s < WG_ACC_SETS; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[s][i][j][e] = 0.f;

    // two blocks of `a` are in flight from memory: block kb + 2 is requested before the MFMAs of block kb, block kb + 1
    // is split and written to the other LDS buffer after them.  The wave's six fragments of B (2 column blocks x 3
    // parts) of block kb + 1 are requested before the MFMAs of block kb as well, into the register set the MFMAs of
    // block kb - 1 read
    float4 ra[2][PJ_A_PASSES];
    bool oka[2][PJ_A_PASSES];
    bf16x8 fb[2][2][3];

    // a block past the end is fetched as zeros of `a` (element 0 where the loads are unguarded) and staged but never
    // multiplied; of B the last block is fetched again (the workspace ends with it) and never multiplied either
    auto fetch = [&](int kb, int set) {
        const int k = kb * PJ_KB + 4 * q;
        const bool kok = kb < nkb;
#pragma unroll
        for (int j = 0; j < PJ_A_PASSES; ++j) {
            const int m = m_first + 64 * j;
            oka[set][j] = m < M && kok;
            if (WIDE)
                ra[set][j] = load4<true>(asrc, K, m, oka[set][j], oka[set][j] ? k : 0);
            else
                ra[set][j] = load4<false>(asrc, K, m, oka[set][j], k);
        }
    };
    auto fetchb = [&](int kb, int set) {
        const unsigned char *at = bsrc + (size_t)(kb < nkb ? kb : nkb - 1) * PJ_B_BLOCK;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < 3; ++t)
                fb[set][i][t] = *reinterpret_cast<const bf16x8 *>(at + t * PJ_B_PART + i * 1024);
    };
    auto stash = [&](int set, int buf) {
#pragma unroll
        for (int j = 0; j < PJ_A_PASSES; ++j) {
            float4 v = ra[set][j];
            if (!oka[set][j]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            uint2 p1, p2, p3;
            split2(v.x, v.y, p1.x, p2.x, p3.x);
            split2(v.z, v.w, p1.y, p2.y, p3.y);
            unsigned char *at = &imga[buf][awoff + 2 * j * PJ_A_MB];
            *reinterpret_cast<uint2 *>(at) = p1;
            *reinterpret_cast<uint2 *>(at + PJ_A_PART) = p2;
            *reinterpret_cast<uint2 *>(at + 2 * PJ_A_PART) = p3;
        }
    };

    // the bias is loaded ahead of the loop, whose waits cover it.  Loaded in the epilogue, inside a branch, it left a
    // pending load at every join of the guarded stores, and a wait for it waits for the stores issued so far as well
    // (one counter for both): each store then waited for the one before it to reach L2
    float bias[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = nt * PJ_NT + (wnb + j) * 32 + l31;
        bias[j] = (p.bias && n < p.N) ? p.bias[n] : 0.f;
    }

    fetch(0, 0);
    fetchb(0, 0);
    fetch(1, 1);
    stash(0, 0);
    __syncthreads();
    for (int kb2 = 0; kb2 < nkb; kb2 += 2) {
#pragma unroll
        for (int cur = 0; cur < 2; ++cur) {     // block kb is in LDS buffer kb & 1 and came through register set kb & 1
            const int kb = kb2 + cur;
            if (kb >= nkb) break;
            fetch(kb + 2, cur);
            fetchb(kb + 1, cur ^ 1);
            bf16x8 fa[2][3];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    fa[i][t] = *reinterpret_cast<const bf16x8 *>(&imga[cur][t * PJ_A_PART + i * PJ_A_MB + aroff]);
            // a1 b1, then the corrections, the smallest first
            constexpr int PA[6] = {0, 2, 0, 1, 1, 0}, PB[6] = {0, 0, 2, 1, 0, 1};
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int set = t > 0 ? WG_ACC_SETS - 1 : 0;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[set][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][PA[t]], fb[cur][j][PB[t]],
                                                                                  acc[set][i][j], 0, 0, 0);
            }
            stash(cur ^ 1, cur ^ 1);    // (its last readers passed the barrier of block kb - 1)
            __syncthreads();
        }
    }

    // C[m][n] of accumulator register e sits at row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = nt * PJ_NT + (wnb + j) * 32 + l31;
        const bool nok = n < p.N;
        const float b = bias[j];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = mt * PJ_RT + (wmb + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
                const float v = WG_ACC_SETS == 2 ? acc[0][i][j][e] + acc[WG_ACC_SETS - 1][i][j][e] : acc[0][i][j][e];
                if (nok && m < p.M) p.out[(size_t)m * p.N + n] = p.bias ? v + b : v;
            }
    }
}

}  // namespace

size_t rnn_proj_workspace_bytes(size_t rows, size_t k, size_t nout, int cu_count) {
    ProjPlan p;
    return proj_admitted(rows, k, nout, cu_count, &p) ? p.bytes : 0;
}

// out (rows, nout) = a (rows, k) B^T + bias, B (nout, k) = w (transposed == 0) or its transpose, w then (k, nout)
int rnn_proj_dispatch(const float *a, const float *w, const float *bias, int transposed, size_t rows, size_t k,
                      size_t nout, int cu_count, float *out, void *ws, size_t wsb, hipStream_t stream) {
    if (!a || !w || !out || !ws || !aligned16(ws)) return TK_ERR_BAD_ARG;
    ProjPlan p;
    if (!proj_plan(rows, k, nout, cu_count, &p)) return TK_ERR_UNSUPPORTED;
    if (wsb < p.bytes) return TK_ERR_WORKSPACE;
    const unsigned pieces = (unsigned)(p.bytes / PJ_B_BLOCK) * (PJ_B_PART / 16);
    hipLaunchKernelGGL(proj_prep_kernel, dim3((pieces + 255) / 256), dim3(256), 0, stream, w,
                       static_cast<unsigned char *>(ws), (int)k, (int)nout, p.nkb, transposed, pieces);
    if (hipGetLastError() != hipSuccess) return TK_ERR_LAUNCH;
    ProjArgs g;
    g.a = a, g.bimg = static_cast<const unsigned char *>(ws), g.bias = bias, g.out = out;
    g.M = (int)rows, g.K = (int)k, g.N = (int)nout;
    g.tiles_m = p.tiles_m, g.tiles_n = p.tiles_n, g.nkb = p.nkb;
    if (aligned16(a))
        hipLaunchKernelGGL(proj_kernel<true>, dim3(p.grid), dim3(PJ_THREADS), 0, stream, g);
    else
        hipLaunchKernelGGL(proj_kernel<false>, dim3(p.grid), dim3(PJ_THREADS), 0, stream, g);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // namespace tk

extern "C" {

size_t tk_rnn_proj_workspace_bytes(size_t rows, size_t k, size_t nout, int cu_count) {
    return tk::rnn_proj_workspace_bytes(rows, k, nout, cu_count);
}

int tk_rnn_input_proj_dev(const float *x, const float *w_ih, const float *bias, size_t rows, size_t insize,
                          size_t gates_size, int cu_count, float *gx, void *workspace, size_t workspace_bytes,
                          void *stream) {
    return tk::rnn_proj_dispatch(x, w_ih, bias, 0, rows, insize, gates_size, cu_count, gx, workspace, workspace_bytes,
                                 static_cast<hipStream_t>(stream));
}

int tk_rnn_input_grad_dev(const float *dgates, const float *w_ih, size_t rows, size_t insize, size_t gates_size,
                          int cu_count, float *dx, void *workspace, size_t workspace_bytes, void *stream) {
    return tk::rnn_proj_dispatch(dgates, w_ih, nullptr, 1, rows, gates_size, insize, cu_count, dx, workspace,
                                 workspace_bytes, static_cast<hipStream_t>(stream));
}

#ifdef TK_LAB
int tk_lab_rnn_proj_plan(size_t rows, size_t k, size_t nout, int cu_count, size_t *out) {
    tk::ProjPlan p;
    if (!tk::proj_admitted(rows, k, nout, cu_count, &p)) return 0;
    const size_t v[6] = {(size_t)tk::PJ_RT, (size_t)tk::PJ_NT, (size_t)p.tiles_m, (size_t)p.tiles_n, (size_t)p.nkb,
                         (size_t)p.grid};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
    return 1;
}
#endif

}  // extern "C"

// beam_kernels.hip -- hash beam search over the flip-flop lattice for gfx950.
//
// Replaces taiyaki/decodeutil/c_hashdecode.c:346-507 (`flipflop_beamsearch`), its guiding
// backward pass c_flipflopfwdbwd.c:55-91 and the wrapper decodeutil.pyx:9-51.
//
// One wavefront per read; the beam (<= 12 elements for the 4-base alphabet; the reference's
// default is 5) lives in lanes 0..W-1 (hash, score, last state), a block's candidate records
// -- W x nbase extensions, then W stays -- one per lane.  What the reference does with two
// quicksorts per block is done without sorting:
//   * merge by hash: a record has at most ONE partner with the same hash (the stay of prefix
//     s and the extension of s[:-1] by its last base); every lane compares its hash with the
//     other candidates' (v_readlane sweep), the later one folds into the earlier one with the
//     reference's logsumexpf;
//   * top-k by score: rank = number of records that beat this one; rank r < width becomes beam
//     element r.  The order of records with EXACTLY equal scores is, in the reference, whatever
//     its quicksort (qsort.h) leaves, and it decides who stays in the beam; such ties turn up in
//     about one block in a hundred.  A block that has one is redone the reference's way: the
//     records are laid out in hash order (ranked in parallel) and lane 0 runs the reference's
//     sort procedure on them (`beam_qsort`), so the beam follows the reference through ties too.
// Sequences are never copied: every block stores one byte per beam element (parent slot,
// appended state) and the best element's sequence is walked back at the end (through LDS when
// the table fits).  The running beam cut (`beam_cut` > 0) is the reference's: a record is
// dropped if it is worse than the best seen BEFORE it by more than log(beam_cut) -- an exclusive
// prefix maximum in candidate order.
// expf / log1pf of the reference's logsumexpf are evaluated in double and rounded to float
// (correctly rounded results, what glibc's float functions return in all but rare cases), so
// scores agree with the reference to the last bit almost everywhere and the beam takes the
// same decisions.
#include "ff_common.h"

// The tables of the log-sum-exp below: ONE copy, here.  basecall_beam.hip (the other library's instantiation of the
// search) includes this file with TK_BEAM_TABLES_ONLY for them, then beam_search.h.
namespace tk {

// The reference's logsumexpf (c_hashdecode.c:50-54) is  max + log1pf(expf(-|x - y|)):  two float
// functions, each rounded to float.  Both are evaluated in double to better than 2^-52 of the result and
// rounded once -- on every third float in [0, 17) (366 M arguments) the pair gives bit for bit what
// glibc's double exp / log1p give -- by TABLE-driven reductions, because what a block of the search
// costs is the length of the DEPENDENT double-precision chain (a half-rate fma every ~40 cycles for a
// lone wave): ocml's generic exp + log1p were ~165 instructions per log-sum-exp, a table-free
// Taylor / atanh form ~50 dependent operations, this one ~24.
//   expf(-a):  n = rint(-a 32 / ln 2), r = -a - n ln2/32 (two-part constant), |r| <= 0.0109:
//              2^(n >> 5) * EXP2[n & 31] * (1 + r + ... + r^6 / 720)
//   log1pf(e): t = 1 + e (exact in double), i = rint(64 (t - 1)), c = 1 + i / 64, r = t / c - 1
//              (|r| <= 1 / 128):  LOGC[i] + r - r^2 / 2 + ... + r^7 / 7
// (degree 5 for the exponential mis-rounds 2 of those 366 M arguments; these degrees none)
constexpr int TAB_EXP2 = 0, TAB_INVC = 32, TAB_LOGC = 97, TAB_N = 162;
__constant__ double BEAM_TAB[TAB_N] = {
    0x1.0000000000000p+0, 0x1.059b0d3158574p+0, 0x1.0b5586cf9890fp+0, 0x1.11301d0125b51p+0,
    0x1.172b83c7d517bp+0, 0x1.1d4873168b9aap+0, 0x1.2387a6e756238p+0, 0x1.29e9df51fdee1p+0,
    0x1.306fe0a31b715p+0, 0x1.371a7373aa9cbp+0, 0x1.3dea64c123422p+0, 0x1.44e086061892dp+0,
    0x1.4bfdad5362a27p+0, 0x1.5342b569d4f82p+0, 0x1.5ab07dd485429p+0, 0x1.6247eb03a5585p+0,
    0x1.6a09e667f3bcdp+0, 0x1.71f75e8ec5f74p+0, 0x1.7a11473eb0187p+0, 0x1.82589994cce13p+0,
    0x1.8ace5422aa0dbp+0, 0x1.93737b0cdc5e5p+0, 0x1.9c49182a3f090p+0, 0x1.a5503b23e255dp+0,
    0x1.ae89f995ad3adp+0, 0x1.b7f76f2fb5e47p+0, 0x1.c199bdd85529cp+0, 0x1.cb720dcef9069p+0,
    0x1.d5818dcfba487p+0, 0x1.dfc97337b9b5fp+0, 0x1.ea4afa2a490dap+0, 0x1.f50765b6e4540p+0,
    0x1.0000000000000p+0, 0x1.f81f81f81f820p-1, 0x1.f07c1f07c1f08p-1, 0x1.e9131abf0b767p-1,
    0x1.e1e1e1e1e1e1ep-1, 0x1.dae6076b981dbp-1, 0x1.d41d41d41d41dp-1, 0x1.cd85689039b0bp-1,
    0x1.c71c71c71c71cp-1, 0x1.c0e070381c0e0p-1, 0x1.bacf914c1bad0p-1, 0x1.b4e81b4e81b4fp-1,
    0x1.af286bca1af28p-1, 0x1.a98ef606a63bep-1, 0x1.a41a41a41a41ap-1, 0x1.9ec8e951033d9p-1,
    0x1.999999999999ap-1, 0x1.948b0fcd6e9e0p-1, 0x1.8f9c18f9c18fap-1, 0x1.8acb90f6bf3aap-1,
    0x1.8618618618618p-1, 0x1.8181818181818p-1, 0x1.7d05f417d05f4p-1, 0x1.78a4c8178a4c8p-1,
    0x1.745d1745d1746p-1, 0x1.702e05c0b8170p-1, 0x1.6c16c16c16c17p-1, 0x1.6816816816817p-1,
    0x1.642c8590b2164p-1, 0x1.6058160581606p-1, 0x1.5c9882b931057p-1, 0x1.58ed2308158edp-1,
    0x1.5555555555555p-1, 0x1.51d07eae2f815p-1, 0x1.4e5e0a72f0539p-1, 0x1.4afd6a052bf5bp-1,
    0x1.47ae147ae147bp-1, 0x1.446f86562d9fbp-1, 0x1.4141414141414p-1, 0x1.3e22cbce4a902p-1,
    0x1.3b13b13b13b14p-1, 0x1.3813813813814p-1, 0x1.3521cfb2b78c1p-1, 0x1.323e34a2b10bfp-1,
    0x1.2f684bda12f68p-1, 0x1.2c9fb4d812ca0p-1, 0x1.29e4129e4129ep-1, 0x1.27350b8812735p-1,
    0x1.2492492492492p-1, 0x1.21fb78121fb78p-1, 0x1.1f7047dc11f70p-1, 0x1.1cf06ada2811dp-1,
    0x1.1a7b9611a7b96p-1, 0x1.1811811811812p-1, 0x1.15b1e5f75270dp-1, 0x1.135c81135c811p-1,
    0x1.1111111111111p-1, 0x1.0ecf56be69c90p-1, 0x1.0c9714fbcda3bp-1, 0x1.0a6810a6810a7p-1,
    0x1.0842108421084p-1, 0x1.0624dd2f1a9fcp-1, 0x1.0410410410410p-1, 0x1.0204081020408p-1,
    0x1.0000000000000p-1, 0x0.0p+0, 0x1.fc0a8b0fc03e4p-7, 0x1.f829b0e783300p-6,
    0x1.77458f632dcfcp-5, 0x1.f0a30c01162a6p-5, 0x1.341d7961bd1d1p-4, 0x1.6f0d28ae56b4cp-4,
    0x1.a926d3a4ad563p-4, 0x1.e27076e2af2e6p-4, 0x1.0d77e7cd08e59p-3, 0x1.29552f81ff523p-3,
    0x1.44d2b6ccb7d1ep-3, 0x1.5ff3070a793d4p-3, 0x1.7ab890210d909p-3, 0x1.9525a9cf456b4p-3,
    0x1.af3c94e80bff3p-3, 0x1.c8ff7c79a9a22p-3, 0x1.e27076e2af2e6p-3, 0x1.fb9186d5e3e2bp-3,
    0x1.0a324e27390e3p-2, 0x1.1675cababa60ep-2, 0x1.22941fbcf7966p-2, 0x1.2e8e2bae11d31p-2,
    0x1.3a64c556945eap-2, 0x1.4618bc21c5ec2p-2, 0x1.51aad872df82dp-2, 0x1.5d1bdbf5809cap-2,
    0x1.686c81e9b14afp-2, 0x1.739d7f6bbd007p-2, 0x1.7eaf83b82afc3p-2, 0x1.89a3386c1425bp-2,
    0x1.947941c2116fbp-2, 0x1.9f323ecbf984cp-2, 0x1.a9cec9a9a084ap-2, 0x1.b44f77bcc8f63p-2,
    0x1.beb4d9da71b7cp-2, 0x1.c8ff7c79a9a22p-2, 0x1.d32fe7e00ebd5p-2, 0x1.dd46a04c1c4a1p-2,
    0x1.e744261d68788p-2, 0x1.f128f5faf06edp-2, 0x1.faf588f78f31fp-2, 0x1.02552a5a5d0ffp-1,
    0x1.0723e5c1cdf40p-1, 0x1.0be72e4252a83p-1, 0x1.109f39e2d4c97p-1, 0x1.154c3d2f4d5eap-1,
    0x1.19ee6b467c96fp-1, 0x1.1e85f5e7040d0p-1, 0x1.23130d7bebf43p-1, 0x1.2795e1289b11bp-1,
    0x1.2c0e9ed448e8cp-1, 0x1.307d7334f10bep-1, 0x1.34e289d9ce1d3p-1, 0x1.393e0d3562a1ap-1,
    0x1.3d9026a7156fbp-1, 0x1.41d8fe84672aep-1, 0x1.4618bc21c5ec2p-1, 0x1.4a4f85db03ebbp-1,
    0x1.4e7d811b75bb1p-1, 0x1.52a2d265bc5abp-1, 0x1.56bf9d5b3f399p-1, 0x1.5ad404c359f2dp-1,
    0x1.5ee02a9241675p-1, 0x1.62e42fefa39efp-1,
};
constexpr double LN2_32_HI = 0x1.62e42fefa3000p-6, LN2_32_LO = 0x1.3de6af278ece6p-47, INV_LN2_32 = 0x1.71547652b82fep+5;

}  // namespace tk
#define TK_BEAM_TABLES_DEFINED
// tables into LDS, beam_lse, the sort procedure and the kernel body: beam_search.h
#ifndef TK_BEAM_TABLES_ONLY
#include "beam_search.h"
#include "dispatch.h"

namespace tk {

// ---------------------------------------------------------------------------------------------
// The single-read lattice passes of the decoder on their own: flipflop_forward / flipflop_backward
// (c_flipflopfwdbwd.c:55-152) with the wrappers' optional initial vector (decodeutil.pyx:54-108).
// One wavefront per read, lane = state; every log-sum-exp in the reference's order, so the
// matrices agree with the reference's to the rounding of expf / log1pf.
//   out (N, T + 1, 2 nbase); total (N) = logsumexp over the last (forward) / first (backward) row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void lattice_kernel(const float *__restrict__ scores, int T, int N, int nb,
                                                       int forward, const float *__restrict__ init,
                                                       float *__restrict__ out, float *__restrict__ total) {
    __shared__ double tab[TAB_N];
    const int n = blockIdx.x, lane = threadIdx.x;
    beam_load_tables(tab, lane);
    const int ns = 2 * nb, S = ns * (nb + 1);
    const size_t rowstride = (size_t)N * S;
    const float *sc = scores + (size_t)n * S;
    float *mat = out + (size_t)n * (T + 1) * ns;
    const int col = min(lane, S - 1), st = min(lane, ns - 1);
    float p = (init != nullptr) ? init[(size_t)n * ns + st] : 0.f;
    if (forward) {
        if (lane < ns) mat[lane] = p;
        for (int blk = 0; blk < T; ++blk) {
            const float row = sc[(size_t)blk * rowstride + col];
            // every lane runs both recurrences (ds_bpermute returns 0 for a source lane that is
            // masked off, so the gathers must not sit in divergent code) and keeps its own
            const int b = st % nb;
            // to the flop of base b: from its flip, then from itself (:129-134)
            const float cflop = beam_lse(bpf(row, ns * nb + b) + bpf(p, b), bpf(row, ns * nb + b + nb) + bpf(p, b + nb), tab);
            // to the flip of base b: from every state, in order (:136-143)
            float cflip = bpf(row, b * ns) + rdl(p, 0);
            for (int fr = 1; fr < ns; ++fr) cflip = beam_lse(cflip, bpf(row, b * ns + fr) + rdl(p, fr), tab);
            const float c = (st >= nb) ? cflop : cflip;
            p = c;
            if (lane < ns) mat[(size_t)(blk + 1) * ns + lane] = c;
        }
    } else {
        if (lane < ns) mat[(size_t)T * ns + lane] = p;
        for (int blk = T; blk > 0; --blk) {
            const float row = sc[(size_t)(blk - 1) * rowstride + col];
            float c = bpf(row, ns * nb + st) + bpf(p, nb + st % nb);
            for (int to = 0; to < nb; ++to) c = beam_lse(c, bpf(row, to * ns + st) + rdl(p, to), tab);
            p = c;
            if (lane < ns) mat[(size_t)(blk - 1) * ns + lane] = c;
        }
    }
    float tot = rdl(p, 0);
    for (int i = 1; i < ns; ++i) tot = beam_lse(tot, rdl(p, i), tab);
    if (lane == 0) total[n] = tot;
}

int lattice_dispatch(const float *scores, size_t T, size_t N, size_t nbase, int forward, const float *init,
                     float *out, float *total, hipStream_t stream) {
    if (nbase < 1 || nbase > 4) return 2;
    if (N == 0) return 0;
    hipLaunchKernelGGL(lattice_kernel, dim3((unsigned)N), dim3(WAVE), 0, stream, scores, (int)T, (int)N, (int)nbase,
                       forward, init, out, total);
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

size_t beam_workspace_bytes(size_t T, size_t N, size_t nbase) {
    return N * (T + 1) * 2 * nbase * sizeof(float) + N * T * 16 + 512;
}

int beam_dispatch(const float *scores, size_t T, size_t N, size_t nbase, int width, float beam_cut, int guided,
                  signed char *seq, int *seqlen, float *score, void *workspace, size_t workspace_bytes,
                  hipStream_t stream) {
    if (const int rc = beam_admit(nbase, width, beam_cut)) return rc;
    if (workspace_bytes < beam_workspace_bytes(T, N, nbase)) return 3;
    BeamArgs a;
    a.scores = scores;
    a.T = (int)T;
    a.N = (int)N;
    a.nbase = (int)nbase;
    a.width = width;
    a.logcut = beam_logcut(beam_cut);
    a.guided = guided;
    const size_t bwd_bytes = (N * (T + 1) * 2 * nbase * sizeof(float) + 255) / 256 * 256;
    a.bwd = static_cast<float *>(workspace);
    a.bp = reinterpret_cast<unsigned char *>(static_cast<char *>(workspace) + bwd_bytes);
    a.seq = seq;
    a.seqlen = seqlen;
    a.score = score;
    a.lds_rows = (int)(T <= BEAM_LDS_ROWS ? T : BEAM_LDS_ROWS);
    if (nbase == 4)
        hipLaunchKernelGGL((beam_kernel<4, BeamArgs>), dim3((unsigned)N), dim3(WAVE), (size_t)a.lds_rows * 16, stream, a);
    else
        hipLaunchKernelGGL((beam_kernel<0, BeamArgs>), dim3((unsigned)N), dim3(WAVE), (size_t)a.lds_rows * 16, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

}  // namespace tk
#endif  // TK_BEAM_TABLES_ONLY

// basecall_beam.hip -- the hash beam search for the reads of a basecalling batch: reads of different lengths, their
// stitched scores packed row after row, ONE launch, one wavefront per read (include/taiyaki_amd_basecall.h, (e)).
//
// The search is beam_search.h's kernel body -- the one tk_flipflop_beamsearch_dev runs -- instantiated with
// BeamPackedArgs; this file holds nothing but the launch.  It is compiled with the flags of beam_kernels.o (not with
// basecall_kernels.o's -ffp-contract=off), so both instantiations evaluate the same expressions the same way.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/taiyaki_amd_basecall.h"

#define TK_BEAM_TABLES_ONLY     // the log-sum-exp tables: their one copy
#include "beam_kernels.hip"
#undef TK_BEAM_TABLES_ONLY
#include "beam_search.h"

namespace tk {

static size_t packed_bwd_bytes(size_t total_rows, size_t nread, size_t nbase) {
    return ((total_rows + nread) * 2 * nbase * sizeof(float) + 255) / 256 * 256;
}

}  // namespace tk

extern "C" {

size_t tk_basecall_beamsearch_workspace_bytes(size_t total_rows, size_t nread, size_t nbase) {
    return tk::packed_bwd_bytes(total_rows, nread, nbase) + total_rows * 16 + 512;
}

int tk_basecall_beamsearch_dev(const float *scores, const int64_t *row_off, const int32_t *nrows, size_t nread,
                               size_t total_rows, size_t max_rows, size_t nbase, const char *alphabet, int beam_width,
                               float beam_cut, int guided, int8_t *states, int32_t *nstate, float *score, uint8_t *seq,
                               int32_t *seqlen, void *workspace, size_t workspace_bytes, uint32_t *status,
                               void *stream) {
    if (!row_off || !nrows || !alphabet || !nstate || !score || !seqlen || !workspace) return TK_ERR_BAD_ARG;
    if (total_rows > 0 && (!scores || !states || !seq)) return TK_ERR_BAD_ARG;
    if (const int rc = tk::beam_admit(nbase, beam_width, beam_cut)) return rc;
    if (nread > (size_t)INT32_MAX || total_rows > (size_t)INT64_MAX / 64 || max_rows > total_rows)
        return TK_ERR_UNSUPPORTED;
    if (workspace_bytes < tk_basecall_beamsearch_workspace_bytes(total_rows, nread, nbase)) return TK_ERR_WORKSPACE;
    if (nread == 0) return TK_OK;
    tk::BeamPackedArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = scores;
    a.nbase = (int)nbase;
    a.width = beam_width;
    a.logcut = tk::beam_logcut(beam_cut);
    a.guided = guided;
    a.bwd = static_cast<float *>(workspace);
    a.bp = reinterpret_cast<unsigned char *>(static_cast<char *>(workspace) +
                                             tk::packed_bwd_bytes(total_rows, nread, nbase));
    a.seq = reinterpret_cast<signed char *>(states);
    a.seqlen = nstate;
    a.score = score;
    // the back-pointer window in LDS is sized from the longest read of the launch; a read past it walks HBM
    a.lds_rows = (int)(max_rows <= tk::BEAM_LDS_ROWS ? max_rows : tk::BEAM_LDS_ROWS);
    a.row_off = row_off;
    a.nrows = nrows;
    a.total_rows = (int64_t)total_rows;
    a.call = seq;
    a.calllen = seqlen;
    for (size_t b = 0; b < nbase; ++b) a.alphabet |= (uint32_t)(unsigned char)alphabet[b] << (8 * b);
    a.status = status;
    a.status_bit = TK_STATUS_CHUNK_PLAN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)a.lds_rows * 16;
    if (nbase == 4)
        hipLaunchKernelGGL((tk::beam_kernel<4, tk::BeamPackedArgs>), dim3((unsigned)nread), dim3(tk::WAVE), lds, s, a);
    else
        hipLaunchKernelGGL((tk::beam_kernel<0, tk::BeamPackedArgs>), dim3((unsigned)nread), dim3(tk::WAVE), lds, s, a);
    return hipGetLastError() == hipSuccess ? TK_OK : TK_ERR_LAUNCH;
}

}  // extern "C"

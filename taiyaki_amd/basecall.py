"""Basecall batches of reads on the device: raw float32 signals in, sequences and quality strings out
(``bin/basecall.py:151-242``: the Viterbi path, `posterior` on or off, or -- ``beam=(width, guided)`` -- the hash beam
search on every read's stitched transition scores).

Between the upload of the signals and the download of the finished characters nothing runs on the host: median / MAD
normalisation, chunking and the tail (stitch, collapse, quality characters) are the three kernels of
include/taiyaki_amd_basecall.h; the network, `flipflop_make_trans`, the Viterbi and `errprobs_from_trans` are the
operators this package already has.  `call_mods` adds, for a cat-mod model, the modified-base scores of every called
base (tk_basecall_mod_weights_dev on the Viterbi paths and the network's categorical columns), in the same download.
With a beam, the stitched scores of all the batch's reads
(tk_basecall_stitch_scores_dev) go through ONE launch of the beam search (tk_basecall_beamsearch_dev), which writes the
calls.  There is no CPU fallback: a model that is not on an AMD GPU raises.
"""
import collections
import ctypes

import numpy as np
import torch

from taiyaki_amd import _lib, basecall_helpers, decode, decodeutil, flipflopfings, layers, qscores

Beam = collections.namedtuple("Beam", "width guided")       # bin/basecall.py's --beam
Slice = collections.namedtuple("Slice", "short first ncol reads")
Slice.__doc__ = """One model invocation of the packing plan: `ncol` columns.  short=False: columns [first, first + ncol)
of the batch's chunk tensor; short=True: the one chunk, of its own length, of read `first`.  `reads`: the read of
every column."""


def chunk_counts(lengths, chunk_size, overlap):
    """Chunks per read in the batch's chunk tensor (samples): the closed form of basecall_helpers.chunk_read's count,
    0 for a read shorter than `chunk_size` (it is called alone, as one chunk of its own length)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    step = chunk_size - overlap
    return np.where(lengths < chunk_size, 0, (lengths - chunk_size + step - 1) // step + 1)


def packing_plan(lengths, chunk_size, overlap, max_concurrent_chunks, pack=True):
    """The model invocations for reads of `lengths` samples, host arithmetic on lengths alone.  Every chunk appears
    once, in read order; no slice is wider than `max_concurrent_chunks`.  pack=True fills every slice across read
    boundaries; pack=False splits per read, as `torch.split` does in bin/basecall.py:208.  Reads shorter than
    `chunk_size` follow as slices of one column each (reads without samples get none)."""
    counts = chunk_counts(lengths, chunk_size, overlap)
    owner = np.repeat(np.arange(len(counts)), counts)
    plan = []
    if pack:
        bounds = [(0, len(owner))]
    else:
        off = np.concatenate([[0], np.cumsum(counts)])
        bounds = [(int(off[r]), int(off[r + 1])) for r in range(len(counts)) if counts[r]]
    for lo, hi in bounds:
        for first in range(lo, hi, max_concurrent_chunks):
            ncol = min(max_concurrent_chunks, hi - first)
            plan.append(Slice(False, first, ncol, tuple(int(r) for r in owner[first:first + ncol])))
    for r, n in enumerate(lengths):
        if 0 < n < chunk_size:
            plan.append(Slice(True, r, 1, (r,)))
    return plan


def stitched_rows(nchunks, siglen, chunk_size, overlap, stride, nrow):
    """Rows that basecall_helpers.stitch_chunks keeps of a read's `nchunks` chunks of `nrow` rows each: the bound of
    the read's call length."""
    if nchunks <= 1:
        return nrow * nchunks
    starts, ends = basecall_helpers.chunk_bounds(siglen, chunk_size, overlap)
    lo = np.concatenate([[starts[0] // stride], (ends[:-1] - starts[1:]) // (2 * stride)])
    hi = np.concatenate([[(ends[0] + starts[1]) // (2 * stride)],
                         (ends[1:-1] + starts[2:] - 2 * starts[1:-1]) // (2 * stride),
                         [(ends[-1] - starts[-1]) // stride]])
    return int(np.maximum(np.minimum(hi, nrow) - np.minimum(lo, nrow), 0).sum())


def check_beam(beam, beam_cut, nbase, fastq):
    """`Basecaller`'s beam arguments -> Beam(width, guided), or None.  ValueError for a beam together with fastq (the
    reference has no quality string for a beam call), for a width outside the search's admission rule (1..12 with
    width * (nbase + 1) <= 64; nbase 1..4) and for a beam_cut outside [0, 1]."""
    if beam is None:
        return None
    if fastq:
        raise ValueError("Basecaller: beam search gives no quality string (fastq=True needs beam=None)")
    try:
        width, guided = beam
    except (TypeError, ValueError):
        raise ValueError("Basecaller: beam is (width, guided), got %r" % (beam,)) from None
    decodeutil.check_beam(nbase, width, beam_cut, "Basecaller")
    return Beam(int(width), bool(guided))


def check_mods(model, mod_output, beam, nbase):
    """`Basecaller`'s mod_output argument -> the model's can_nmods as a list, or None.  ValueError for mod_output
    together with a beam (the search's states are not per chunk), on a model whose last layer is not
    GlobalNormFlipFlopCatMod, and on one without a modification (or with more than the kernel's
    TK_BASECALL_MAX_NMOD, or whose canonical alphabet is not `nbase` long)."""
    if not mod_output:
        return None
    if beam is not None:
        raise ValueError("Basecaller: mod_output needs the Viterbi path (beam=None); the beam search's states are not "
                         "per chunk")
    if not (isinstance(model, layers.Serial) and layers.is_cat_mod_model(model)):
        raise ValueError("Basecaller: mod_output needs a model whose last layer is GlobalNormFlipFlopCatMod")
    can_nmods = [int(n) for n in model[-1].can_nmods]
    cap = _lib.BASECALL_DEFINES["TK_BASECALL_MAX_NMOD"]
    if sum(can_nmods) == 0:
        raise ValueError("Basecaller: mod_output on a model without a modification (can_nmods %r)" % (can_nmods,))
    if len(can_nmods) != nbase or sum(can_nmods) > cap:
        raise ValueError("Basecaller: can_nmods %r does not fit an alphabet of %d bases and at most %d modifications"
                         % (can_nmods, nbase, cap))
    return can_nmods


def _align(n, to=16):
    return (n + to - 1) // to * to


class Basecaller:
    """`call(signals)` -> [(sequence, quality string or None, nsamples)] for a batch of reads; with mod_output=True,
    `call_mods(signals)` -> (the same list, [the modified-base scores of every read's call]).

    chunk_size / overlap are in blocks of the model's stride, as on the reference's command line; `stride` is guessed
    from the model when not given (helpers.guess_model_stride).  `reverse`: the signals are reversed before calling
    (the reference's model.metadata['reverse']).  `pack`: fill the model's batches across read boundaries; False
    splits them per read, exactly as the reference's loop does.  `beam`: (width, guided) decodes every read with the
    hash beam search on its stitched scores instead of the Viterbi path (`beam_cut` as decodeutil.beamsearch's); no
    quality strings then.  `mod_output`: the model is a cat-mod model (its last layer GlobalNormFlipFlopCatMod) and
    `call_mods` is wanted; `call` gives what it gives without it."""

    def __init__(self, model, stride=None, chunk_size=1000, overlap=100, max_concurrent_chunks=128, alphabet="ACGT",
                 posterior=True, temperature=1.0, fastq=False, qscore_scale=1.0, qscore_offset=0.0, reverse=False,
                 pack=True, beam=None, beam_cut=0.0, mod_output=False):
        self.beam, self.beam_cut = check_beam(beam, beam_cut, len(alphabet), fastq), float(beam_cut)
        self.can_nmods = check_mods(model, mod_output, beam, len(alphabet))
        self.model = model
        self.device = basecall_helpers.get_model_device(model)
        if self.device.type != "cuda":
            raise RuntimeError("Basecaller: the model is on %s; basecalling only runs as HIP kernels on an AMD GPU "
                               "(no CPU fallback)" % self.device)
        self.stride = int(stride) if stride is not None else basecall_helpers.guess_model_stride(model)
        self.chunk_size, self.overlap = int(chunk_size) * self.stride, int(overlap) * self.stride
        if not 0 <= self.overlap < self.chunk_size:
            raise ValueError("overlap must be smaller than chunk_size")
        self.max_concurrent_chunks = int(max_concurrent_chunks)
        self.alphabet = alphabet.encode("ascii")
        self.n_can_state = flipflopfings.nstate_flipflop(len(alphabet))
        self.posterior, self.temperature, self.fastq = bool(posterior), float(temperature), bool(fastq)
        self.qscore_scale, self.qscore_offset = float(qscore_scale), float(qscore_offset)
        self.reverse, self.pack = bool(reverse), bool(pack)

    def plan(self, lengths):
        return packing_plan(lengths, self.chunk_size, self.overlap, self.max_concurrent_chunks, self.pack)

    # -- steps 4-8 of a call: the network and the decode operators on one chunk tensor ---------------------------------
    def _trans(self, outs):
        if self.can_nmods:      # (`_run` kept the categorical columns)
            outs = [o[:, :, :self.n_can_state] for o in outs]
        trans = torch.cat(outs, 1) * self.temperature
        if self.posterior:
            trans = (decode.flipflop_make_trans(trans) + 1e-8).log()
        return trans

    def _decode(self, outs):
        trans = self._trans(outs)
        path = decode.flipflop_viterbi_path(trans)
        return path, (qscores.errprobs_from_trans(trans, path) if self.fastq else None)

    def _run(self, chunks):
        """The network on one chunk tensor: its transition scores and, with mod_output, the categorical columns
        behind them."""
        out = self.model(chunks)
        return out if self.can_nmods else out[:, :, :self.n_can_state]

    def _mod_weights(self, outs):
        return torch.cat([o[:, :, self.n_can_state:] for o in outs], 1).contiguous()

    def call(self, signals, read_params=None):
        return self._call(signals, read_params, False)[0]

    def call_mods(self, signals, read_params=None):
        """-> (results, mods): `results` is exactly what `call` returns; mods[r] is a float32 array (len(sequence r),
        nmod): row i holds, for character i of read r's call, the log-probabilities of the modifications of ITS
        canonical base (the network's categorical columns at the block before the move, flipflopfings.py:100-143) and
        NaN in the columns of the other bases' modifications; columns in can_nmods order.  With reverse=True the rows
        are in the order of the unreversed call string in `results` -- the call of the reversed signal -- which
        `write_records(reverse=True)` writes back to front.  The network runs once per slice, and the scores ride in
        the call's one download, behind seq | qual."""
        if not self.can_nmods:
            raise RuntimeError("Basecaller.call_mods needs mod_output=True at construction")
        return self._call(signals, read_params, True)

    def _call(self, signals, read_params, want_mods):
        L, dev, nread = _lib.basecall_lib(), self.device, len(signals)
        if nread == 0:
            return [], []
        sigs = [np.asarray(s, dtype=np.float32).reshape(-1) for s in signals]
        if self.reverse:
            sigs = [s[::-1] for s in sigs]
        lens = np.array([len(s) for s in sigs], dtype=np.int64)
        params = list(read_params) if read_params is not None else [None] * nread
        given = np.array([p is not None for p in params])
        # 1. ONE upload: signals | offsets | the caller's shift and scale
        nsig = int(lens.sum())
        o_off = _align(4 * nsig)
        o_shift = o_off + _align(8 * (nread + 1))
        o_scale = o_shift + _align(4 * nread)
        host = np.zeros(o_scale + _align(4 * nread), dtype=np.uint8)
        host[:4 * nsig].view(np.float32)[:] = np.concatenate(sigs) if nsig else 0
        host[o_off:o_off + 8 * (nread + 1)].view(np.int64)[:] = np.concatenate([[0], np.cumsum(lens)])
        host[o_shift:o_shift + 4 * nread].view(np.float32)[:] = [p[0] if p is not None else 0 for p in params]
        host[o_scale:o_scale + 4 * nread].view(np.float32)[:] = [p[1] if p is not None else 1 for p in params]
        plan = self.plan(lens)
        counts = chunk_counts(lens, self.chunk_size, self.overlap)
        total = int(counts.sum())
        with torch.cuda.device(dev), torch.no_grad():
            stream = _lib.stream_ptr()
            up = torch.from_numpy(host).to(dev)
            signal, sig_off = up[:4 * max(nsig, 1)].view(torch.float32), up[o_off:o_off + 8 * (nread + 1)].view(torch.int64)
            shift = up[o_shift:o_shift + 4 * nread].view(torch.float32)
            scale = up[o_scale:o_scale + 4 * nread].view(torch.float32)
            # the ONE download comes from here: seqlen | status | seq | qual (sized once the block counts are known)
            head = torch.zeros(_align(4 * nread) + 16, dtype=torch.uint8, device=dev)
            seqlen, status = head[:4 * nread].view(torch.int32), head[_align(4 * nread):]
            # 2. median / MAD where no parameters were given
            if not given.all():
                medmad = torch.empty(2, nread, dtype=torch.float32, device=dev)
                _lib.check(L.tk_signal_med_mad_dev(_lib.ptr(signal), _lib.ptr(sig_off), nread, _lib.ptr(medmad[0]),
                                                   _lib.ptr(medmad[1]), _lib.ptr(status), stream), "tk_signal_med_mad_dev")
                if given.any():
                    mask = torch.from_numpy(given).to(dev)
                    shift, scale = torch.where(mask, shift, medmad[0]), torch.where(mask, scale, medmad[1])
                else:
                    shift, scale = medmad[0], medmad[1]
            # 3. normalise + chunk: the batch's chunk tensor, and each short read as one chunk of its own length
            starts = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
            ends = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
            read_chunk_off = torch.empty(nread + 1, dtype=torch.int64, device=dev)
            chunks = torch.empty(self.chunk_size, total, 1, dtype=torch.float32, device=dev)
            ws = torch.empty(max(L.tk_basecall_gather_workspace_bytes(total), 16), dtype=torch.uint8, device=dev)
            _lib.check(L.tk_basecall_gather_chunks_dev(
                _lib.ptr(signal), _lib.ptr(sig_off), nread, nsig, _lib.ptr(shift), _lib.ptr(scale), self.chunk_size,
                self.overlap, total, _lib.ptr(chunks), _lib.ptr(starts), _lib.ptr(ends), _lib.ptr(read_chunk_off),
                _lib.ptr(ws), ws.numel(), _lib.ptr(status), stream), "tk_basecall_gather_chunks_dev")
            one = torch.tensor([0, 1], dtype=torch.int64, device=dev)      # read_chunk_off of a read called alone
            outs, short, short_w = [], [], {}
            for sl in plan:
                if not sl.short:
                    # 4. the network on column slices of at most max_concurrent_chunks
                    outs.append(self._run(chunks[:, sl.first:sl.first + sl.ncol].contiguous()))
                    continue
                r, n = sl.first, int(lens[sl.first])
                own = torch.empty(n, 1, 1, dtype=torch.float32, device=dev)
                geo = torch.empty(3, 2, dtype=torch.int64, device=dev)     # starts, ends, read_chunk_off
                w1 = torch.empty(16, dtype=torch.uint8, device=dev)
                _lib.check(L.tk_basecall_gather_chunks_dev(
                    _lib.ptr(signal), _lib._vp(sig_off.data_ptr() + 8 * r), 1, nsig, _lib._vp(shift.data_ptr() + 4 * r),
                    _lib._vp(scale.data_ptr() + 4 * r), n, 0, 1, _lib.ptr(own), _lib.ptr(geo[0]), _lib.ptr(geo[1]),
                    _lib.ptr(geo[2]), _lib.ptr(w1), w1.numel(), _lib.ptr(status), stream), "tk_basecall_gather_chunks_dev")
                if self.beam:
                    short.append((r, self._trans([self._run(own)]).contiguous(), None, geo))
                    continue
                out = self._run(own)
                path, err = self._decode([out])
                short.append((r, path, err, geo))
                if want_mods:
                    short_w[r] = self._mod_weights([out])
            if self.beam:
                return self._call_beam(outs, short, counts, lens, starts, ends, read_chunk_off, scale, head), None
            # 5.-8. temperature, posterior, Viterbi, error probabilities on all the batch's chunks at once
            path = err = None
            if total:
                path, err = self._decode(outs)
            # room per read: its stitched row count bounds its call length
            rows = np.zeros(nread, dtype=np.int64)
            for r in range(nread):
                if counts[r]:
                    rows[r] = stitched_rows(int(counts[r]), int(lens[r]), self.chunk_size, self.overlap, self.stride,
                                            path.shape[0])
            for r, spath, _, _ in short:
                rows[r] = spath.shape[0]
            out_off_host = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
            cap = max(int(out_off_host[-1]), 1)
            out_off = torch.from_numpy(out_off_host).to(dev)
            nmod = sum(self.can_nmods) if want_mods else 0
            body = torch.empty(2 * _align(cap) + 4 * cap * nmod, dtype=torch.uint8, device=dev)
            seq, qual = body[:cap], body[_align(cap):_align(cap) + cap]
            if want_mods:       # behind seq | qual: read r's rows from row out_off[r], as its characters
                mods = body[2 * _align(cap):].view(torch.float32)
                nbase, can_nmods = len(self.alphabet), (ctypes.c_int * len(self.alphabet))(*self.can_nmods)
                weights = self._mod_weights(outs) if total else None
            qs, qo = self.qscore_scale, self.qscore_offset
            # 9. the tail (reads without a chunk in `path` get seqlen 0 here; the short ones are written next)
            if total:
                _lib.check(L.tk_basecall_call_dev(
                    _lib.ptr(path), _lib.ptr(err), path.shape[0] - 1, total, _lib.ptr(starts), _lib.ptr(ends),
                    _lib.ptr(read_chunk_off), _lib.ptr(scale), nread, self.stride, len(self.alphabet), self.alphabet,
                    qs, qo, _lib.ptr(out_off), _lib.ptr(seq), _lib.ptr(qual), _lib.ptr(seqlen), _lib.ptr(status),
                    stream), "tk_basecall_call_dev")
            for r, spath, serr, geo in short:
                _lib.check(L.tk_basecall_call_dev(
                    _lib.ptr(spath), _lib.ptr(serr), spath.shape[0] - 1, 1, _lib.ptr(geo[0]), _lib.ptr(geo[1]),
                    _lib.ptr(one), _lib._vp(scale.data_ptr() + 4 * r), 1, self.stride, len(self.alphabet),
                    self.alphabet, qs, qo, _lib._vp(out_off.data_ptr() + 8 * r), _lib.ptr(seq), _lib.ptr(qual),
                    _lib._vp(seqlen.data_ptr() + 4 * r), _lib.ptr(status), stream), "tk_basecall_call_dev")
            # 9b. the modified-base scores at the same moves: the same walk, the same offsets, the same seqlen
            if want_mods and total:
                _lib.check(L.tk_basecall_mod_weights_dev(
                    _lib.ptr(path), _lib.ptr(weights), path.shape[0] - 1, total, _lib.ptr(starts), _lib.ptr(ends),
                    _lib.ptr(read_chunk_off), _lib.ptr(scale), nread, self.stride, nbase, can_nmods, _lib.ptr(out_off),
                    _lib.ptr(mods), _lib.ptr(seqlen), _lib.ptr(status), stream), "tk_basecall_mod_weights_dev")
            for r, spath, _, geo in short if want_mods else ():
                _lib.check(L.tk_basecall_mod_weights_dev(
                    _lib.ptr(spath), _lib.ptr(short_w[r]), spath.shape[0] - 1, 1, _lib.ptr(geo[0]), _lib.ptr(geo[1]),
                    _lib.ptr(one), _lib._vp(scale.data_ptr() + 4 * r), 1, self.stride, nbase, can_nmods,
                    _lib._vp(out_off.data_ptr() + 8 * r), _lib.ptr(mods), _lib._vp(seqlen.data_ptr() + 4 * r),
                    _lib.ptr(status), stream), "tk_basecall_mod_weights_dev")
            # 10. ONE download
            got = torch.cat([head, body]).cpu().numpy()
        nhead = head.numel()
        bits = int(got[_align(4 * nread):nhead].view(np.uint32)[0])
        if bits & _lib.BASECALL_DEFINES["TK_STATUS_CHUNK_PLAN"]:
            raise RuntimeError("basecall: the device's chunk plan disagrees with the host's (status %#x)" % bits)
        called, seq_h = got[:4 * nread].view(np.int32), got[nhead:nhead + cap]
        qual_h = got[nhead + _align(cap):nhead + _align(cap) + cap]
        results = []
        for r in range(nread):
            lo, hi = int(out_off_host[r]), int(out_off_host[r]) + int(called[r])
            q = qual_h[lo:hi].tobytes().decode("ascii") if self.fastq else None
            results.append((seq_h[lo:hi].tobytes().decode("ascii"), q, int(lens[r])))
        if not want_mods:
            return results, None
        mods_h = got[nhead + 2 * _align(cap):].view(np.float32).reshape(cap, nmod)
        return results, [mods_h[int(out_off_host[r]):int(out_off_host[r]) + int(called[r])].copy() for r in range(nread)]

    def _call_beam(self, outs, short, counts, lens, starts, ends, read_chunk_off, scale, head):
        """The rest of a call with a beam, inside `call`'s device context (bin/basecall.py:216-221 for every read):
        stitch the scores of the batch's chunk tensor and of each short read's own chunk into ONE packed buffer, ONE
        launch of the beam search, which also writes the calls, ONE download of seqlen | status | seq."""
        L, dev, nread, stream = _lib.basecall_lib(), self.device, len(lens), _lib.stream_ptr()
        seqlen, status = head[:4 * nread].view(torch.int32), head[_align(4 * nread):]
        total = int(counts.sum())
        trans = self._trans(outs).contiguous() if total else None
        # room per read: its stitched row count
        rows = np.zeros(nread, dtype=np.int64)
        for r in range(nread):
            if counts[r]:
                rows[r] = stitched_rows(int(counts[r]), int(lens[r]), self.chunk_size, self.overlap, self.stride,
                                        trans.shape[0])
        for r, strans, _, _ in short:
            rows[r] = strans.shape[0]
        row_off_host = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        total_rows = int(row_off_host[-1])
        row_off = torch.from_numpy(row_off_host).to(dev)
        packed = torch.empty(total_rows, self.n_can_state, dtype=torch.float32, device=dev)
        nrows = torch.zeros(nread, dtype=torch.int32, device=dev)
        one = torch.tensor([0, 1], dtype=torch.int64, device=dev)
        if total:       # (reads without a chunk in `trans` get 0 rows here; the short ones are written next)
            _lib.check(L.tk_basecall_stitch_scores_dev(
                _lib.ptr(trans), trans.shape[0], total, trans.shape[2], _lib.ptr(starts), _lib.ptr(ends),
                _lib.ptr(read_chunk_off), _lib.ptr(scale), nread, self.stride, _lib.ptr(row_off), total_rows,
                _lib.ptr(packed), _lib.ptr(nrows), _lib.ptr(status), stream), "tk_basecall_stitch_scores_dev")
        for r, strans, _, geo in short:
            _lib.check(L.tk_basecall_stitch_scores_dev(
                _lib.ptr(strans), strans.shape[0], 1, strans.shape[2], _lib.ptr(geo[0]), _lib.ptr(geo[1]), _lib.ptr(one),
                _lib._vp(scale.data_ptr() + 4 * r), 1, self.stride, _lib._vp(row_off.data_ptr() + 8 * r), total_rows,
                _lib.ptr(packed), _lib._vp(nrows.data_ptr() + 4 * r), _lib.ptr(status), stream),
                "tk_basecall_stitch_scores_dev")
        _, _, _, seq, _ = decodeutil.beamsearch_packed(packed, row_off, nrows, int(rows.max()), self.alphabet,
                                                       self.beam.width, self.beam_cut, self.beam.guided, status, seqlen)
        got = torch.cat([head, seq[:max(total_rows, 1)]]).cpu().numpy()
        nhead = head.numel()
        bits = int(got[_align(4 * nread):nhead].view(np.uint32)[0])
        if bits & _lib.BASECALL_DEFINES["TK_STATUS_CHUNK_PLAN"]:
            raise RuntimeError("basecall: the device's chunk plan disagrees with the host's (status %#x)" % bits)
        called, seq_h = got[:4 * nread].view(np.int32), got[nhead:]
        return [(seq_h[int(row_off_host[r]):int(row_off_host[r]) + int(called[r])].tobytes().decode("ascii"), None,
                 int(lens[r])) for r in range(nread)]


def write_records(fh, ids, results, fastq, reverse=False):
    """The output loop of bin/basecall.py:280-291: one FASTA / FASTQ record per read with a non-empty call
    (`reverse`: sequence and qualities written back to front).  Returns (nbase, ncalled, nread, nsample)."""
    nbase = ncalled = nread = nsample = 0
    for read_id, (basecall, qstring, read_nsample) in zip(ids, results):
        if basecall is not None and len(basecall) > 0:
            fh.write("{}{}\n{}\n".format("@" if fastq else ">", read_id, basecall[::-1] if reverse else basecall))
            nbase += len(basecall)
            ncalled += 1
            if fastq:
                fh.write("+\n{}\n".format(qstring[::-1] if reverse else qstring))
        nread += 1
        nsample += read_nsample
    return nbase, ncalled, nread, nsample

"""Drop-in for ``taiyaki.decodeutil`` (taiyaki/decodeutil/decodeutil.pyx): ``beamsearch`` (9-51),
the hash beam search over the flip-flop lattice, and the decoder's ``forward`` / ``backward``
lattice passes (54-108), on the gfx950 kernels of csrc/beam_kernels.hip.

The reference decodes one read per call on the host; here a call takes one read ``(T, S)`` --
same return value ``(sequence, score)`` -- or a batch ``(T, N, S)`` (one wavefront per read, one
launch) and then returns ``(list of sequences, scores)``.  ``beamsearch_batch`` takes reads of DIFFERENT lengths and
decodes them in one launch too (tk_basecall_beamsearch_dev: the same kernel body over packed rows).
"""
import numpy as np
import torch

from taiyaki_amd import _lib, flipflopfings


def beamsearch(score, beam_cut=0.0, beam_width=5, guided=True):
    """decodeutil.pyx:9-51.  `score`: torch tensor on the GPU (or a numpy array, uploaded) of
    shape (T, ntrans) or (T, N, ntrans).  Returns (int8 flip-flop state sequence, score) resp.
    ([sequences], scores (N,) float32)."""
    if not torch.is_tensor(score):
        if not torch.cuda.is_available():
            raise RuntimeError("beamsearch: no AMD GPU; the flip-flop operators only run as HIP kernels "
                               "(no CPU fallback)")
        score = torch.as_tensor(np.ascontiguousarray(score, dtype=np.float32)).cuda()
    _lib.require_gpu(score, "beamsearch")
    single = score.dim() == 2
    sc = (score.unsqueeze(1) if single else score).detach().float().contiguous()
    T, N, S = sc.shape
    nbase = flipflopfings.nbase_flipflop(S)
    if not 1 <= int(beam_width) <= 12 or int(beam_width) * (nbase + 1) > 64:
        raise ValueError("beamsearch: beam_width %d not in 1..12 (one candidate record per lane of a wavefront: "
                         "beam_width * (nbase + 1) <= 64)" % int(beam_width))
    if not 0.0 <= float(beam_cut) <= 1.0:
        raise ValueError("beamsearch: beam_cut %r outside [0, 1]" % (beam_cut,))
    L = _lib.lib()
    dev = sc.device
    with torch.cuda.device(dev):
        seq = torch.empty((N, T), dtype=torch.int8, device=dev)
        seqlen = torch.empty(N, dtype=torch.int32, device=dev)
        out = torch.empty(N, dtype=torch.float32, device=dev)
        wsb = L.tk_flipflop_beamsearch_workspace_bytes(T, N, nbase)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rc = L.tk_flipflop_beamsearch_dev(_lib.ptr(sc), T, N, nbase, int(beam_width), float(beam_cut),
                                          int(bool(guided)), _lib.ptr(seq), _lib.ptr(seqlen), _lib.ptr(out),
                                          _lib.ptr(ws), wsb, _lib.stream_ptr())
        _lib.check(rc, "tk_flipflop_beamsearch_dev")
    seq_h, len_h, sc_h = seq.cpu().numpy(), seqlen.cpu().numpy(), out.cpu().numpy()
    seqs = [seq_h[n, :len_h[n]].copy() for n in range(N)]
    if single:
        return seqs[0], float(sc_h[0])
    return seqs, sc_h


def check_beam(nbase, beam_width, beam_cut, what="beamsearch"):
    """The admission rule of `beamsearch` and of the kernels behind it: ValueError outside it."""
    if not 1 <= nbase <= 4:
        raise ValueError("%s: %d bases; the beam search takes alphabets of 1 to 4" % (what, nbase))
    if int(beam_width) != beam_width or not 1 <= int(beam_width) <= 12 or int(beam_width) * (nbase + 1) > 64:
        raise ValueError("%s: beam_width %r not in 1..12 (one candidate record per lane of a wavefront: "
                         "beam_width * (nbase + 1) <= 64)" % (what, beam_width))
    if not 0.0 <= float(beam_cut) <= 1.0:
        raise ValueError("%s: beam_cut %r outside [0, 1]" % (what, beam_cut))


def beamsearch_packed(packed, row_off, nrows, max_rows, alphabet, beam_width, beam_cut, guided, status=None, seqlen=None):
    """tk_basecall_beamsearch_dev on device tensors: `packed` (total_rows, ntrans) f32, `row_off` (nread + 1) int64,
    `nrows` (nread) int32; `max_rows`: the longest room (host int).  Enqueues ONE launch and returns the device tensors
    (states int8, nstate int32, score f32, seq uint8, seqlen int32), each read's at its row_off.  `status`: the
    basecall library's device status word; `seqlen`: where the call lengths go, when the caller has a place for them."""
    L, dev, nread = _lib.basecall_lib(), packed.device, nrows.numel()
    total, nbase = packed.shape[0], flipflopfings.nbase_flipflop(packed.shape[1])
    assert packed.is_contiguous() and packed.dtype == torch.float32 and len(alphabet) == nbase
    with torch.cuda.device(dev):
        states = torch.empty(max(total, 1), dtype=torch.int8, device=dev)
        seq = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        nstate = torch.empty(nread, dtype=torch.int32, device=dev)
        seqlen = seqlen if seqlen is not None else torch.empty(nread, dtype=torch.int32, device=dev)
        score = torch.empty(nread, dtype=torch.float32, device=dev)
        wsb = L.tk_basecall_beamsearch_workspace_bytes(total, nread, nbase)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _lib.check(L.tk_basecall_beamsearch_dev(
            _lib.ptr(packed), _lib.ptr(row_off), _lib.ptr(nrows), nread, total, int(max_rows), nbase, alphabet,
            int(beam_width), float(beam_cut), int(bool(guided)), _lib.ptr(states), _lib.ptr(nstate), _lib.ptr(score),
            _lib.ptr(seq), _lib.ptr(seqlen), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr()),
            "tk_basecall_beamsearch_dev")
    return states, nstate, score, seq, seqlen


def beamsearch_batch(scores, beam_cut=0.0, beam_width=5, guided=True):
    """`beamsearch` for a list of reads of different lengths, `scores[i]` of shape (T_i, ntrans) (tensors on the GPU or
    numpy arrays; T_i = 0 is allowed), in ONE launch, one wavefront per read.  Returns ([int8 flip-flop state sequences],
    float32 scores (len(scores),)): read for read what `beamsearch` returns, bit for bit.  The launch lasts as long as
    its longest read."""
    if not torch.cuda.is_available():
        raise RuntimeError("beamsearch_batch: no AMD GPU; the flip-flop operators only run as HIP kernels "
                           "(no CPU fallback)")
    if len(scores) == 0:
        return [], np.zeros(0, dtype=np.float32)
    dev = next((s.device for s in scores if torch.is_tensor(s)), torch.device("cuda", torch.cuda.current_device()))
    rows = []
    for s in scores:
        if not torch.is_tensor(s):
            s = torch.as_tensor(np.ascontiguousarray(s, dtype=np.float32)).to(dev)
        _lib.require_gpu(s, "beamsearch_batch")
        if s.device != dev:
            raise ValueError("beamsearch_batch: reads on %s and %s; one launch runs on one device" % (dev, s.device))
        if s.dim() != 2 or (rows and s.shape[1] != rows[0].shape[1]):
            raise ValueError("beamsearch_batch: every read is (T_i, ntrans) with the same ntrans")
        rows.append(s.detach().float())
    nbase = flipflopfings.nbase_flipflop(rows[0].shape[1])
    check_beam(nbase, beam_width, beam_cut, "beamsearch_batch")
    lens = np.array([r.shape[0] for r in rows], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    with torch.cuda.device(dev):
        packed = torch.cat(rows, 0).contiguous()
        states, nstate, score, _, _ = beamsearch_packed(
            packed, torch.from_numpy(off).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), int(lens.max()),
            bytes(range(65, 65 + nbase)), beam_width, beam_cut, guided)
    st_h, n_h = states.cpu().numpy(), nstate.cpu().numpy()
    return [st_h[off[i]:off[i] + n_h[i]].copy() for i in range(len(rows))], score.cpu().numpy()


def _lattice(score, init, forward_pass, what):
    if not torch.is_tensor(score):
        if not torch.cuda.is_available():
            raise RuntimeError("%s: no AMD GPU; the flip-flop operators only run as HIP kernels "
                               "(no CPU fallback)" % what)
        score = torch.as_tensor(np.ascontiguousarray(score, dtype=np.float32)).cuda()
    _lib.require_gpu(score, what)
    single = score.dim() == 2
    sc = (score.unsqueeze(1) if single else score).detach().float().contiguous()
    T, N, S = sc.shape
    nbase = flipflopfings.nbase_flipflop(S)
    dev = sc.device
    with torch.cuda.device(dev):
        init_d = None
        if init is not None:
            init_d = torch.as_tensor(np.asarray(init, dtype=np.float32) if not torch.is_tensor(init) else init,
                                     dtype=torch.float32).to(dev).reshape(-1, 2 * nbase)
            if init_d.shape[0] == 1 and N > 1:
                init_d = init_d.expand(N, -1)
            init_d = init_d.contiguous()
            assert init_d.shape == (N, 2 * nbase), "init: one vector of 2 nbase states (per read)"
        out = torch.empty((N, T + 1, 2 * nbase), dtype=torch.float32, device=dev)
        total = torch.empty(N, dtype=torch.float32, device=dev)
        rc = _lib.lib().tk_flipflop_lattice_dev(_lib.ptr(sc), T, N, nbase, int(forward_pass), _lib.ptr(init_d),
                                                _lib.ptr(out), _lib.ptr(total), _lib.stream_ptr())
        _lib.check(rc, "tk_flipflop_lattice_dev")
    out_h, tot_h = out.cpu().numpy(), total.cpu().numpy()
    if single:
        return out_h[0], float(tot_h[0])
    return out_h, tot_h


def forward(score, init=None):
    """decodeutil.pyx:82-108 / c_flipflopfwdbwd.c:112-152: forward scores (T + 1, 2 nbase) of every
    block (row 0 = `init` or zeros) and their final log-sum-exp.  A batch (T, N, ntrans) returns
    (N, T + 1, 2 nbase) and (N,)."""
    return _lattice(score, init, True, "decodeutil.forward")


def backward(score, init=None):
    """decodeutil.pyx:54-79 / c_flipflopfwdbwd.c:55-91: backward scores (row T = `init` or zeros)."""
    return _lattice(score, init, False, "decodeutil.backward")

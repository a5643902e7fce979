"""Drop-in for the flip-flop entry points of ``taiyaki.decode`` (decode.py:15-115)."""
import numpy as np
import torch

from taiyaki_amd import _lib, flipflopfings


def flipflop_viterbi(scores, _never_use_cupy=False):
    """decode.py:15-39.  Returns (fwd (T+1,N,2nb) f32, traceback (T,N,2nb) int64,
    path (T+1,N) int64), bit-identical to the reference's torch path
    (decode.py:75-115: first-index tie rule)."""
    del _never_use_cupy
    _lib.require_gpu(scores, "flipflop_viterbi")
    L = _lib.lib()
    sc = scores.detach().float().contiguous()
    T, N, S = sc.shape
    nbase = flipflopfings.nbase_flipflop(S)
    dev = sc.device
    with torch.cuda.device(dev):
        fwd = torch.empty(T + 1, N, 2 * nbase, dtype=torch.float32, device=dev)
        tb = torch.empty(T, N, 2 * nbase, dtype=torch.int64, device=dev)
        path = torch.empty(T + 1, N, dtype=torch.int64, device=dev)
        wsb = L.tk_flipflop_viterbi_workspace_bytes(T, N, nbase)
        ws = _lib.workspace(wsb, dev, "viterbi")         # one scratch buffer per (device, stream), like ctc / layers
        rc = L.tk_flipflop_viterbi_dev(_lib.ptr(sc), T, N, nbase, _lib.ptr(fwd), _lib.ptr(tb),
                                       _lib.ptr(path), _lib.ptr(ws), wsb, _lib.stream_ptr())
        _lib.check(rc, "tk_flipflop_viterbi_dev")
    return fwd, tb, path


def _column_lengths(lengths, T, N, what):
    """`lengths` of an operator on (T, N, S) scores -> int32 (N), checked before anything is launched.  A host
    sequence holds one value in 0..T per column; a device tensor is taken as it is, without waiting for its values
    (the kernels clamp every entry to 0..T).  Anything else is a ValueError."""
    if torch.is_tensor(lengths) and lengths.is_cuda:
        if lengths.shape != (N,) or lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError("%s: lengths must hold one integer for each of the %d columns" % (what, N))
        return lengths.to(torch.int32).contiguous()
    try:
        host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths)
        ok = host.shape == (N,) and host.dtype.kind in "iu" and (N == 0 or (host.min() >= 0 and host.max() <= T))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: lengths must hold one integer in 0..%d for each of the %d columns" % (what, T, N))
    return torch.from_numpy(host.astype(np.int32))


def _varlen_args(scores, lengths, what):
    T, N, S = scores.shape
    lens = _column_lengths(lengths, T, N, what)
    _lib.require_gpu(scores, what)
    sc = scores.detach().float().contiguous()
    nbase = flipflopfings.nbase_flipflop(S)
    V = _lib.decode_varlen_lib()
    wsb = V.tk_decode_varlen_workspace_bytes(T, N, nbase)
    if wsb == 0:
        raise RuntimeError("%s: nbase=%d is not built" % (what, nbase))
    return V, sc, lens.to(sc.device), nbase, wsb


def flipflop_viterbi_path(scores, lengths=None):
    """Path-only Viterbi: what bin/basecall.py:222 keeps of `flipflop_viterbi` (the forward
    scores and the int64 traceback tensor, five times the size of the input, are not
    written).  `lengths` (a host sequence or a device tensor, one entry 0..T per column): column n has
    lengths[n] rows; path[:lengths[n] + 1, n] is what the column gives alone, every row beyond repeats
    path[lengths[n], n]."""
    if lengths is not None:
        V, sc, lens, nbase, wsb = _varlen_args(scores, lengths, "flipflop_viterbi_path")
        T, N, _ = sc.shape
        with torch.cuda.device(sc.device):
            path = torch.empty(T + 1, N, dtype=torch.int64, device=sc.device)
            ws = _lib.workspace(wsb, sc.device, "decode_varlen")
            _lib.check(V.tk_flipflop_viterbi_varlen_dev(_lib.ptr(sc), _lib.ptr(lens), T, N, nbase, _lib.ptr(path),
                                                        _lib.ptr(ws), wsb, _lib.stream_ptr()),
                       "tk_flipflop_viterbi_varlen_dev")
        return path
    _lib.require_gpu(scores, "flipflop_viterbi_path")
    L = _lib.lib()
    sc = scores.detach().float().contiguous()
    T, N, S = sc.shape
    nbase = flipflopfings.nbase_flipflop(S)
    dev = sc.device
    with torch.cuda.device(dev):
        path = torch.empty(T + 1, N, dtype=torch.int64, device=dev)
        wsb = L.tk_flipflop_viterbi_workspace_bytes(T, N, nbase)
        ws = _lib.workspace(wsb, dev, "viterbi")
        rc = L.tk_flipflop_viterbi_dev(_lib.ptr(sc), T, N, nbase, None, None, _lib.ptr(path),
                                       _lib.ptr(ws), wsb, _lib.stream_ptr())
        _lib.check(rc, "tk_flipflop_viterbi_dev")
    return path


def flipflop_make_trans(scores, _never_use_cupy=False, lengths=None):
    """decode.py:42-72: posterior transition probabilities (not logs) =
    d logZ / d scores; always detached, like the reference.  `lengths` (as for `flipflop_viterbi_path`):
    rows [0, lengths[n]) of column n are those of the column alone, every row beyond is 0."""
    del _never_use_cupy
    if lengths is not None:
        V, sc, lens, nbase, wsb = _varlen_args(scores, lengths, "flipflop_make_trans")
        T, N, _ = sc.shape
        with torch.cuda.device(sc.device):
            trans = torch.empty_like(sc)
            ws = _lib.workspace(wsb, sc.device, "decode_varlen")
            status = _lib.status_word(sc.device)
            _lib.check(V.tk_flipflop_posterior_varlen_dev(_lib.ptr(sc), _lib.ptr(lens), T, N, nbase, _lib.ptr(trans),
                                                          None, _lib.ptr(ws), wsb, _lib.ptr(status),
                                                          _lib.stream_ptr()), "tk_flipflop_posterior_varlen_dev")
            _lib.finish(status)
        return trans
    from taiyaki_amd.layers import _logz_launch
    _, trans = _logz_launch(scores, True)
    return trans

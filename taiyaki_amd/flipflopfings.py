"""Index algebra of the flip-flop code (host side, numpy) -- same names and
semantics as taiyaki/flipflopfings.py:6-184.  The training path does NOT use
these (ids are built on the device, csrc/crf_kernels.hip); they exist so that
callers and tests written against the reference module keep working.
`extract_mod_weights` is the exception: device tensors in, a HIP kernel, device tensors out."""
import ctypes

import numpy as np

DEFAULT_ALPHABET = 'ACGT'


def move_indices(labels, nbase=len(DEFAULT_ALPHABET)):
    """flipflopfings.py:6-17: labels[:-1] + min(labels[1:], nbase) * 2 nbase"""
    labels = np.asarray(labels)
    return labels[:-1] + np.minimum(labels[1:], nbase) * (nbase + nbase)


def stay_indices(labels, nbase=len(DEFAULT_ALPHABET)):
    """flipflopfings.py:20-31"""
    labels = np.asarray(labels)
    return labels + np.minimum(labels, nbase) * (nbase + nbase)


def flopmask(labels):
    """flipflopfings.py:34-53: True where a label sits at an even (2nd, 4th, ...)
    position within a run of identical labels.  Vectorised: position within the run = index
    minus the index at which the run started."""
    labels = np.asarray(labels)
    n = len(labels)
    if n == 0:
        return np.zeros(0, dtype=bool)
    idx = np.arange(n)
    new_run = np.ones(n, dtype=bool)
    new_run[1:] = labels[1:] != labels[:-1]
    run_start = np.maximum.accumulate(np.where(new_run, idx, 0))
    return ((idx - run_start) & 1).astype(bool)


def flipflop_code(labels, alphabet_length=4):
    """flipflopfings.py:56-78"""
    x = np.array(labels, copy=True)
    x[flopmask(x)] += alphabet_length
    return x


def path_to_str(path, alphabet=DEFAULT_ALPHABET, include_first_source=True):
    """flipflopfings.py:81-97: collapse a flip-flop state path into a basecall."""
    path = np.asarray(path)
    move = np.ediff1d(path, to_begin=1 if include_first_source else 0) != 0
    letters = np.frombuffer((alphabet * 2).encode(), dtype='u1')
    return letters[path[move]].tobytes().decode()


def extract_mod_weights(mod_weights, path, can_nmods):
    """flipflopfings.py:100-143 on DEVICE tensors (the function Megalodon's Taiyaki backend calls): the modified-base
    scores at the moves of a flip-flop path.  `mod_weights` holds, per block, the nbase + nmod categorical
    log-probabilities of a cat-mod model in the layer's grouped order (base 0 unmodified, its modifications, base 1
    ...); `can_nmods` the modifications of each canonical base.  Two forms:

    one read   mod_weights (T, ncat) float32, path (T + 1,) -> the reference's result, (nmoves + 1, nmod) float32 on the
               device: row 0 all NaN (the first state is never moved into), row i + 1 the i-th move's scores, NaN in
               the columns of other bases' modifications.
    a batch    mod_weights (T, N, ncat), path (T + 1, N) -> (scores, nbase): `scores` (nbase.sum(), nmod) float32,
               PACKED: the rows of read 0, then of read 1, ... WITHOUT the NaN row 0, so that row i of a read belongs to
               character i of path_to_str(path, include_first_source=False); `nbase` (N,) int32 on the device, the rows
               of every read (the read's offset is the sum of the counts before it).

    Both are ONE launch of tk_basecall_mod_weights_dev (include/taiyaki_amd_basecall.h) with every column as a read of
    one chunk; a pure selection, bit for bit.  The compaction to packed rows reads the counts (one host sync).  There
    is no CPU fallback: a CPU tensor raises."""
    import torch
    from taiyaki_amd import _lib
    _lib.require_gpu(mod_weights, "extract_mod_weights(mod_weights)")
    _lib.require_gpu(path, "extract_mod_weights(path)")
    single = mod_weights.dim() == 2
    if single:
        mod_weights, path = mod_weights[:, None], path[:, None]
    can_nmods = [int(n) for n in can_nmods]
    nmod = sum(can_nmods)
    if mod_weights.dim() != 3 or mod_weights.dtype != torch.float32:
        raise ValueError("extract_mod_weights: mod_weights is (T, ncat) or (T, N, ncat) float32")
    T, N, ncat = mod_weights.shape
    if tuple(path.shape) != (T + 1, N) or ncat != len(can_nmods) + nmod:
        raise ValueError("extract_mod_weights: path is (T + 1%s) and mod_weights has len(can_nmods) + sum(can_nmods) "
                         "columns; got %s and %s" % ("" if single else ", N", tuple(path.shape), tuple(mod_weights.shape)))
    if nmod == 0 or min(can_nmods) < 0:
        raise ValueError("extract_mod_weights: can_nmods has no modification")
    dev = mod_weights.device
    with torch.cuda.device(dev):
        path, mod_weights = path.to(torch.int64).contiguous(), mod_weights.contiguous()
        mods = torch.empty(N * T, nmod, dtype=torch.float32, device=dev)
        count = torch.zeros(N, dtype=torch.int32, device=dev)
        if T and N:
            geo = torch.zeros(N, dtype=torch.int64, device=dev)         # (a read of one chunk keeps all its rows)
            rco = torch.arange(N + 1, dtype=torch.int64, device=dev)
            room = rco * T                                              # every read has room for T moves
            _lib.check(_lib.basecall_lib().tk_basecall_mod_weights_dev(
                _lib.ptr(path), _lib.ptr(mod_weights), T, N, _lib.ptr(geo), _lib.ptr(geo), _lib.ptr(rco), None, N, 1,
                len(can_nmods), (ctypes.c_int * len(can_nmods))(*can_nmods), _lib.ptr(room), _lib.ptr(mods),
                _lib.ptr(count), None, _lib.stream_ptr()), "tk_basecall_mod_weights_dev")
        if single:
            first = torch.full((1, nmod), float("nan"), dtype=torch.float32, device=dev)
            return torch.cat([first, mods[:int(count.item())]])
        keep = torch.arange(T, device=dev)[None, :] < count[:, None]
        return mods.view(N, T, nmod)[keep], count


def nstate_flipflop(nbase):
    """flipflopfings.py:146-168: 2 nbase (nbase + 1) transitions"""
    return 2 * nbase * (nbase + 1)


def nbase_flipflop(nstate):
    """Inverse of `nstate_flipflop` (reference: flipflopfings.py:171-184, which solves the
    quadratic in floating point and asserts an integer root).  Integer arithmetic here:
    nstate = 2 b (b + 1)  <=>  b = (isqrt(1 + 2 nstate) - 1) / 2 with an exact square."""
    nstate = int(nstate)
    root = int(np.floor(np.sqrt(1.0 + 2.0 * nstate)))
    while root * root > 1 + 2 * nstate:        # (float sqrt may land one off for large values)
        root -= 1
    while (root + 1) * (root + 1) <= 1 + 2 * nstate:
        root += 1
    nbase = (root - 1) // 2
    if nstate <= 0 or root * root != 1 + 2 * nstate or nstate_flipflop(nbase) != nstate:
        raise AssertionError("%d transitions is not a flip-flop layout: no whole number of bases b has "
                             "2 b (b + 1) = %d" % (nstate, nstate))
    return nbase

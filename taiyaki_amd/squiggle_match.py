"""Drop-in for ``taiyaki.squiggle_match`` (taiyaki/squiggle_match/squiggle_match.pyx): the match of
observed signals against predicted squiggles -- per sequence position a level, a log-scale and a move
logit -- behind bin/train_squiggle.py (`squiggle_match_loss`) and bin/map_to_squiggle.py
(`squiggle_match_path`).  The dynamic programmes run as HIP kernels on the GPU
(csrc/squiggle_kernels.hip through the C ABI); there is no CPU fallback.

Same names, signatures and return values as the reference:

* `squiggle_match_cost`, `squiggle_match_grad`, `squiggle_match_path` take and return numpy arrays
  (they stage through the device);
* `squiggle_match_loss` (`SquiggleMatch.apply`) takes device tensors and returns the cost ON THE
  DEVICE (the reference returns a CPU tensor);
* `embed_sequence` is host code.

Lengths that cannot be right (a siglen <= 0, sum(siglen) > len(signal), no positions) raise
ValueError where the reference asserts or reads out of bounds: at once for host-resident lengths,
through the status word (like the other operators) for device-resident ones.
"""
import numpy as np
import torch

from taiyaki_amd import _lib

DEFAULT_ALPHABET = 'ACGT'       # taiyaki/constants.py
LARGE_LOG_VAL = 50000.0         # taiyaki/constants.py: what localpen / minscore = None stand for
MAX_NPOS = 1024                 # positions per read the kernels are built for (64 lanes x 16)

_base_mapping = {k: i for i, k in enumerate(DEFAULT_ALPHABET)}
_cartesian_tetrahedron = np.array([[1.0, 0.0, -1.0 / np.sqrt(2.0)],
                                   [-1.0, 0.0, -1.0 / np.sqrt(2.0)],
                                   [0.0, 1.0, 1.0 / np.sqrt(2.0)],
                                   [0.0, -1.0, 1.0 / np.sqrt(2.0)]], dtype=np.float32)


def embed_sequence(seq, alphabet=DEFAULT_ALPHABET):
    """Embed a sequence of bases (str / bytes over DEFAULT_ALPHABET, or base indices with
    alphabet=None) as vertices of a tetrahedron: (len(seq), 3) float32."""
    if alphabet == DEFAULT_ALPHABET:
        if isinstance(seq, (bytes, bytearray)):
            seq = seq.decode()
        seq_index = np.array([_base_mapping[b] for b in seq], dtype=np.int64)
    elif alphabet is None:
        seq_index = seq
    else:
        raise Exception('Alphabet not recognised in squiggle_match embed_sequence()')
    return _cartesian_tetrahedron[seq_index]


def _check_shapes(params_shape, nsignal, nlen):
    if len(params_shape) != 3 or params_shape[2] != 3:
        raise ValueError("squiggle match: params must be (npos, nbatch, 3), got %s" % (tuple(params_shape),))
    npos, nbatch = int(params_shape[0]), int(params_shape[1])
    if npos == 0:
        raise ValueError("squiggle match: params has no positions (npos = 0)")
    if npos > MAX_NPOS:
        raise ValueError("squiggle match: npos = %d is beyond the %d positions per read the kernels support"
                         % (npos, MAX_NPOS))
    if nbatch == 0 or nlen != nbatch:
        raise ValueError("squiggle match: params has %d reads but siglen has %d" % (nbatch, nlen))
    return npos, nbatch


def _check_host_lengths(siglen, nsignal):
    siglen = np.asarray(siglen)
    if siglen.ndim != 1:
        raise ValueError("squiggle match: siglen must be a vector")
    if np.any(siglen <= 0):
        raise ValueError("squiggle match: every siglen must be > 0 (got %d)" % int(siglen.min()))
    if int(siglen.astype(np.int64).sum()) > nsignal:
        raise ValueError("squiggle match: sum(siglen) = %d exceeds len(signal) = %d"
                         % (int(siglen.astype(np.int64).sum()), nsignal))


def _device_args(params, signal, siglen, what):
    """Checks and device-side staging shared by every entry: (params, signal, siglen int32, sig_off
    int64 (nbatch + 1), npos, nbatch, nsignal).  Host lengths are checked here; device lengths in
    the kernels (status word)."""
    _lib.require_gpu(params, what)
    _lib.require_gpu(signal, what)
    npos, nbatch = _check_shapes(tuple(params.shape), signal.numel(), int(siglen.shape[0]) if siglen.ndim else -1)
    if signal.ndim != 1:
        raise ValueError("squiggle match: signal must be a flat vector")
    dev = params.device
    if not siglen.is_cuda:
        _check_host_lengths(siglen.numpy(), signal.numel())
        siglen = siglen.to(dev)
    siglen = siglen.to(torch.int32).contiguous()
    sig_off = torch.zeros(nbatch + 1, dtype=torch.int64, device=dev)
    torch.cumsum(siglen, 0, out=sig_off[1:])
    params = params.detach().to(torch.float32).contiguous()
    signal = signal.detach().to(device=dev, dtype=torch.float32).contiguous()
    return params, signal, siglen, sig_off, npos, nbatch, signal.numel()


def _workspace_bytes(op, npos, nbatch, nsignal):
    return int(_lib.lib().tk_squiggle_match_workspace_bytes(op, npos, nbatch, nsignal))


def cost_dev(params, signal, siglen, back_prob, lattice=None):
    """Negated forward scores (nbatch,) on the device.  `lattice`: a device buffer of
    `lattice_bytes(...)` bytes that is left holding the forward columns for `grad_dev(...,
    lattice=...)` on the same inputs."""
    params, signal, siglen, sig_off, npos, nbatch, nsignal = _device_args(params, signal, siglen,
                                                                          "squiggle_match_cost")
    dev = params.device
    cost = torch.empty(nbatch, dtype=torch.float32, device=dev)
    status = _lib.status_word(dev)
    wsb = lattice.numel() if lattice is not None else 0
    _lib.check(_lib.lib().tk_squiggle_match_cost_dev(
        _lib.ptr(params), _lib.ptr(signal), _lib.ptr(siglen), _lib.ptr(sig_off), npos, nbatch, nsignal,
        float(back_prob), _lib.ptr(cost), _lib.ptr(lattice), wsb, _lib.ptr(status), _lib.stream_ptr()),
        "tk_squiggle_match_cost_dev")
    _lib.finish(status)
    return cost


def lattice_bytes(params, signal):
    npos, nbatch = int(params.shape[0]), int(params.shape[1])
    return _workspace_bytes(1, npos, nbatch, int(signal.numel()))


def grad_dev(params, signal, siglen, back_prob, lattice=None):
    """Negated gradient (npos, nbatch, 3) on the device, as c_squiggle_match.c:591-694 computes it.
    With `lattice` (filled by `cost_dev`) only the backward sweep runs."""
    params, signal, siglen, sig_off, npos, nbatch, nsignal = _device_args(params, signal, siglen,
                                                                          "squiggle_match_grad")
    dev = params.device
    grad = torch.empty((npos, nbatch, 3), dtype=torch.float32, device=dev)
    have = lattice is not None
    if not have:
        lattice = _lib.workspace(_workspace_bytes(1, npos, nbatch, nsignal), dev, "squiggle_lattice")
    status = _lib.status_word(dev)
    _lib.check(_lib.lib().tk_squiggle_match_grad_dev(
        _lib.ptr(params), _lib.ptr(signal), _lib.ptr(siglen), _lib.ptr(sig_off), npos, nbatch, nsignal,
        float(back_prob), int(have), None, _lib.ptr(grad), _lib.ptr(lattice), lattice.numel(),
        _lib.ptr(status), _lib.stream_ptr()), "tk_squiggle_match_grad_dev")
    _lib.finish(status)
    return grad


def path_dev(params, signal, siglen, back_prob, localpen=None, minscore=None):
    """(negated Viterbi scores (nbatch,), path (len(signal),) int32) on the device."""
    params, signal, siglen, sig_off, npos, nbatch, nsignal = _device_args(params, signal, siglen,
                                                                          "squiggle_match_path")
    localpen = LARGE_LOG_VAL if localpen is None else float(localpen)
    minscore = LARGE_LOG_VAL if minscore is None else float(minscore)
    dev = params.device
    cost = torch.empty(nbatch, dtype=torch.float32, device=dev)
    path = torch.zeros(nsignal, dtype=torch.int32, device=dev)
    ws = _lib.workspace(_workspace_bytes(2, npos, nbatch, nsignal), dev, "squiggle_path")
    status = _lib.status_word(dev)
    _lib.check(_lib.lib().tk_squiggle_match_path_dev(
        _lib.ptr(params), _lib.ptr(signal), _lib.ptr(siglen), _lib.ptr(sig_off), npos, nbatch, nsignal,
        float(back_prob), localpen, minscore, _lib.ptr(cost), _lib.ptr(path), _lib.ptr(ws), ws.numel(),
        _lib.ptr(status), _lib.stream_ptr()), "tk_squiggle_match_path_dev")
    _lib.finish(status)
    return cost, path


# ---------------------------------------------------------------------------------------------------
# the reference's numpy entry points (squiggle_match.pyx:27-97)
# ---------------------------------------------------------------------------------------------------
def _stage(params, signal, siglen, what):
    params = np.ascontiguousarray(params, dtype=np.float32)
    signal = np.ascontiguousarray(signal, dtype=np.float32)
    siglen = np.ascontiguousarray(siglen, dtype=np.int32)
    if signal.ndim != 1:
        raise ValueError("squiggle match: signal must be a flat vector")
    _check_shapes(params.shape, signal.size, siglen.shape[0] if siglen.ndim == 1 else -1)
    _check_host_lengths(siglen, signal.size)
    if not torch.cuda.is_available():
        raise RuntimeError("%s: the squiggle match runs as HIP kernels on an AMD GPU and none is available "
                           "(no CPU fallback)" % what)
    dev = torch.device("cuda", torch.cuda.current_device())
    return (torch.from_numpy(params).to(dev), torch.from_numpy(signal).to(dev), torch.from_numpy(siglen).to(dev))


def squiggle_match_cost(params, signal, siglen, back_prob):
    """Negated forward scores (nbatch,) float32 of matching `signal` (reads back to back, lengths
    `siglen`) to the predicted squiggles `params` (npos, nbatch, 3)."""
    return cost_dev(*_stage(params, signal, siglen, "squiggle_match_cost"), back_prob).cpu().numpy()


def squiggle_match_grad(params, signal, siglen, back_prob):
    """Negated gradient (npos, nbatch, 3) float32 of the forward scores (as the reference computes it)."""
    return grad_dev(*_stage(params, signal, siglen, "squiggle_match_grad"), back_prob).cpu().numpy()


def squiggle_match_path(params, signal, siglen, back_prob, localpen, minscore):
    """(negated Viterbi scores (nbatch,) float32, paths int32 like `signal`): per sample the position
    it is aligned to, -1 in the start / end states.  None for localpen / minscore = LARGE_LOG_VAL."""
    cost, path = path_dev(*_stage(params, signal, siglen, "squiggle_match_path"), back_prob, localpen, minscore)
    return cost.cpu().numpy(), path.cpu().numpy()


class SquiggleMatch(torch.autograd.Function):
    """Autograd function of the squiggle-match cost on device tensors (squiggle_match.pyx:164-192).
    The forward keeps its lattice for the backward, which then runs only the backward sweep.
    The cost stays on the device."""
    @staticmethod
    def forward(ctx, params, signal, siglen, back_prob):
        back_prob = float(back_prob)
        ctx.back_prob = back_prob
        lattice = None
        if ctx.needs_input_grad[0]:
            lattice = _lib.workspace(lattice_bytes(params, signal), params.device, "squiggle_lattice", fresh=True)
        cost = cost_dev(params, signal, siglen, back_prob, lattice=lattice)
        ctx.lattice = lattice
        ctx.save_for_backward(params, signal, siglen)
        return cost.to(params.dtype)

    @staticmethod
    def backward(ctx, output_grads):
        params, signal, siglen = ctx.saved_tensors
        grad = grad_dev(params, signal, siglen, ctx.back_prob, lattice=ctx.lattice)
        ctx.lattice = None
        grad = grad.to(params.dtype)
        return grad * output_grads.unsqueeze(1).to(grad.device), None, None, None


squiggle_match_loss = SquiggleMatch.apply


# ---------------------------------------------------------------------------------------------------
# bin/predict_squiggle.py: sequences -> predicted squiggles
# ---------------------------------------------------------------------------------------------------
def predict_squiggle(model, sequences, alphabet=DEFAULT_ALPHABET):
    """The model's (`models.squiggle_predictor`) prediction for every sequence of a batch: per sequence its
    (len, 3) float32 array of level, log-scale and move logit (predict_squiggle.py:38-47, which calls the network
    one sequence at a time).  Sequences of different lengths go as zero-padded columns with their lengths -- one
    upload, one call of the network, one download -- and every column's rows are what that sequence gives alone."""
    embedded = [embed_sequence(seq, alphabet) for seq in sequences]
    if not embedded:
        return []
    lens = np.array([len(e) for e in embedded], dtype=np.int32)
    x = np.zeros((max(int(lens.max()), 1), len(embedded), 3), dtype=np.float32)
    for n, e in enumerate(embedded):
        x[:len(e), n] = e
    param = next(model.parameters())
    with torch.no_grad():
        y = model(torch.from_numpy(x).to(device=param.device, dtype=param.dtype), lengths=lens).cpu().numpy()
    return [np.ascontiguousarray(y[:m, n], dtype=np.float32) for n, m in enumerate(lens)]


def write_predicted_squiggle(fh, sequence, squiggle):
    """The table of predict_squiggle.py:49-52: a header line, then per position the base, the level, exp(log-scale)
    and exp(-move logit), the numbers as numpy float32 values print."""
    if isinstance(sequence, (bytes, bytearray)):
        sequence = sequence.decode()
    fh.write('base\tcurrent\tsd\tdwell\n')
    for base, (mean, logsd, dwell) in zip(sequence, np.asarray(squiggle, dtype=np.float32)):
        fh.write('{}\t{}\t{}\t{}\n'.format(base, mean, np.exp(logsd), np.exp(-dwell)))

"""tk_lstm_forward_dev's saved tensors at the C ABI.  The forward kernel stages a step's h, c and gate activations in
LDS and stores them as whole rows of U units, 16 bytes per lane (csrc/lstm_kernels.hip, rows_to_global in
csrc/rnn_common.h), so what can go wrong is a row landing in the wrong place, a row not stored, and a wide store that
runs past a ragged column or past the last time step.

The shapes are the smallest that take each path: H 256 / N 5 is U = 64, C = 2 with a ragged last group (3 groups); H 256 /
N 130 is the C = 4 instantiation (33 groups of 4 workgroups, the last ragged); H 64 / N 3 and H 32 / N 9 are one workgroup per group; H 16 / N 9
has U = H = 16, rows of 4 chunks.  T = 1 is the epilogue's store alone, T = 2 has exactly one deferred store, T = 7 has
both parities of the staging block several times.

Values: y, gates and cell against the same layer in float64 that returns its activations, under the rule of
tests/test_lstm_hip.py: error over the tensor's largest entry <= 2 x MIOpen's own + 2e-6.  MIOpen returns y only, so
its y error is the allowance of all three: the gates and c are the operands y = o tanh(c) is computed from in one more
rounding, each taken over its own largest entry."""
import functools

import pytest
import torch

from taiyaki_amd import _lib, layers

pytestmark = pytest.mark.gpu

SHAPES = [(256, 5), (256, 130), (64, 3), (32, 9), (16, 9)]
STEPS = [1, 2, 7]
GUARD = 1024                     # floats in front of and behind every output
GUARD_BITS = 0x7FC0BEEF          # a quiet NaN with a payload: what the guards hold
SENTINEL = -77.0                 # no activation and no c of <= 7 steps


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _float64_lstm(x, w_ih, w_hh, b, reverse):
    """y (T, N, H), the gate activations i, f, g, o (T, N, 4H) and c (T, N, H) of one nn.LSTM layer, h0 = c0 = 0."""
    T, N, _ = x.shape
    H = w_hh.shape[1]
    h, c = x.new_zeros(N, H), x.new_zeros(N, H)
    y, gates, cell = x.new_zeros(T, N, H), x.new_zeros(T, N, 4 * H), x.new_zeros(T, N, H)
    for s in range(T):
        t = T - 1 - s if reverse else s
        a = x[t] @ w_ih.t() + h @ w_hh.t() + b
        i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 3 * H:])
        g = torch.tanh(a[:, 2 * H:3 * H])
        c = f * c + i * g
        h = o * torch.tanh(c)
        y[t], cell[t], gates[t] = h, c, torch.cat([i, f, g, o], 1)
    return y, gates, cell


@functools.lru_cache(maxsize=None)
def _case(H, N, T):
    """One layer at its own initialisation, its input, and the float64 tensors of both directions (computed once)."""
    torch.manual_seed(1000 * H + 10 * N + T)
    rnn = layers.Lstm(H, H).rnn
    x = torch.randn(T, N, H)
    w_ih, w_hh = rnn.weight_ih_l0.detach().double(), rnn.weight_hh_l0.detach().double()
    b = (rnn.bias_ih_l0 + rnn.bias_hh_l0).detach().double()
    ref = {rev: _float64_lstm(x.double(), w_ih, w_hh, b, rev) for rev in (0, 1)}
    return rnn, x, ref


def _guarded(shape, dev, shift):
    """A tensor of `shape` filled with SENTINEL between two guards; shift floats off the allocation's alignment."""
    n = 1
    for d in shape:
        n *= d
    flat = torch.full((GUARD + shift + n + GUARD,), GUARD_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    body = flat[GUARD + shift:GUARD + shift + n]
    body.fill_(SENTINEL)
    return flat, body.view(shape)


def _guards_intact(flat, shift, n):
    bits = flat.view(torch.int32)
    return bool((bits[:GUARD + shift] == GUARD_BITS).all()) and bool((bits[GUARD + shift + n:] == GUARD_BITS).all())


def _forward(gx, whh, rev, shift=0):
    """tk_lstm_forward_dev into guarded, sentinel-filled buffers; asserts the bounds and returns y, gates, cell."""
    T, N, H4 = gx.shape
    H, dev, L = H4 // 4, gx.device, _lib.lib()
    wsb = L.tk_lstm_workspace_bytes(N, H, _cus(dev))
    assert wsb > 0
    bufs = [_guarded(s, dev, shift) for s in ((T, N, H), (T, N, 4 * H), (T, N, H))]
    (_, y), (_, gates), (_, cell) = bufs
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.tk_lstm_forward_dev(_lib.ptr(gx), _lib.ptr(whh), T, N, H, rev, _cus(dev), _lib.ptr(y), _lib.ptr(gates),
                               _lib.ptr(cell), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr())
    _lib.check(rc, "tk_lstm_forward_dev")
    torch.cuda.synchronize()
    assert int(status.item()) == 0, int(status.item())
    for name, (flat, body) in zip(("y", "gates", "cell"), bufs):
        assert _guards_intact(flat, shift, body.numel()), (name, "a store outside the tensor")
        unwritten = int((body == SENTINEL).sum().item())
        assert unwritten == 0, (name, "elements not stored", unwritten)
        assert bool(torch.isfinite(body).all()), name
    return y, gates, cell


def _inputs(H, N, T, dev):
    rnn, x, ref = _case(H, N, T)
    w_ih, w_hh = rnn.weight_ih_l0.detach().to(dev), rnn.weight_hh_l0.detach().to(dev).contiguous()
    b = (rnn.bias_ih_l0 + rnn.bias_hh_l0).detach().to(dev)
    gx = (x.to(dev) @ w_ih.t() + b).contiguous()
    return rnn, x, ref, gx, w_hh


def _miopen_y(rnn, x, rev, dev):
    import copy
    m = copy.deepcopy(rnn).to(dev)
    with torch.no_grad():
        xin = x.to(dev)
        return torch.flip(m(torch.flip(xin, (0,)))[0], (0,)) if rev else m(xin)[0]


def _rel(a, ref):
    return (a.double().cpu() - ref).abs().max().item() / (ref.abs().max().item() or 1.0)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("H,N", SHAPES)
def test_saved_tensors_match_float64_inside_their_bounds(gpu_device, H, N, T, rev):
    rnn, x, ref, gx, w_hh = _inputs(H, N, T, gpu_device)
    got = _forward(gx, w_hh, rev)
    e_mio = _rel(_miopen_y(rnn, x, rev, gpu_device), ref[rev][0])
    for name, a, r in zip(("y", "gates", "cell"), got, ref[rev]):
        e = _rel(a, r)
        print("H %d N %d T %d rev %d %s: error %.3e, MIOpen's y %.3e" % (H, N, T, rev, name, e, e_mio))
        assert e <= 2 * e_mio + 2e-6, (H, N, T, rev, name, e, e_mio)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("H,N,T", [(256, 5, 7), (256, 130, 2), (16, 9, 7)])
def test_two_calls_give_the_same_bits(gpu_device, H, N, T, rev):
    _, _, _, gx, w_hh = _inputs(H, N, T, gpu_device)
    a, b = _forward(gx, w_hh, rev), _forward(gx, w_hh, rev)
    for name, p, q in zip(("y", "gates", "cell"), a, b):
        assert torch.equal(p, q), name


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("H,N,T", [(256, 5, 7), (16, 9, 2)])
def test_outputs_one_float_off_16_byte_alignment(gpu_device, H, N, T, rev):
    """The ABI asks for float tensors, not 16-byte aligned ones: the same bits, and the same bounds, 4 bytes on."""
    _, _, _, gx, w_hh = _inputs(H, N, T, gpu_device)
    a, b = _forward(gx, w_hh, rev), _forward(gx, w_hh, rev, shift=1)
    assert b[0].data_ptr() % 16 == 4
    for name, p, q in zip(("y", "gates", "cell"), a, b):
        assert torch.equal(p, q), name


def test_backward_consumes_what_the_forward_saved(gpu_device):
    """layers.Lstm forward and backward at H 256 / N 5 / T 7: dx and the weight gradients against the float64 layer."""
    T, N, H = 7, 5, 256
    torch.manual_seed(21)
    lstm = layers.Lstm(H, H)
    x, dy = torch.randn(T, N, H), torch.randn(T, N, H) / (T * N) ** 0.5

    def grads(layer, x, dy):
        x = x.detach().clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        (layer(x) * dy).sum().backward()
        out = {"x": x.grad, "w_ih": layer.rnn.weight_ih_l0.grad, "w_hh": layer.rnn.weight_hh_l0.grad,
               "b_ih": layer.rnn.bias_ih_l0.grad}
        return {k: v.detach().clone() for k, v in out.items()}

    ref = grads(lstm.double(), x.double(), dy.double())
    lstm = lstm.float().to(gpu_device)
    assert layers.hip_lstm_workspace_bytes(lstm.rnn, x.to(gpu_device)) > 0
    hip = grads(lstm, x.to(gpu_device), dy.to(gpu_device))
    old = layers.USE_HIP_LSTM
    try:
        layers.USE_HIP_LSTM = False
        miopen = grads(lstm, x.to(gpu_device), dy.to(gpu_device))
    finally:
        layers.USE_HIP_LSTM = old
    for k, r in ref.items():
        e_hip, e_mio = _rel(hip[k], r), _rel(miopen[k], r)
        print("d%s: error %.3e, MIOpen's %.3e" % (k, e_hip, e_mio))
        assert e_hip <= 2 * e_mio + 2e-6, (k, e_hip, e_mio)

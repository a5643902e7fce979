"""The LSTM forward that saves nothing at hidden sizes 192 and 384 on the matrix cores
(include/taiyaki_amd_lstm_matrix_sizes.h, csrc/lstm_matrix_sizes.hip, the "matrix_sizes" row of layers._rnn_route): groups
of size / 32 workgroups that hand h to each other.  Against nn.LSTM in float64 by the rule of tests/test_lstm_hip.py, bit
for bit across batch widths, places in a group, per-column lengths and slabs, and the route by width, grad mode and
switch."""
import copy

import pytest
import torch

from taiyaki_amd import _lib, layers

SIZES = (192, 384)
COLUMNS = {H: _lib.lstm_matrix_sizes_lib().tk_lstm_matrix_sizes_columns(H) for H in SIZES}
pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("H", SIZES), pytest.mark.parametrize("reverse", [False, True])]


def _run(gx, whh, lens, reverse, cus=None):
    """tk_lstm_matrix_sizes_forward_dev -> y, which starts as NaN: a row the kernel does not write shows.  The workspace
    is what the query asks for at this call; the status word must stay 0."""
    T, N, H = gx.shape[0], gx.shape[1], whh.shape[1]
    gx, dev = gx.contiguous(), gx.device
    L = _lib.lstm_matrix_sizes_lib()
    cus = cus or layers._cu_count(dev)
    wsb = L.tk_lstm_matrix_sizes_workspace_bytes(N, H, cus)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    y = torch.full((T, N, H), float("nan"), device=dev)
    with torch.cuda.device(dev):
        rc = L.tk_lstm_matrix_sizes_forward_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(lens), T, N, H, int(reverse), cus,
                                                _lib.ptr(y), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
    assert status.item() == 0
    return y


@pytest.mark.parametrize("shape", ["1x1", "3xC", "5xC+1", "37x2C+1", "800x16"])
def test_entry_and_layer_match_float64(gpu_device, monkeypatch, H, reverse, shape):
    """(3, C): one full group; (5, C + 1): a second group with one live column; (800, 16): the longest chunk, where the
    split's error would accumulate.  The error over the largest entry is at most 2 x nn.LSTM's on the device + 2e-6."""
    dev, C = gpu_device, COLUMNS[H]
    T, N = int(shape.split("x")[0]), {"1": 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1, "16": 16}[shape.split("x")[1]]
    monkeypatch.setattr(layers, "LSTM_MATRIX_SIZES_MIN_COLUMNS", {H: 1})
    monkeypatch.setattr(layers, "USE_HIP_LSTM_MATRIX_SIZES", True)
    torch.manual_seed(T + N)
    lstm = layers.Lstm(20, H)
    x = torch.randn(T, N, 20)
    l64 = copy.deepcopy(lstm).double()
    with torch.no_grad():
        ref = l64(x.double(), reverse=reverse)
        gx64 = x.double() @ l64.rnn.weight_ih_l0.t() + l64.rnn.bias_ih_l0 + l64.rnn.bias_hh_l0
        lstm, xd = lstm.to(dev), x.to(dev)
        before = layers.lstm_matrix_sizes_calls["inference"], dict(layers.rnn_wide_calls)
        y = lstm(xd, reverse=reverse)
        assert (layers.lstm_matrix_sizes_calls["inference"], layers.rnn_wide_calls) == (before[0] + 1, before[1])
        monkeypatch.setattr(layers, "USE_HIP_LSTM", False)
        miopen = lstm(xd, reverse=reverse)
    entry = _run(gx64.float().to(dev), lstm.rnn.weight_hh_l0.detach(), None, reverse)
    scale = ref.abs().max().item()
    e_mio = (miopen.double().cpu() - ref).abs().max().item() / scale
    for what, got in (("layer", y), ("entry", entry)):
        err = (got.double().cpu() - ref).abs().max().item() / scale
        print("H %d T %d N %d rev %d %s: matrix_sizes %.3e, nn.LSTM %.3e" % (H, T, N, reverse, what, err, e_mio))
        assert err <= 2 * e_mio + 2e-6, (what, err, e_mio)


def _case(T, N, H, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, N, 4 * H, generator=g).to(dev), (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)


def test_a_column_is_the_same_bits_alone_and_at_another_place(gpu_device, H, reverse):
    T, N = 23, 2 * COLUMNS[H] + 5
    gx, whh = _case(T, N, H, gpu_device, 11)
    batch = _run(gx, whh, None, reverse)
    assert torch.isfinite(batch).all() and batch.abs().max() > 0.1
    for n in range(N):
        assert torch.equal(_run(gx[:, n:n + 1], whh, None, reverse), batch[:, n:n + 1]), n
    moved = torch.roll(gx, 5, dims=1)       # column n at place (n + 5) % N: another place, for some another group
    assert torch.equal(torch.roll(_run(moved, whh, None, reverse), -5, dims=1), batch)


def test_lengths(gpu_device, H, reverse):
    dev, T = gpu_device, 41
    # C + 3 columns: a second group with three, two of them live
    lengths = [T, 0, 1, T // 2, T - 1, T] + [7] * (COLUMNS[H] - 5) + [0, 33]
    N = len(lengths)
    gx, whh = _case(T, N, H, dev, 12)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    beyond = torch.arange(T, device=dev)[:, None] >= lens[None, :]
    dirty = gx.clone()
    dirty[beyond] = float("nan")
    got = _run(dirty, whh, lens, reverse)
    assert torch.isfinite(got).all(), "a NaN beyond a length reached the output"
    assert not got[beyond].any(), "rows at and beyond the length are 0"
    assert torch.equal(got, _run(gx, whh, lens, reverse))
    for n, ln in enumerate(lengths):
        if ln:
            assert torch.equal(_run(gx[:ln, n:n + 1], whh, None, reverse), got[:ln, n:n + 1]), n
    full = torch.full((N,), T, dtype=torch.int32, device=dev)
    assert torch.equal(_run(gx, whh, None, reverse), _run(gx, whh, full, reverse))


@pytest.mark.parametrize("with_lengths", [False, True])
def test_slabs_are_the_bits_of_one_launch(gpu_device, H, reverse, with_lengths):
    """H / 32 CUs: one group per launch, so 2 C + 3 columns are three launches on windows of the tensors."""
    dev, C = gpu_device, COLUMNS[H]
    assert _lib.lstm_matrix_sizes_lib().tk_lstm_matrix_sizes_slab(H, H // 32) == C
    T, N = 9, 2 * C + 3
    gx, whh = _case(T, N, H, dev, 13)
    lens = None
    if with_lengths:
        lens = (torch.arange(N, dtype=torch.int32) * 7 % (T + 1)).to(dev)
    one = _run(gx, whh, lens, reverse)
    assert torch.isfinite(one).all()
    assert torch.equal(_run(gx, whh, lens, reverse, cus=H // 32), one)


@pytest.mark.parametrize("how,taken", [("at", True), ("below", False), ("grad", False), ("off", False)])
def test_route(gpu_device, monkeypatch, H, reverse, how, taken):
    """At the threshold under no_grad the layer, with and without lengths, and forward_varlen take the new row; one
    column fewer, grad mode and the switch off each go where they went: the main library (with lengths its counter
    moves), never the slabs."""
    dev = gpu_device
    monkeypatch.setattr(layers, "LSTM_MATRIX_SIZES_MIN_COLUMNS", {H: 20})
    monkeypatch.setattr(layers, "USE_HIP_LSTM_MATRIX_SIZES", how != "off")
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    torch.manual_seed(1)
    lstm = layers.Lstm(12, H).to(dev)
    N = 19 if how == "below" else 20
    x = torch.randn(6, N, 12, device=dev)
    counters = (layers.lstm_matrix_sizes_calls, layers.rnn_wide_calls, layers.rnn_varlen_calls,
                layers.lstm_matrix_group_calls, layers.lstm_matrix_calls)
    before = [sum(c.values()) for c in counters]
    with torch.enable_grad() if how == "grad" else torch.no_grad():
        y = lstm(x, reverse=reverse)
        yl = lstm(x, reverse=reverse, lengths=[6] * N)
        yv = layers.forward_varlen(layers.Serial([layers.Reverse(lstm) if reverse else lstm]), x, [6] * N)[0]
    assert torch.isfinite(y).all() and (y - yl).abs().max().item() < 1e-5 and (y - yv).abs().max().item() < 1e-5
    moved = [sum(c.values()) - b for c, b in zip(counters, before)]
    if taken:
        assert moved == [3, 0, 0, 0, 0] and torch.equal(y, yl), (how, moved)
    else:
        assert moved[:2] == [0, 0] and moved[2] >= 1 and moved[3:] == [0, 0], (how, moved)

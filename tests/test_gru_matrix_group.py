"""The GRU forward that saves nothing at hidden size 256 on the matrix cores (include/taiyaki_amd_gru_matrix_group.h,
csrc/gru_matrix_group.hip, the "gru_matrix_group" row of layers._rnn_route): groups of workgroups that hand h to each
other.  Against nn.GRU in float64 by the rule of tests/test_gru_hip.py, bit for bit across batch widths, places in a
group, per-column lengths and slabs, and the route by width, grad mode and switch."""
import copy

import pytest
import torch

from taiyaki_amd import _lib, layers

H = 256
C = _lib.gru_matrix_group_lib().tk_gru_matrix_group_columns(H)
G = 256 // (_lib.gru_matrix_group_lib().tk_gru_matrix_group_slab(H, 256) // C)


def _run(gx, whh, bhh, lens, reverse, cus=None):
    """tk_gru_matrix_group_forward_dev -> y, which starts as NaN: a row the kernel does not write shows.  The workspace
    is what the query asks for at this call; the status word must stay 0."""
    T, N, _ = gx.shape
    gx, dev = gx.contiguous(), gx.device
    L, cus = _lib.gru_matrix_group_lib(), cus or layers._cu_count(dev)
    wsb = L.tk_gru_matrix_group_workspace_bytes(N, H, cus)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    y = torch.full((T, N, H), float("nan"), device=dev)
    with torch.cuda.device(dev):
        rc = L.tk_gru_matrix_group_forward_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(bhh), _lib.ptr(lens), T, N, H,
                                               int(reverse), cus, _lib.ptr(y), _lib.ptr(ws), wsb, _lib.ptr(status),
                                               _lib.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
    assert status.item() == 0
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(1, 1), (3, C), (5, C + 1), (37, 2 * C + 1), (800, 16)])
@pytest.mark.parametrize("reverse", [False, True])
def test_entry_and_layer_match_float64(gpu_device, monkeypatch, T, N, reverse):
    """(3, C): one full group; (5, C + 1): a second group with one live column; (800, 16): the longest chunk, where the
    split's error would accumulate.  b_hh is live, so bhh_n's place inside the reset product counts.  The error over the
    largest entry is at most 2 x nn.GRU's on the device + 2e-6."""
    dev = gpu_device
    monkeypatch.setattr(layers, "GRU_MATRIX_GROUP_MIN_COLUMNS", 1)
    monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX_GROUP", True)
    torch.manual_seed(T + N)
    gru = layers.GruMod(20, H)
    with torch.no_grad():
        gru.rnn.bias_hh_l0.normal_(0.0, 0.5)
    x = torch.randn(T, N, 20)
    g64 = copy.deepcopy(gru).double()
    with torch.no_grad():
        ref = g64(x.double(), reverse=reverse)
        gx64 = x.double() @ g64.rnn.weight_ih_l0.t() + g64.rnn.bias_ih_l0
        gru, xd = gru.to(dev), x.to(dev)
        before = layers.gru_matrix_group_calls["inference"], dict(layers.rnn_wide_calls)
        y = gru(xd, reverse=reverse)
        assert (layers.gru_matrix_group_calls["inference"], layers.rnn_wide_calls) == (before[0] + 1, before[1])
        monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX_GROUP", False)
        monkeypatch.setattr(layers, "USE_HIP_GRU", False)
        miopen = gru(xd, reverse=reverse)
        assert layers.gru_matrix_group_calls["inference"] == before[0] + 1
    entry = _run(gx64.float().to(dev), gru.rnn.weight_hh_l0.detach(), gru.rnn.bias_hh_l0.detach(), None, reverse)
    scale = ref.abs().max().item()
    e_mio = (miopen.double().cpu() - ref).abs().max().item() / scale
    for what, got in (("layer", y), ("entry", entry)):
        err = (got.double().cpu() - ref).abs().max().item() / scale
        print("T %d N %d rev %d %s: matrix_group %.3e, nn.GRU %.3e" % (T, N, reverse, what, err, e_mio))
        assert err <= 2 * e_mio + 2e-6, (what, err, e_mio)


def _case(T, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, N, 3 * H, generator=g).to(dev), (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(dev),
            (0.5 * torch.randn(3 * H, generator=g)).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_a_column_is_the_same_bits_alone_and_at_another_place(gpu_device, reverse):
    T, N = 23, 2 * C + 5
    gx, whh, bhh = _case(T, N, gpu_device, 11)
    batch = _run(gx, whh, bhh, None, reverse)
    assert torch.isfinite(batch).all() and batch.abs().max() > 0.1
    for n in range(N):
        assert torch.equal(_run(gx[:, n:n + 1], whh, bhh, None, reverse), batch[:, n:n + 1]), n
    moved = torch.roll(gx, 5, dims=1)       # column n at place (n + 5) % N: another place, for some another group
    assert torch.equal(torch.roll(_run(moved, whh, bhh, None, reverse), -5, dims=1), batch)


VT, VLENS = 41, [41, 0, 1, 20, 40, 41] + [7] * (C - 5) + [0, 33]        # C + 3 columns: a second group with three, two of them live


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_lengths(gpu_device, reverse):
    dev = gpu_device
    N = len(VLENS)
    gx, whh, bhh = _case(VT, N, dev, 12)
    lens = torch.tensor(VLENS, dtype=torch.int32, device=dev)
    beyond = torch.arange(VT, device=dev)[:, None] >= lens[None, :]
    dirty = gx.clone()
    dirty[beyond] = float("nan")
    got = _run(dirty, whh, bhh, lens, reverse)
    assert torch.isfinite(got).all(), "a NaN beyond a length reached the output"
    assert not got[beyond].any(), "rows at and beyond the length are 0"
    assert torch.equal(got, _run(gx, whh, bhh, lens, reverse))
    for n, ln in enumerate(VLENS):
        if ln:
            assert torch.equal(_run(gx[:ln, n:n + 1], whh, bhh, None, reverse), got[:ln, n:n + 1]), n
    full = torch.full((N,), VT, dtype=torch.int32, device=dev)
    assert torch.equal(_run(gx, whh, bhh, None, reverse), _run(gx, whh, bhh, full, reverse))


@pytest.mark.gpu
@pytest.mark.parametrize("with_lengths", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_slabs_are_the_bits_of_one_launch(gpu_device, reverse, with_lengths):
    """G CUs: one group per launch, so 2 C + 3 columns are three launches on windows of the tensors."""
    assert _lib.gru_matrix_group_lib().tk_gru_matrix_group_slab(H, G) == C
    T, N = 9, 2 * C + 3
    gx, whh, bhh = _case(T, N, gpu_device, 13)
    lens = (torch.arange(N, dtype=torch.int32) * 7 % (T + 1)).to(gpu_device) if with_lengths else None
    one = _run(gx, whh, bhh, lens, reverse)
    assert torch.isfinite(one).all()
    assert torch.equal(_run(gx, whh, bhh, lens, reverse, cus=G), one)


@pytest.mark.gpu
@pytest.mark.parametrize("how,group", [("at", True), ("below", False), ("grad", False), ("off", False)])
def test_route(gpu_device, monkeypatch, how, group):
    """At the threshold under no_grad the layer, with and without lengths, and forward_varlen take the new row; one
    column fewer, grad mode and the switch off each go where they went: the main library, never the slabs."""
    dev = gpu_device
    monkeypatch.setattr(layers, "GRU_MATRIX_GROUP_MIN_COLUMNS", 20)
    monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX_GROUP", how != "off")
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    torch.manual_seed(1)
    gru = layers.GruMod(12, H).to(dev)
    N = 19 if how == "below" else 20
    x = torch.randn(6, N, 12, device=dev)
    counters = (layers.gru_matrix_group_calls, layers.rnn_wide_calls, layers.rnn_varlen_calls)
    before = [sum(c.values()) for c in counters]
    with torch.enable_grad() if how == "grad" else torch.no_grad():
        y = gru(x)
        yl = gru(x, lengths=[6] * N)
        yv = layers.forward_varlen(layers.Serial([gru]), x, [6] * N)[0]
    assert torch.isfinite(y).all() and (y - yl).abs().max().item() < 1e-5 and (y - yv).abs().max().item() < 1e-5
    moved = [sum(c.values()) - b for c, b in zip(counters, before)]
    if group:
        assert moved == [3, 0, 0] and torch.equal(y, yl), (how, moved)
    else:
        assert moved[:2] == [0, 0] and moved[2] >= 1, (how, moved)

"""The recurrences' forward with per-column lengths (include/taiyaki_amd_rnn_varlen.h) at the C ABI: every column's
rows against the existing forward (tk_lstm_forward_dev / tk_gru_forward_dev) run on that column alone at its own
length, the rows beyond exactly 0, and lengths = NULL against the existing forward on the whole batch, bit for bit.
y is filled with NaN before every launch: an unwritten row shows."""
import ctypes

import pytest
import torch

from taiyaki_amd import _lib

pytestmark = pytest.mark.gpu


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _finish(rc, status, what):
    _lib.check(rc, what)
    torch.cuda.synchronize()
    assert int(status.item()) == 0, (what, int(status.item()))


def _lstm_saving(gx, whh, rev):
    """tk_lstm_forward_dev's y."""
    T, N, H4 = gx.shape
    H, dev, L = H4 // 4, gx.device, _lib.lib()
    wsb = L.tk_lstm_workspace_bytes(N, H, _cus(dev))
    assert wsb > 0
    y = torch.full((T, N, H), float("nan"), device=dev)
    gates, cell = torch.empty(T, N, 4 * H, device=dev), torch.empty(T, N, H, device=dev)
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.tk_lstm_forward_dev(_lib.ptr(gx), _lib.ptr(whh), T, N, H, rev, _cus(dev), _lib.ptr(y), _lib.ptr(gates),
                               _lib.ptr(cell), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr())
    _finish(rc, status, "tk_lstm_forward_dev")
    return y


def _gru_saving(gx, whh, bhh, rev):
    """tk_gru_forward_dev's y."""
    T, N, H3 = gx.shape
    H, dev, L = H3 // 3, gx.device, _lib.lib()
    wsb = L.tk_gru_workspace_bytes(N, H, _cus(dev))
    assert wsb > 0
    y = torch.full((T, N, H), float("nan"), device=dev)
    gates, q = torch.empty(T, N, 3 * H, device=dev), torch.empty(T, N, H, device=dev)
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.tk_gru_forward_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(bhh), T, N, H, rev, _cus(dev), _lib.ptr(y),
                              _lib.ptr(gates), _lib.ptr(q), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr())
    _finish(rc, status, "tk_gru_forward_dev")
    return y


def _varlen(kind, gx, whh, bhh, lengths, rev):
    """tk_lstm_forward_varlen_dev / tk_gru_forward_varlen_dev: y, NaN before the launch."""
    T, N, HG = gx.shape
    lstm = kind == "lstm"
    H, dev, V = HG // (4 if lstm else 3), gx.device, _lib.varlen_lib()
    wsb = V.tk_rnn_varlen_workspace_bytes(_lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM" if lstm else "TK_RNN_KIND_GRU"], N, H,
                                          _cus(dev))
    assert wsb > 0
    y = torch.full((T, N, H), float("nan"), device=dev)
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    tail = (T, N, H, rev, _cus(dev), _lib.ptr(y), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr())
    if lstm:
        rc = V.tk_lstm_forward_varlen_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(lens), *tail)
    else:
        rc = V.tk_gru_forward_varlen_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(bhh), _lib.ptr(lens), *tail)
    _finish(rc, status, "tk_%s_forward_varlen_dev" % kind)
    return y


def _lstm_same_geometry(n, h, cus):
    """Do the launches at n columns and at 1 column have the same (U, C)?  (tk_lab_lstm_geometry, the lab library)"""
    L = _lib.use_lab(True)
    try:
        plans = []
        for cols in (n, 1):
            out = (ctypes.c_size_t * 8)()
            assert L.tk_lab_lstm_geometry(cols, h, cus, out)
            plans.append((out[2], out[3]))
    finally:
        _lib.use_lab(False)
    return plans[0] == plans[1]


def _check_columns(y, alone, lengths, columns, exact, what):
    """Rows [0, len) of every column in `columns` against alone(n, len); rows [len, T) exactly 0."""
    for n in columns:
        ln = lengths[n]
        assert torch.equal(y[ln:, n], torch.zeros_like(y[ln:, n])), (what, n, "rows beyond the length")
        if ln == 0:
            continue
        a, b = y[:ln, n], alone(n, ln)[:, 0]
        assert torch.isfinite(a).all(), (what, n)
        if exact:
            assert torch.equal(a, b), (what, n, (a - b).abs().max().item())
        else:
            err, bound = (a - b).abs().max().item(), 1e-5 * a.abs().max().item()
            print("%s column %d: max|a - b| %.3g, bound %.3g" % (what, n, err, bound))
            assert err <= bound, (what, n, err, bound)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("H", [64, 256])
def test_lstm_columns_equal_the_column_run_alone(gpu_device, H, rev):
    T, N, lengths = 37, 5, [37, 1, 0, 20, 36]
    g = torch.Generator().manual_seed(100 + H + rev)
    gx = torch.randn(T, N, 4 * H, generator=g).to(gpu_device)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(gpu_device)
    y = _varlen("lstm", gx, whh, None, lengths, rev)
    exact = _lstm_same_geometry(N, H, _cus(gpu_device))
    _check_columns(y, lambda n, ln: _lstm_saving(gx[:ln, n:n + 1].contiguous(), whh, rev), lengths, range(N), exact,
                   "lstm H %d rev %d" % (H, rev))


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("H,N,T,lengths", [(96, 5, 41, [41, 1, 0, 20, 40]), (256, 6, 23, [23, 0, 1, 12, 22, 23])])
def test_gru_columns_equal_the_column_run_alone(gpu_device, H, N, T, lengths, rev):
    """One column per workgroup at H 96 (both launches), groups of four workgroups with 4 columns at H 256 (both
    launches): the same (U, C) on either side, so bit for bit."""
    g = torch.Generator().manual_seed(200 + H + rev)
    gx = torch.randn(T, N, 3 * H, generator=g).to(gpu_device)
    whh = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(gpu_device)
    bhh = (0.3 * torch.randn(3 * H, generator=g)).to(gpu_device)
    y = _varlen("gru", gx, whh, bhh, lengths, rev)
    _check_columns(y, lambda n, ln: _gru_saving(gx[:ln, n:n + 1].contiguous(), whh, bhh, rev), lengths, range(N), True,
                   "gru H %d rev %d" % (H, rev))


@pytest.mark.parametrize("rev", [0, 1])
def test_gru_two_columns_per_workgroup(gpu_device, rev):
    """More columns than CUs: 2 columns per workgroup, against the 1-column launch of a column alone (not the same
    (U, C): the rounding-level rule)."""
    H, T = 96, 8
    N = _cus(gpu_device) + 44
    lengths = [n % 9 for n in range(N)]
    g = torch.Generator().manual_seed(300 + rev)
    gx = torch.randn(T, N, 3 * H, generator=g).to(gpu_device)
    whh = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(gpu_device)
    bhh = (0.3 * torch.randn(3 * H, generator=g)).to(gpu_device)
    y = _varlen("gru", gx, whh, bhh, lengths, rev)
    assert torch.isfinite(y).all()
    for n in range(N):
        assert torch.equal(y[lengths[n]:, n], torch.zeros_like(y[lengths[n]:, n])), n
    sample = sorted({0, 1, 7, 8, 16, 17, 26, 35, 100, 101, N // 2, N // 2 + 1, N - 4, N - 3, N - 2, N - 1})
    assert len(sample) == 16
    _check_columns(y, lambda n, ln: _gru_saving(gx[:ln, n:n + 1].contiguous(), whh, bhh, rev), lengths, sample, False,
                   "gru C 2 rev %d" % rev)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("kind,H,N,T", [("lstm", 64, 5, 37), ("lstm", 256, 5, 37), ("gru", 96, 5, 41),
                                        ("gru", 256, 6, 23)])
def test_null_lengths_equal_the_existing_forward(gpu_device, kind, H, N, T, rev):
    ng = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(400 + H + rev)
    gx = torch.randn(T, N, ng * H, generator=g).to(gpu_device)
    whh = (torch.randn(ng * H, H, generator=g) / H ** 0.5).to(gpu_device)
    bhh = (0.3 * torch.randn(ng * H, generator=g)).to(gpu_device)
    want = _lstm_saving(gx, whh, rev) if kind == "lstm" else _gru_saving(gx, whh, bhh, rev)
    assert torch.equal(_varlen(kind, gx, whh, bhh, None, rev), want)
    assert torch.equal(_varlen(kind, gx, whh, bhh, [T] * N, rev), want)

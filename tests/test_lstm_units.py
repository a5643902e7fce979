"""The LSTM recurrence at U = 16, 32 and 64 hidden units per workgroup (csrc/lstm_kernels.hip, lstm_plan): every
geometry against float64, the geometries against each other, run-to-run and captured-replay bit identity, and (CPU)
the launch plan inside the admitted grid and workspace."""
import ctypes

import pytest
import torch

from taiyaki_amd import _lib, layers
from tests.test_lstm_hip import _compare, _grads


def _plan(L, n, h, cus):
    out = (ctypes.c_size_t * 8)()
    if not L.tk_lab_lstm_geometry(n, h, cus, out):
        return None
    return dict(zip(["C16", "groups16", "U", "C", "groups", "grid", "fwd_bytes", "bwd_bytes"], list(out)))


class _units:
    """The lab build with the units per workgroup forced (0 = the release rule)."""

    def __init__(self, u):
        self.u = u

    def __enter__(self):
        self.L = _lib.use_lab(True)
        self.L.tk_lab_lstm_units(self.u)
        return self.L

    def __exit__(self, *exc):
        self.L.tk_lab_lstm_units(0)
        _lib.use_lab(False)


def test_plan_stays_inside_the_admitted_grid_and_workspace():
    L = _lib.use_lab(True)
    try:
        for cus in (8, 32, 64, 128, 256, 304):
            for h in (16, 32, 64, 128, 256):
                for n in (1, 2, 3, 5, 7, 8, 9, 31, 64, 100, 127, 128, 129, 171, 200, 256, 300, 511, 512):
                    ws = L.tk_lstm_workspace_bytes(n, h, cus)
                    for u in (0, 16, 32, 64):
                        L.tk_lab_lstm_units(u)
                        p = _plan(L, n, h, cus)
                        assert (p is not None) == (ws > 0), (n, h, cus, u)
                        if p is None:
                            continue
                        want = min(u or 64, h)
                        assert p["U"] == want and p["C"] * p["U"] == 16 * p["C16"], (n, h, cus, u, p)
                        assert p["groups"] * p["C"] >= n > (p["groups"] - 1) * p["C"], (n, h, cus, u, p)
                        assert p["grid"] == p["groups"] * (h // p["U"]) <= cus, (n, h, cus, u, p)
                        assert p["fwd_bytes"] <= p["bwd_bytes"] <= ws, (n, h, cus, u, p)
                    L.tk_lab_lstm_units(0)
        # the flagship layer: 64 groups of 2 columns x 4 workgroups at the release rule, a quarter of the U = 16 buffer
        p = _plan(L, 128, 256, 256)
        assert (p["U"], p["C"], p["groups"], p["grid"]) == (64, 2, 64, 256)
        assert p["bwd_bytes"] == 2 * 64 * 4 * 2 * 256 * 8 == L.tk_lstm_workspace_bytes(128, 256, 256) // 4
    finally:
        L.tk_lab_lstm_units(0)
        _lib.use_lab(False)


@pytest.mark.gpu
@pytest.mark.parametrize("units", [16, 32, 64])
@pytest.mark.parametrize("T,N,H,I", [(1, 5, 16, 7), (37, 5, 32, 16), (50, 6, 64, 32), (25, 70, 64, 20),
                                     (30, 37, 128, 16), (20, 130, 256, 256), (800, 128, 256, 256)])
@pytest.mark.parametrize("reverse", [False, True])
def test_each_geometry_matches_float64(gpu_device, units, T, N, H, I, reverse):
    with _units(units):
        _compare(T, N, H, I, reverse, gpu_device, seed=3 if T == 800 else T + N)      # (config 2: test_lstm_hip's seed)


def _layer_case(dev, T=60, N=40, I=64, H=256, seed=5):
    torch.manual_seed(seed)
    layer = layers.Reverse(layers.Lstm(I, H)).to(dev)
    return layer, torch.randn(T, N, I, device=dev), torch.randn(T, N, H, device=dev)


@pytest.mark.gpu
def test_geometries_agree_and_repeat_bit_identical(gpu_device):
    layer, x, dy = _layer_case(gpu_device)
    runs = {}
    for u in (16, 32, 64):
        with _units(u):
            runs[u] = _grads(layer, x, dy)
            again = _grads(layer, x, dy)
        for k in runs[u]:
            assert torch.equal(runs[u][k], again[k]), (u, k)
    for u in (32, 64):
        for k, a in runs[16].items():
            assert (runs[u][k] - a).abs().max().item() <= 1e-5 * a.abs().max().item(), (u, k)


@pytest.mark.gpu
def test_captured_train_step_replays_bit_identical_at_32_units(gpu_device):
    layer, x, dy = _layer_case(gpu_device, T=90, N=21, I=32, H=64, seed=7)
    x = x.requires_grad_(True)
    strict = _lib.is_strict()
    _lib.set_strict(False)
    try:
        with _units(32):
            def step():
                for p in layer.parameters():
                    p.grad = None
                x.grad = None
                y = layer(x)
                (y * dy).sum().backward()
                return y
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                eager = step().detach().clone()
                eager_dx = x.grad.detach().clone()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = step()
            for _ in range(3):
                out.fill_(float("nan"))
                x.grad.fill_(float("nan"))
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager)
                assert torch.equal(x.grad, eager_dx)
        _lib.raise_if_nonfinite()
    finally:
        _lib.set_strict(strict)

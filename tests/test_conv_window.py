"""Convolution(16 -> 96 ... 384, window 19 or 31, stride 5, 10 or 12, swish), the mLstm models' third layer at the fast and
the RNA models' shapes, on the kernels of libtaiyaki_amd_conv_window.so (include/taiyaki_amd_conv_window.h;
csrc/conv_strided.hip built -DTK_CONV_WINDOW) against nn.Conv1d + swish in float64 on the host, with the path it replaces
(pad + unfold + rocBLAS GEMM + element-wise kernels) as the yardstick: the criterion of tests/test_conv_strided.py, the
error relative to the largest reference entry at most twice the GEMM path's on the same inputs, plus 2e-6 -- for each
of y, dx, dW and db."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
from torch import nn

from taiyaki_amd import _lib, basecall, layers, models, synth

pytestmark = pytest.mark.gpu

CUS = 256
OK = 0
CIN, KB = 16, 16
GEOMETRIES = ((19, 5), (31, 10), (31, 12))
ADMITTED = (96, 128, 192, 256, 384)
# T per geometry: all padding but the centre (1), halos at both ends, T not a multiple of the stride (the dx crop),
# T >= 47: every r of the dx image with its absent taps, and 129 windows: the next 128-row tile at N = 1
TIMES = {(19, 5): (1, 4, 5, 6, 9, 10, 19, 23, 641), (31, 10): (1, 9, 10, 11, 15, 16, 31, 47, 1281),
         (31, 12): (1, 11, 12, 13, 15, 16, 31, 47, 1537)}
MID = {(19, 5): 23, (31, 10): 47, (31, 12): 47}
PLAN_KEYS = ("tiles_m", "f_tiles_n", "f_nkb", "f_grid", "d_tiles_n", "d_nkb", "splits", "nsub", "run_rows", "sub_rows",
             "w_grid", "bytes")
ALL_SHAPES = frozenset((c, w, s) for c in ADMITTED for w, s in GEOMETRIES)


def _owned_by_the_strided_library(cout, win, stride):
    return (win, stride) == (19, 5) and cout in (192, 256, 384)


def _grid():
    cases = []
    for win, stride in GEOMETRIES:
        for cout in (96, 256):
            cases += [(win, stride, cout, T, N) for T in TIMES[(win, stride)] for N in (1, 63, 65)]
        for cout in (128, 192, 384):
            cases += [(win, stride, cout, T, N) for T in (MID[(win, stride)], TIMES[(win, stride)][-1]) for N in (1, 65)]
    return [c for c in cases if not _owned_by_the_strided_library(c[2], c[0], c[1])]


def _cdiv(a, b):
    return -(-a // b)


def _plan(L, T, N, cout, win, stride, cus=CUS):
    out = (ctypes.c_size_t * 12)()
    if not L.tk_lab_conv_window_plan(T, N, cout, win, stride, cus, out):
        return None
    return dict(zip(PLAN_KEYS, out))


@pytest.fixture
def every_shape_in_grad_mode(monkeypatch):
    """the kernels at every shape of the rule in grad mode too, whatever the measured table holds"""
    monkeypatch.setattr(layers, "CONV_WINDOW_GRAD_SHAPES", ALL_SHAPES)


GUARD = 64


def _guarded(numel, dev):
    buf = torch.full((GUARD + numel + GUARD,), 7.0, device=dev)
    out = buf[GUARD:GUARD + numel]
    out.fill_(float("nan"))
    return buf, out


def _run(x, w, b, dy, stride, poison=0xFF, want_dx=True, want_z=True):
    """One forward and one backward call on device tensors.  Every output lies between two guard bands over a sentinel,
    the workspace is poisoned and of exactly the size asked; returns y, dx (or None), dw, db."""
    L = _lib.conv_window_lib()
    T, N, _ = x.shape
    cout, _, win = w.shape
    tout = _cdiv(T, stride)
    rows = tout * N
    dev = x.device
    wsb = L.tk_conv_window_workspace_bytes(T, N, cout, win, stride, CUS)
    assert wsb > 0
    ws = torch.full((wsb,), poison, dtype=torch.uint8, device=dev)
    sizes = dict(z=rows * cout, y=rows * cout, dz=rows * cout, dx=T * N * CIN, dw=cout * CIN * win, db=cout)
    bufs = {k: _guarded(n, dev) for k, n in sizes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    rc = L.tk_conv_window_forward_dev(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), T, N, cout, win, stride, CUS,
                                      _lib.ptr(o["z"] if want_z else None), _lib.ptr(o["y"]), _lib.ptr(ws), wsb,
                                      _lib.stream_ptr())
    assert rc == OK
    if want_z:
        ws.fill_(poison)
        rc = L.tk_conv_window_backward_dev(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(o["z"]), _lib.ptr(w), T, N, cout, win,
                                           stride, CUS, _lib.ptr(o["dz"]), _lib.ptr(o["dx"] if want_dx else None),
                                           _lib.ptr(o["dw"]), _lib.ptr(o["db"]), _lib.ptr(ws), wsb, _lib.stream_ptr())
        assert rc == OK
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert (buf[:GUARD] == 7.0).all() and (buf[GUARD + sizes[k]:] == 7.0).all(), "guard bands of " + k
    written = ["y"] + (["z", "dz", "dw", "db"] + (["dx"] if want_dx else []) if want_z else [])
    for k in sizes:
        if k in written:
            assert torch.isfinite(o[k]).all(), "every element of %s is written" % k
        else:
            assert torch.isnan(o[k]).all(), "%s is not touched" % k
    return dict(y=o["y"].view(tout, N, cout).clone(), dx=o["dx"].view(T, N, CIN).clone() if want_dx and want_z else None,
                dw=o["dw"].view(cout, CIN, win).clone(), db=o["db"].clone())


def _ref64(x, w, b, dy, stride):
    """nn.Conv1d + swish and their gradients, float64 on the host"""
    cout, _, win = w.shape
    conv = nn.Conv1d(CIN, cout, win, stride=stride).double()
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    x = x.double().requires_grad_(True)
    z = conv(nn.functional.pad(x.permute(1, 2, 0), (win // 2, (win - 1) // 2)))
    y = (z * torch.sigmoid(z)).permute(2, 0, 1)
    (y * dy.double()).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dw=conv.weight.grad, db=conv.bias.grad)


@functools.lru_cache(maxsize=None)
def _inputs(kind, win, stride, cout, T, N):
    """x, w, b, dy on the host (float32) and the float64 results.  `kind`: randn; cancel (x = 1 + 2^-10 randn against
    filters that sum to about 0, as tests/test_conv_strided.py builds it: away from the padding z is made of the
    correction terms)."""
    g = torch.Generator().manual_seed(11 * T + 5 * N + cout + 7 * stride + len(kind))
    tout = _cdiv(T, stride)
    x = torch.randn(T, N, CIN, generator=g)
    w = torch.randn(cout, CIN, win, generator=g) / (CIN * win) ** 0.5
    b = torch.randn(cout, generator=g)
    dy = torch.randn(tout, N, cout, generator=g) / (tout * N) ** 0.5
    if kind == "cancel":
        x = 1 + x * 2.0 ** -10
        w = w - w.mean((1, 2), keepdim=True)
        b = torch.zeros(cout)
    return x, w, b, dy, _ref64(x, w, b, dy, stride)


def _layer(cout, win, stride):
    return layers.Convolution(CIN, cout, win, stride=stride, fun=layers.swish)


def _with_weights(cout, win, stride, w, b, dev):
    layer = _layer(cout, win, stride).to(dev)
    with torch.no_grad():
        layer.conv.weight.copy_(w)
        layer.conv.bias.copy_(b)
    return layer


def _layer_grads(layer, x, dy, switch, name="USE_HIP_CONV_WINDOW"):
    old = getattr(layers, name)
    setattr(layers, name, switch)
    try:
        x = x.detach().clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        y = layer(x)
        (y * dy).sum().backward()
    finally:
        setattr(layers, name, old)
    return dict(y=y.detach().clone(), dx=x.grad, dw=layer.conv.weight.grad.clone(), db=layer.conv.bias.grad.clone())


def _gemm_path(x, w, b, dy, stride):
    """what the layer runs with the switch off, on the same device tensors"""
    cout, _, win = w.shape
    before = dict(layers.conv_window_calls)
    res = _layer_grads(_with_weights(cout, win, stride, w, b, x.device), x, dy, False)
    assert layers.conv_window_calls == before
    return res


def _rel(got, ref):
    return (got.double().cpu() - ref).abs().max().item() / (ref.abs().max().item() or 1.0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(kind, win, stride, cout, T, N, dev):
    x, w, b, dy, ref = _inputs(kind, win, stride, cout, T, N)
    x, w, b, dy = (v.to(dev) for v in (x, w, b, dy))
    got, gemm = _run(x, w, b, dy, stride), _gemm_path(x, w, b, dy, stride)
    for k in ("y", "dx", "dw", "db"):
        e_hip, e_gemm = _rel(got[k], ref[k]), _rel(gemm[k], ref[k])
        print("conv %s (win, stride, Cout, T, N) = %s %s: kernel %.3g, GEMM path %.3g" % (
            kind, (win, stride, cout, T, N), k, e_hip, e_gemm))
        assert e_hip <= 2 * e_gemm + 2e-6, (kind, win, stride, cout, T, N, k, e_hip, e_gemm)
    return got


@pytest.mark.parametrize("win,stride,cout,T,N", _grid())
def test_against_float64_with_the_gemm_path_as_yardstick(gpu_device, win, stride, cout, T, N):
    """Guard bands, every element written, the workspace poisoned and of exactly the size asked (_run); the column-tile
    edges: 96 and 192 channels inside a tile, 160 and 192 dx columns, 496 window columns."""
    _check("randn", win, stride, cout, T, N, gpu_device)


@pytest.mark.parametrize("cout", [96, 256])
@pytest.mark.parametrize("win,stride", [(31, 10), (31, 12)])
def test_the_cancelling_input(gpu_device, win, stride, cout):
    T, N = 128 * stride + 1, 65
    x, w, b, _, ref = _inputs("cancel", win, stride, cout, T, N)
    # ... cancels: in the interior z is below 1 % of the sum of the magnitudes of its products
    xp = nn.functional.pad(x.permute(1, 2, 0).double(), (win // 2, (win - 1) // 2))
    mags = nn.functional.conv1d(xp.abs(), w.double().abs(), stride=stride)
    z = nn.functional.conv1d(xp, w.double(), stride=stride)
    assert z[:, :, 2:-2].abs().max().item() < 1e-2 * mags[:, :, 2:-2].max().item()
    _check("cancel", win, stride, cout, T, N, gpu_device)


def test_two_runs_are_bit_identical_whatever_the_workspace_held(gpu_device):
    win, stride = 31, 10
    x, w, b, dy, _ = _inputs("randn", win, stride, 256, 1281, 65)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    one, two, three = _run(x, w, b, dy, stride), _run(x, w, b, dy, stride), _run(x, w, b, dy, stride, poison=0x3F)
    for k in one:
        assert torch.equal(_bits(one[k]), _bits(two[k])), k
        assert torch.equal(_bits(one[k]), _bits(three[k])), k


@pytest.mark.parametrize("win,stride", GEOMETRIES)
def test_a_column_alone_has_the_bits_it_has_in_a_batch(gpu_device, win, stride):
    T, N = 47, 65
    x, w, b, dy, _ = _inputs("randn", win, stride, 96, T, N)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    full = _run(x, w, b, dy, stride, want_z=False)["y"]
    for n in (0, 31, 64):
        alone = _run(x[:, n:n + 1].contiguous(), w, b, None, stride, want_z=False)["y"]
        assert torch.equal(_bits(alone), _bits(full[:, n:n + 1])), n


@pytest.mark.parametrize("win,stride,cout", [(31, 10, 96), (31, 12, 256)])
def test_without_dx_and_without_z(gpu_device, win, stride, cout):
    """dx NULL: dw and db keep their bits and dx is not touched; z NULL (the forward under no_grad): y keeps its bits."""
    x, w, b, dy, _ = _inputs("randn", win, stride, cout, 47, 63)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    full = _run(x, w, b, dy, stride)
    nodx, noz = _run(x, w, b, dy, stride, want_dx=False), _run(x, w, b, dy, stride, want_z=False)
    assert nodx["dx"] is None
    for k in ("y", "dw", "db"):
        assert torch.equal(_bits(full[k]), _bits(nodx[k])), k
    assert torch.equal(_bits(full["y"]), _bits(noz["y"]))


@pytest.mark.parametrize("win,stride,cout,T,N,splits,want", [
    (31, 10, 96, 1281, 100, 1, (1, 2)), (31, 10, 96, 1281, 65, 3, (3, 1)), (31, 12, 256, 47, 63, 1, (1, 1)),
    (19, 5, 96, 641, 100, 5, (5, 1))])
def test_forced_runs_and_chain_parts_of_the_weight_gradient(gpu_device, labenv, win, stride, cout, T, N, splits, want):
    """The lab hook forces the number of runs: one run of 12900 rows is cut into two chain parts, the last block
    ragged (12900 = 806 x 16 + 4); three runs of 8385 rows; one run and one part at 252 rows; five runs."""
    labenv.lib()
    L = _lib.conv_window_lib()
    assert _lib.is_lab()
    try:
        L.tk_lab_conv_window_set_splits(splits)
        plan = _plan(L, T, N, cout, win, stride)
        assert (plan["splits"], plan["nsub"]) == want and (_cdiv(T, stride) * N) % KB != 0
        forced = _check("randn", win, stride, cout, T, N, gpu_device)
    finally:
        L.tk_lab_conv_window_set_splits(0)
    free = _check("randn", win, stride, cout, T, N, gpu_device)
    for k in ("y", "dx"):       # (the forward and dx do not depend on the runs)
        assert torch.equal(_bits(forced[k]), _bits(free[k])), k


# ---------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------
def test_the_function_through_the_layer(gpu_device, every_shape_in_grad_mode):
    """Convolution(16, 96, 31, stride=12) takes the kernels and the counters move; the autograd Function gives the bits
    of the C calls; an input that needs no gradient gets None from the backward; under no_grad y has the bits it has in
    grad mode; each of the three switches off is the former code, bit for bit."""
    win, stride, cout, T, N = 31, 12, 96, 47, 63
    x, w, b, dy, _ = _inputs("randn", win, stride, cout, T, N)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    layer = _with_weights(cout, win, stride, w, b, gpu_device)
    assert layer._hip_window(x) and not layer._hip_strided(x)
    before = dict(layers.conv_window_calls)
    abi, got = _run(x, w, b, dy, stride), _layer_grads(layer, x, dy, True)
    assert layers.conv_window_calls == {"forward": before["forward"] + 1, "backward": before["backward"] + 1}
    for k in abi:
        assert torch.equal(_bits(abi[k]), _bits(got[k])), k
    # dx not wanted
    layer.zero_grad(set_to_none=True)
    y = layers.WindowConvolution.apply(x, layer.conv.weight, layer.conv.bias, True, stride)
    assert y.grad_fn is not None and y.grad_fn.needs_input_grad[0] is False
    with torch.no_grad():
        grads = layers.WindowConvolution.backward(y.grad_fn, dy)
    assert len(grads) == 5 and grads[0] is None and grads[3] is None and grads[4] is None
    assert torch.equal(_bits(grads[1]), _bits(abi["dw"])) and torch.equal(_bits(grads[2]), _bits(abi["db"]))
    # no_grad
    with torch.no_grad():
        calls = layers.conv_window_calls["forward"]
        assert torch.equal(_bits(layer(x)), _bits(abi["y"]))
        assert layers.conv_window_calls["forward"] == calls + 1
        for t, n in [(1, 1), (3, 2), (13, 1), (1, 5)]:
            xs = x[:t, :n].contiguous()
            want = _run(xs, w, b, None, stride, want_z=False)["y"]
            assert torch.equal(_bits(layer(xs)), _bits(want)), (t, n)
    # each switch off: the former code (pad + unfold + addmm + swish), bit for bit
    def former():
        xr = x.detach().clone().requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        xp = nn.functional.pad(xr, (0, 0, 0, 0, win // 2, (win - 1) // 2))
        unf = xp.unfold(0, win, stride)
        out = torch.addmm(layer.conv.bias, unf.reshape(unf.shape[0] * unf.shape[1], -1),
                          layer.conv.weight.reshape(cout, -1).t())
        yr = layers.swish(out.view(unf.shape[0], unf.shape[1], -1))
        (yr * dy).sum().backward()
        return dict(y=yr.detach().clone(), dx=xr.grad, dw=layer.conv.weight.grad.clone(), db=layer.conv.bias.grad.clone())

    want = former()
    calls = dict(layers.conv_window_calls)
    for name in ("USE_HIP_CONV", "USE_HIP_CONV_STRIDED", "USE_HIP_CONV_WINDOW"):
        off = _layer_grads(layer, x, dy, False, name)
        for k in want:
            assert torch.equal(_bits(off[k]), _bits(want[k])), (name, k)
    assert layers.conv_window_calls == calls


def test_grad_mode_asks_the_table_and_no_grad_does_not(gpu_device, monkeypatch):
    """A configuration outside CONV_WINDOW_GRAD_SHAPES runs the former code in grad mode and the kernels under no_grad;
    the shapes of the strided library keep that library."""
    monkeypatch.setattr(layers, "CONV_WINDOW_GRAD_SHAPES", frozenset())
    layer = _layer(96, 31, 12).to(gpu_device)
    x = torch.randn(47, 3, CIN, device=gpu_device)
    before = dict(layers.conv_window_calls)
    assert not layer._hip_window(x)
    layer(x).sum().backward()
    assert layers.conv_window_calls == before
    with torch.no_grad():
        assert layer._hip_window(x)
        layer(x)
    assert layers.conv_window_calls == {"forward": before["forward"] + 1, "backward": before["backward"]}
    old = _layer(256, 19, 5).to(gpu_device)
    with torch.no_grad():
        assert old._hip_strided(x)
        old(x)
    assert layers.conv_window_calls == {"forward": before["forward"] + 1, "backward": before["backward"]}


def _captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def test_captured_forward_replays_bit_identical(gpu_device):
    torch.manual_seed(7)
    layer = _layer(96, 31, 12).to(gpu_device)
    x = torch.randn(47, 3, CIN, device=gpu_device)
    with torch.no_grad():
        assert layer._hip_window(x)
        eager = layer(x)
        g, out = _captured(lambda: layer(x))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager))


def test_captured_training_forward_and_backward_replay_bit_identical(gpu_device, every_shape_in_grad_mode):
    """The grad-mode forward (z written and saved) and the backward (dz, dx, dW, db) captured into one graph: the replay,
    on new contents of the same input buffers, has the bits of the eager run."""
    win, stride, cout, T, N = 31, 12, 96, 47, 63
    x, w, b, dy, _ = _inputs("randn", win, stride, cout, T, N)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    layer = _with_weights(cout, win, stride, w, b, gpu_device)
    calls = layers.conv_window_calls["backward"]
    eager = _layer_grads(layer, x, dy, True)
    assert layers.conv_window_calls["backward"] == calls + 1
    sx = torch.zeros_like(x).requires_grad_(True)       # the graph's static inputs, filled before the replay
    sdy = torch.zeros_like(dy)

    def step():
        y = layer(sx)
        grads = torch.autograd.grad(y, [sx, layer.conv.weight, layer.conv.bias], sdy)
        return (y.detach(),) + grads

    g, out = _captured(step)
    with torch.no_grad():
        sx.copy_(x)
        sdy.copy_(dy)
        for t in out:
            t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for k, t in zip(("y", "dx", "dw", "db"), out):
        assert torch.equal(_bits(t), _bits(eager[k])), k


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(size=96), dict(size=96, winlen=31, stride=12), dict(size=256, winlen=31, stride=10)],
                         ids=["96-19-5", "96-31-12", "256-31-10"])
def test_a_reads_scores_do_not_depend_on_its_batch(gpu_device, kw):
    """Under no_grad, T = 240, N = 5: column n of a batch's scores is bit for bit the scores of column n alone."""
    torch.manual_seed(5)
    model = models.mLstm_flipflop(**kw).to(gpu_device).eval()
    x = torch.randn(240, 5, 1, device=gpu_device)
    with torch.no_grad():
        calls = layers.conv_window_calls["forward"]
        whole = model(x)
        assert layers.conv_window_calls["forward"] == calls + 1
        for n in range(5):
            assert torch.equal(_bits(whole[:, n:n + 1]), _bits(model(x[:, n:n + 1].contiguous()))), n


def _parent_forward(self, x):
    """Convolution.forward as it was before the layer had kernels at these shapes (the strided library's shapes apart)"""
    if not self.use_gemm:
        out = self.activation(self.conv(self.pad(x.permute(1, 2, 0))))
        return out.permute(2, 0, 1)
    if self._hip_small(x):
        return layers.SmallConvolution.apply(x, self.conv.weight, self.conv.bias)
    xp = nn.functional.pad(x, (0, 0, 0, 0, self.winlen // 2, (self.winlen - 1) // 2))
    win = xp.unfold(0, self.winlen, self.stride)
    tout, n = win.shape[0], win.shape[1]
    w = self.conv.weight.reshape(self.conv.weight.shape[0], -1)
    out = torch.addmm(self.conv.bias, win.reshape(tout * n, -1), w.t())
    return self.activation(out.view(tout, n, -1))


def _net_grads(net, x, dy, switch):
    old = layers.USE_HIP_CONV_WINDOW
    layers.USE_HIP_CONV_WINDOW = switch
    try:
        for p in net.parameters():
            p.grad = None
        out = net(x)
        (out * dy).sum().backward()
    finally:
        layers.USE_HIP_CONV_WINDOW = old
    res = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    res["out"] = out.detach().clone()
    return res


@pytest.mark.parametrize("make,kw,T", [(models.mLstm_flipflop, dict(size=96), 200),
                                       (models.mLstm_cat_mod_flipflop, dict(size=256, winlen=31, stride=10), 400)],
                         ids=["mLstm-96-19-5", "cat-mod-256-31-10"])
def test_model_with_the_switch_on_and_off(gpu_device, monkeypatch, every_shape_in_grad_mode, make, kw, T):
    """A chunk of 40 blocks, 4 columns.  Switch off: the output and every gradient are the bits of the layer's forward
    as it was.  Switch on: they differ from the switch-off run by at most twice what that run differs from float64 by,
    plus 2e-6 (relative to the largest entry)."""
    torch.manual_seed(5)
    net = make(**kw)
    x = torch.randn(T, 4, 1)
    dy = torch.randn(*net(x).shape) / 40 ** 0.5
    n64 = copy.deepcopy(net).double()
    ref = _net_grads(n64, x.double(), dy.double(), True)
    net = net.to(gpu_device)
    x, dy = x.to(gpu_device), dy.to(gpu_device)
    calls = dict(layers.conv_window_calls)
    on = _net_grads(net, x, dy, True)
    assert layers.conv_window_calls == {"forward": calls["forward"] + 1, "backward": calls["backward"] + 1}
    off = _net_grads(net, x, dy, False)
    with monkeypatch.context() as mp:
        mp.setattr(layers.Convolution, "forward", _parent_forward)
        parent = _net_grads(net, x, dy, True)
    assert layers.conv_window_calls == {"forward": calls["forward"] + 1, "backward": calls["backward"] + 1}
    assert set(on) == set(off) == set(parent) == set(ref)
    for k, r in ref.items():
        assert torch.equal(_bits(off[k]), _bits(parent[k])), k
        scale = r.abs().max().item() or 1.0
        d_on = (on[k] - off[k]).abs().max().item() / scale
        e_off = (off[k].double().cpu() - r).abs().max().item() / scale
        print("%s %s: kernels - GEMM path %.3g, GEMM path - float64 %.3g" % (make.__name__, k, d_on, e_off))
        assert d_on <= 2 * e_off + 2e-6, (k, d_on, e_off)


def _window_31_model(dev):
    torch.manual_seed(7)
    return synth.excite_network(models.mLstm_flipflop(size=96, winlen=31, stride=12)).to(dev).eval()


def _off(fn):
    old = layers.USE_HIP_CONV_WINDOW
    layers.USE_HIP_CONV_WINDOW = False
    try:
        calls = dict(layers.conv_window_calls)
        res = fn()
        assert layers.conv_window_calls == calls
        return res
    finally:
        layers.USE_HIP_CONV_WINDOW = old


def test_forward_varlen_through_a_window_31_model(gpu_device):
    """Two columns of different lengths in one call: the output lengths are conv_out_lengths', every row behind a
    column's end is 0, and the Viterbi calls are those of the switch-off run."""
    from taiyaki_amd import decode
    net = _window_31_model(gpu_device)
    lengths = np.array([600, 333])
    x = torch.randn(600, 2, 1, device=gpu_device)
    x[333:, 1] = 0
    with torch.no_grad():
        calls = layers.conv_window_calls["forward"]
        out, out_lens = layers.forward_varlen(net, x, lengths)
        assert layers.conv_window_calls["forward"] > calls
        assert out_lens.tolist() == layers.conv_out_lengths(lengths, 12).tolist() == [50, 28]
        for n in range(2):
            assert not out[out_lens[n]:, n].any()
        off, off_lens = _off(lambda: layers.forward_varlen(net, x, lengths))
        assert off_lens.tolist() == out_lens.tolist()
        for n in range(2):
            got = decode.flipflop_viterbi(out[:out_lens[n], n:n + 1].contiguous())[2]
            want = decode.flipflop_viterbi(off[:out_lens[n], n:n + 1].contiguous())[2]
            assert torch.equal(got, want), n


def test_basecaller_through_a_window_31_model(gpu_device):
    """Two short signals, the second shorter than a chunk: the calls of the switch-off run."""
    net = _window_31_model(gpu_device)
    rs = np.random.RandomState(3)
    sigs = [(90 + 12 * rs.standard_normal(n)).astype(np.float32) for n in (2900, 500)]

    def call():     # (a caller of its own for each path)
        return basecall.Basecaller(net, stride=12, chunk_size=100, overlap=10, fastq=True).call(sigs)

    calls = layers.conv_window_calls["forward"]
    got = call()
    assert layers.conv_window_calls["forward"] > calls
    want = _off(call)
    assert [c[2] for c in got] == [2900, 500] and all(len(s) == len(q) > 0 for s, q, _ in got)
    assert [c[0] for c in got] == [c[0] for c in want]

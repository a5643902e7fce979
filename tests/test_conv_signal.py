"""Convolution(1 -> Cout, window 19, stride 1 ... 8, tanh), the mGru models' first layer, on the kernels of
csrc/conv_signal.hip (include/taiyaki_amd_conv_signal.h) against nn.Conv1d + tanh in float64 on the host, with the path
it replaces (pad + unfold + rocBLAS GEMM + element-wise kernels: the same layer with USE_HIP_CONV_SIGNAL = False) as
the yardstick: the criterion of tests/test_rnn_proj.py and tests/test_conv_strided.py, the error relative to the
largest reference entry at most twice the GEMM path's on the same inputs, plus 2e-6 -- for each of y, dW and db."""
import copy
import functools

import pytest
import torch
from torch import nn

from taiyaki_amd import _lib, layers, models
from tests.helpers import gru_net

pytestmark = pytest.mark.gpu

CUS = 256
OK = 0
WIN, COUT = 19, 96
ADMITTED = (32, 64, 96, 128, 192, 256, 384)
GUARD = 64


def _cdiv(a, b):
    return -(-a // b)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(numel, dev):
    buf = torch.full((GUARD + numel + GUARD,), 7.0, device=dev)
    out = buf[GUARD:GUARD + numel]
    out.view(torch.uint8).fill_(0xFF)
    return buf, out


def _run(x, w, b, dy, stride, cus=CUS):
    """One forward call and (dy given) one backward call on device tensors: x (T, N).  Every output lies between two
    guard bands over a sentinel and is pre-filled with 0xFF bytes, as is the workspace, of exactly the size asked."""
    L = _lib.conv_signal_lib()
    T, N = x.shape
    cout = w.shape[0]
    tout = _cdiv(T, stride)
    dev = x.device
    sizes = dict(y=tout * N * cout, dw=cout * WIN, db=cout)
    bufs = {k: _guarded(n, dev) for k, n in sizes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    assert o["y"].data_ptr() % 16 == 0
    rc = L.tk_conv_signal_forward_dev(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), T, N, cout, stride, cus, _lib.ptr(o["y"]),
                                      _lib.stream_ptr())
    assert rc == OK
    if dy is not None:
        wsb = L.tk_conv_signal_workspace_bytes(T, N, cout, stride, cus)
        assert wsb > 0
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev)
        rc = L.tk_conv_signal_backward_dev(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(o["y"]), T, N, cout, stride, cus,
                                           _lib.ptr(o["dw"]), _lib.ptr(o["db"]), _lib.ptr(ws), wsb, _lib.stream_ptr())
        assert rc == OK
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert (buf[:GUARD] == 7.0).all() and (buf[GUARD + sizes[k]:] == 7.0).all(), "guard bands of " + k
    res = dict(y=o["y"].view(tout, N, cout).clone())
    if dy is not None:
        res.update(dw=o["dw"].view(cout, 1, WIN).clone(), db=o["db"].clone())
    return res


def _ref64(x, w, b, dy, stride):
    """nn.Conv1d + tanh and their gradients, float64 on the host; `dw_abs`, `db_abs`: the sums of the magnitudes of the
    gradients' terms"""
    cout = w.shape[0]
    conv = nn.Conv1d(1, cout, WIN, stride=stride).double()
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    xp = nn.functional.pad(x.double().t().unsqueeze(1), (WIN // 2, (WIN - 1) // 2))     # (N, 1, T + 18)
    z = conv(xp).permute(2, 0, 1)
    y = torch.tanh(z)
    (y * dy.double()).sum().backward()
    dz = (dy.double() * (1 - y.detach() ** 2)).abs()
    win = xp[:, 0].t().unfold(0, WIN, stride).abs()         # (Tout, N, 19)
    return dict(y=y.detach(), z=z.detach(), dw=conv.weight.grad, db=conv.bias.grad,
                dw_abs=torch.einsum("tnc,tnk->ck", dz, win), db_abs=dz.sum((0, 1)))


def _make(kind, T, N, cout, stride, seed=0):
    g = torch.Generator().manual_seed(1000 * T + 10 * N + cout + stride + seed)
    tout = _cdiv(T, stride)
    x = torch.randn(T, N, generator=g)
    w = torch.randn(cout, 1, WIN, generator=g) / WIN ** 0.5
    b = torch.randn(cout, generator=g) * 0.5
    dy = torch.randn(tout, N, cout, generator=g) / (tout * N) ** 0.5
    if kind == "saturate":      # a spike of +-1e4 every 40 samples of a column (a window holds at most one): the
        for n in range(N):      # pre-activations of its windows reach thousands
            at = torch.arange(7 + 3 * n, T, 40)
            x[at, n] = 1e4 * (1 - 2 * (torch.arange(len(at)) % 2)).float()
    if kind == "cancel":        # dy alternates in sign along t over a slowly varying signal: dW's terms cancel
        x = 1 + x * 2.0 ** -6
        w, b = w * 0.05, b * 0.1
        dy = (1 + dy * 2.0 ** -6) * (1 - 2 * (torch.arange(tout) % 2)).float()[:, None, None] / (tout * N)
    return x, w, b, dy, _ref64(x, w, b, dy, stride)


_inputs = functools.lru_cache(maxsize=None)(_make)


def _layer(cout, stride, w, b, dev):
    layer = layers.Convolution(1, cout, WIN, stride=stride).to(dev)
    with torch.no_grad():
        layer.conv.weight.copy_(w)
        layer.conv.bias.copy_(b)
    return layer


def _switched(value, fn):
    old = layers.USE_HIP_CONV_SIGNAL
    layers.USE_HIP_CONV_SIGNAL = value
    try:
        return fn()
    finally:
        layers.USE_HIP_CONV_SIGNAL = old


def _layer_grads(layer, x3, dy, switch):
    def go():
        for p in layer.parameters():
            p.grad = None
        y = layer(x3)
        (y * dy).sum().backward()
        return dict(y=y.detach().clone(), dw=layer.conv.weight.grad.clone(), db=layer.conv.bias.grad.clone())
    return _switched(switch, go)


def _gemm_path(x, w, b, dy, stride):
    """what the layer runs with the switch off, on the same device tensors"""
    before = dict(layers.conv_signal_calls)
    res = _layer_grads(_layer(w.shape[0], stride, w, b, x.device), x.unsqueeze(2), dy, False)
    assert layers.conv_signal_calls == before
    return res


def _rel(got, ref, scale=None):
    return (got.double().cpu() - ref).abs().max().item() / ((ref.abs().max().item() if scale is None else scale) or 1.0)


def _hold(what, got, gemm, ref, scales=None):
    for k in ("y", "dw", "db"):
        scale = None if scales is None or k == "y" else ref[k + "_abs"].max().item()
        e_hip, e_gemm = _rel(got[k], ref[k], scale), _rel(gemm[k], ref[k], scale)
        print("signal conv %s %s: kernel %.3g, GEMM path %.3g" % (what, k, e_hip, e_gemm))
        assert torch.isfinite(got[k]).all(), (what, k)
        assert e_hip <= 2 * e_gemm + 2e-6, (what, k, e_hip, e_gemm)


def _check(kind, T, N, cout, stride, dev, cus=CUS):
    x, w, b, dy, ref = _inputs(kind, T, N, cout, stride)
    x, w, b, dy = (v.to(dev) for v in (x, w, b, dy))
    got, gemm = _run(x, w, b, dy, stride, cus), _gemm_path(x, w, b, dy, stride)
    _hold("%s (T, N, Cout, stride, CUs) = %s" % (kind, (T, N, cout, stride, cus)), got, gemm, ref,
          scales="abs" if kind == "cancel" else None)
    return got, ref


@pytest.mark.parametrize("stride", [1, 2, 4, 5])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("T", [1, 9, 10, 19, 23, 41])
def test_window_edges(gpu_device, T, N, stride):
    """T shorter than half a window, both pads overlapping, T not a multiple of the stride, a last window that reads
    past T; odd N: rows of x off 16-byte alignment."""
    _check("randn", T, N, COUT, stride, gpu_device)


@pytest.mark.parametrize("cout", ADMITTED)
@pytest.mark.parametrize("T,N,stride", [(23, 3, 5), (641, 65, 2)])
def test_every_admitted_cout(gpu_device, T, N, stride, cout):
    """The second shape: 405 tiles, five tile columns (the last one column wide), more than one partial result."""
    _check("randn", T, N, cout, stride, gpu_device)


def test_partial_results_at_three_cu_counts(gpu_device):
    """2, 14 and 405 workgroups: each meets the criterion; the forward's bits do not depend on cu_count; two backward
    runs at one cu_count are bit-identical (outputs and workspace pre-filled with 0xFF bytes, _run)."""
    T, N, stride = 641, 65, 2
    L = _lib.conv_signal_lib()
    slab = COUT * 20 * 4
    assert [L.tk_conv_signal_workspace_bytes(T, N, COUT, stride, c) // slab for c in (1, 7, 256)] == [2, 14, 405]
    x, w, b, dy, _ = _inputs("randn", T, N, COUT, stride)
    dx, dw_, db_, ddy = (v.to(gpu_device) for v in (x, w, b, dy))
    runs = {}
    for cus in (1, 7, 256):
        runs[cus], _ = _check("randn", T, N, COUT, stride, gpu_device, cus)
        again = _run(dx, dw_, db_, ddy, stride, cus)
        for k in ("y", "dw", "db"):
            assert torch.equal(_bits(runs[cus][k]), _bits(again[k])), (cus, k)
    for cus in (7, 256):
        assert torch.equal(_bits(runs[1]["y"]), _bits(runs[cus]["y"])), cus


def test_saturation(gpu_device):
    """x entries of +-1e4: y is exactly +-1 wherever the float64 pre-activation is beyond +-30 (thousands of rows
    reach +-1e3 and more), never outside [-1, 1], every gradient finite, the criterion as ever."""
    T, N, stride = 641, 3, 2
    got, ref = _check("saturate", T, N, COUT, stride, gpu_device)
    y, z = got["y"].cpu(), ref["z"]
    sat = z.abs() >= 30
    assert int(sat.sum()) > 1000 and float(z.abs().max()) > 1e3
    assert torch.equal(y[sat], torch.sign(z[sat]).float())
    assert torch.isfinite(y).all() and float(y.abs().max()) == 1.0


def test_cancelling_weight_gradient(gpu_device):
    """dy alternates in sign along t: dW and db are sums of terms that cancel; their errors are taken relative to the
    largest entry of the float64 sum of the terms' magnitudes."""
    T, N, stride = 641, 65, 2
    ref = _inputs("cancel", T, N, COUT, stride)[4]
    assert ref["dw"].abs().max().item() < 2e-2 * ref["dw_abs"].max().item()
    assert ref["db"].abs().max().item() < 2e-2 * ref["db_abs"].max().item()
    _check("cancel", T, N, COUT, stride, gpu_device)


@pytest.mark.parametrize("T", [23, 641])
def test_a_column_alone_has_the_bits_it_has_in_a_batch(gpu_device, T):
    N, stride = 65, 2
    x, w, b, _, _ = _inputs("randn", T, N, COUT, stride)
    x, w, b = (v.to(gpu_device) for v in (x, w, b))
    full = _run(x, w, b, None, stride)["y"]
    for n in (0, 15, 16, 31, 64):
        alone = _run(x[:, n:n + 1].contiguous(), w, b, None, stride)["y"]
        assert torch.equal(_bits(alone), _bits(full[:, n:n + 1])), n


def test_a_prefix_of_the_signal_has_the_bits_it_has_in_the_whole(gpu_device):
    T, T1, N, stride = 641, 200, 65, 4
    x, w, b, _, _ = _inputs("randn", T, N, COUT, stride)
    x, w, b = (v.to(gpu_device) for v in (x, w, b))
    full, head = _run(x, w, b, None, stride)["y"], _run(x[:T1].contiguous(), w, b, None, stride)["y"]
    keep = [t for t in range(_cdiv(T1, stride)) if stride * t + 9 < T1]
    assert len(keep) == 48 and head.shape[0] == 50
    assert torch.equal(_bits(head[keep]), _bits(full[keep]))


def test_a_nan_stays_in_the_rows_whose_windows_hold_it(gpu_device):
    T, N, stride = 641, 65, 4
    x, w, b, _, _ = _inputs("randn", T, N, COUT, stride)
    x, w, b = (v.to(gpu_device) for v in (x, w, b))
    clean = _run(x, w, b, None, stride)["y"]
    t_bad, n_bad = 320, 17
    bad = x.clone()
    bad[t_bad, n_bad] = float("nan")
    got = _run(bad, w, b, None, stride)["y"]
    holds = torch.zeros(clean.shape[:2], dtype=torch.bool, device=gpu_device)
    for t in range(clean.shape[0]):
        holds[t, n_bad] = abs(stride * t - t_bad) <= 9
    assert int(holds.sum()) == 5
    assert torch.isnan(got[holds]).all()
    assert torch.equal(_bits(got[~holds]), _bits(clean[~holds]))


def test_the_shipped_network(gpu_device):
    """The reference's shipped mGru network (tests/golden/gru_net*.npz): its first layer, 1 -> 96 at stride 4, on its
    (2000, 16) signal under the criterion; the whole network's scores against the float64 model built from the same
    arrays under the same criterion, with the switch on and off."""
    arrays = gru_net.load_arrays()
    signal = torch.from_numpy(arrays["signal"])
    assert signal.shape == (2000, 16)
    net64 = gru_net.build_model(arrays, torch.float64)
    net = gru_net.build_model(arrays).to(gpu_device)
    first = net[0]
    assert (first.conv.weight.shape, first.stride) == ((96, 1, WIN), 4)
    xg = signal.to(gpu_device).unsqueeze(2)
    with torch.no_grad():
        ref_y, ref = net64[0](signal.double().unsqueeze(2)), net64(signal.double().unsqueeze(2))
        assert first._hip_signal(xg)
        calls = layers.conv_signal_calls["forward"]
        y_on, y_off = _switched(True, lambda: first(xg)), _switched(False, lambda: first(xg))
        on, off = _switched(True, lambda: net(xg)), _switched(False, lambda: net(xg))
        assert layers.conv_signal_calls["forward"] == calls + 2
    for what, got, gemm, r in (("first layer", y_on, y_off, ref_y), ("scores, switch on", on, off, ref),
                               ("scores, switch off", off, off, ref)):
        e_hip, e_gemm = _rel(got, r), _rel(gemm, r)
        print("shipped network %s: %.3g, GEMM path %.3g" % (what, e_hip, e_gemm))
        assert e_hip <= 2 * e_gemm + 2e-6, (what, e_hip, e_gemm)


class _Ctx:
    saved = None

    def save_for_backward(self, *tensors):
        self.saved = tensors


def _param_grads(net, x, dy, switch):
    def go():
        for p in net.parameters():
            p.grad = None
        out = net(x)
        (out * dy).sum().backward()
        res = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
        res["out"] = out.detach().clone()
        return res
    return _switched(switch, go)


@pytest.mark.parametrize("make", [lambda: layers.Convolution(1, 96, WIN, stride=2),
                                  lambda: models.mGru_flipflop(size=32, stride=2)], ids=["layer", "mGru_flipflop"])
def test_through_the_layer_and_the_model(gpu_device, make):
    """T 200, N 3: the output and every parameter's gradient with the switch on within twice the switch-off error from
    the float64 CPU model, plus 2e-6; one forward and one backward launch counted."""
    torch.manual_seed(5)
    net = make()
    x = torch.randn(200, 3, 1)
    dy = torch.randn(*net(x).shape) / 300 ** 0.5
    ref = _param_grads(copy.deepcopy(net).double(), x.double(), dy.double(), True)
    net = net.to(gpu_device)
    x, dy = x.to(gpu_device), dy.to(gpu_device)
    before = dict(layers.conv_signal_calls)
    on = _param_grads(net, x, dy, True)
    assert layers.conv_signal_calls == {"forward": before["forward"] + 1, "backward": before["backward"] + 1}
    off = _param_grads(net, x, dy, False)
    assert layers.conv_signal_calls == {"forward": before["forward"] + 1, "backward": before["backward"] + 1}
    assert set(on) == set(off) == set(ref)
    for k, r in ref.items():
        e_on, e_off = _rel(on[k], r), _rel(off[k], r)
        print("%s: kernels %.3g, GEMM path %.3g" % (k, e_on, e_off))
        assert e_on <= 2 * e_off + 2e-6, (k, e_on, e_off)


def test_no_grad_saves_nothing_and_keeps_the_bits(gpu_device):
    torch.manual_seed(6)
    layer = layers.Convolution(1, 96, WIN, stride=2).to(gpu_device)
    x = torch.randn(200, 3, 1, device=gpu_device)
    y_grad = layer(x)
    assert y_grad.grad_fn is not None and len(y_grad.grad_fn.saved_tensors) == 2
    kept = y_grad.grad_fn.saved_tensors[0]
    assert torch.equal(kept, x) and kept.data_ptr() != x.data_ptr()      # (a copy: the input buffer may be reloaded)
    with torch.no_grad():
        y = layer(x)
    assert y.grad_fn is None and torch.equal(_bits(y), _bits(y_grad))
    w, b = layer.conv.weight, layer.conv.bias
    for save in (False, True):
        ctx = _Ctx()
        out = layers.SignalConvolution.forward(ctx, x, w, b, save, 2)
        assert (ctx.saved is not None) == save and torch.equal(_bits(out), _bits(y_grad))
    # an empty batch: no launch, empty or zero results
    before = dict(layers.conv_signal_calls)
    for shape in [(0, 3, 1), (200, 0, 1)]:
        e = layers.SignalConvolution.apply(torch.empty(*shape, device=gpu_device), w, b, True, 2)
        assert e.shape == (_cdiv(shape[0], 2), shape[1], 96)
        gw, gb = torch.autograd.grad(e.sum(), [w, b])
        assert not gw.any() and not gb.any() and gw.shape == w.shape
    assert layers.conv_signal_calls == before


def test_captured_forward_replays_bit_identical(gpu_device):
    torch.manual_seed(7)
    layer = layers.Convolution(1, 96, WIN, stride=2).to(gpu_device)
    x = torch.randn(23, 3, 1, device=gpu_device)
    assert layer._hip_signal(x)
    with torch.no_grad():
        eager = layer(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            layer(x)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = layer(x)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager))


def test_captured_training_forward_and_backward_replay_bit_identical(gpu_device):
    """The grad-mode forward (y and a copy of x saved) and the backward captured into one graph: the replay, after the
    input buffers were reloaded in place, has the bits of the eager run."""
    T, N, stride = 200, 3, 2
    x, w, b, dy, _ = _inputs("randn", T, N, COUT, stride)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    layer = _layer(COUT, stride, w, b, gpu_device)
    eager = _layer_grads(layer, x.unsqueeze(2), dy, True)
    sx, sdy = torch.zeros(T, N, 1, device=gpu_device), torch.zeros_like(dy)     # the graph's static inputs

    def step():
        y = layer(sx)
        return (y.detach(),) + torch.autograd.grad(y, [layer.conv.weight, layer.conv.bias], sdy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    with torch.no_grad():
        sx.copy_(x.unsqueeze(2))
        sdy.copy_(dy)
        for t in out:
            t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for k, t in zip(("y", "dw", "db"), out):
        assert torch.equal(_bits(t), _bits(eager[k])), k

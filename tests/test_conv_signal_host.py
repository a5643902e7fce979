"""Convolution(1 -> Cout, window 19, stride 1 ... 8, tanh), the mGru models' first layer, on the kernels of
csrc/conv_signal.hip (include/taiyaki_amd_conv_signal.h): what is decided on the host -- the binding, the rule, the
workspace, the refusals before a launch and the layer's dispatch.  No GPU in this file."""
import ctypes
import re
import subprocess

import torch

from taiyaki_amd import _lib, layers

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
ADMITTED = (32, 64, 96, 128, 192, 256, 384)     # every Cout the rule admits: the GRU kernels' sizes
WIN = 19
NT, TILE_ROWS = 16, 64      # a tile: at most 16 columns, at most 64 rows (csrc/conv_signal.hip)
BWD_PER_CU = 2              # workgroups per CU of the backward's full grid: one partial result each
NAMES = {"tk_conv_signal_supported", "tk_conv_signal_workspace_bytes", "tk_conv_signal_forward_dev",
         "tk_conv_signal_backward_dev"}


def _cdiv(a, b):
    return -(-a // b)


def workspace_py(T, N, cout, stride, cus):
    """The rule restated: one partial result of Cout x 20 floats per workgroup of the backward launch."""
    if cout not in ADMITTED or not 1 <= stride <= 8 or T == 0 or N == 0 or cus < 1:
        return 0
    tout = _cdiv(T, stride)
    if tout * N * cout >= 1 << 31:
        return 0
    nt = min(N, NT)
    tt = TILE_ROWS // nt
    ntiles = _cdiv(N, nt) * _cdiv(tout, tt)
    return min(ntiles, BWD_PER_CU * cus) * cout * (WIN + 1) * 4


def test_header_parses_into_the_binding():
    assert set(_lib.CONV_SIGNAL_SIGNATURES) == NAMES
    assert len(_lib.CONV_SIGNAL_SIGNATURES["tk_conv_signal_forward_dev"][1]) == 10
    assert len(_lib.CONV_SIGNAL_SIGNATURES["tk_conv_signal_backward_dev"][1]) == 13
    assert _lib.CONV_SIGNAL_SIGNATURES["tk_conv_signal_workspace_bytes"][0] is ctypes.c_size_t
    L = _lib.conv_signal_lib()      # every symbol resolves
    assert all(hasattr(L, n) for n in NAMES)


def test_the_library_exports_the_header_and_nothing_else():
    import os
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib.CONV_SIGNAL_LIBNAME)],
                         check=True, capture_output=True, text=True).stdout
    exported = {m.group(1) for m in re.finditer(r"(?m)^[0-9a-f]+ [TDBR] (\w+)$", out)}
    assert exported == NAMES, exported


def test_the_rule_admits_what_is_documented():
    L = _lib.conv_signal_lib()
    for cin in (1, 4, 16):
        for win in (5, 17, 19, 21):
            for stride in (0, 1, 5, 8, 9):
                for cout in (16, 32, 96, 100, 384, 512):
                    want = cin == 1 and win == 19 and 1 <= stride <= 8 and cout in ADMITTED
                    assert bool(L.tk_conv_signal_supported(cin, cout, win, stride)) == want, (cin, win, stride, cout)
    for cout in ADMITTED:
        for stride in range(1, 9):
            assert L.tk_conv_signal_supported(1, cout, 19, stride) == 1


def test_the_workspace_is_the_rule_restated():
    ws = _lib.conv_signal_lib().tk_conv_signal_workspace_bytes
    for cus in (256, 304):
        for T, N, cout, stride in [(2000, 64, 96, 2), (4000, 128, 256, 5), (100000, 64, 96, 4), (23, 3, 96, 5),
                                   (641, 65, 384, 2), (1, 1, 32, 8)]:
            want = workspace_py(T, N, cout, stride, cus)
            assert ws(T, N, cout, stride, cus) == want > 0, (T, N, cout, stride, cus)
    assert ws(2000, 64, 96, 2, 256) == 512 * 96 * 20 * 4       # (1000 tiles: a full grid)
    assert ws(23, 3, 96, 5, 256) == 1 * 96 * 20 * 4            # (5 x 3 rows: one tile)
    assert ws(0, 64, 96, 2, 256) == 0 and ws(2000, 0, 96, 2, 256) == 0 and ws(2000, 64, 96, 2, 0) == 0
    assert ws(2000, 64, 100, 2, 256) == 0 and ws(2000, 64, 96, 0, 256) == 0 and ws(2000, 64, 96, 9, 256) == 0
    for cout in ADMITTED:       # the first shape with rows x Cout >= 2^31
        edge = _cdiv(1 << 31, cout)
        assert ws(edge - 1, 1, cout, 1, 256) == workspace_py(edge - 1, 1, cout, 1, 256) > 0
        assert ws(edge, 1, cout, 1, 256) == 0 and ws(1, edge, cout, 1, 256) == 0
        assert ws(4 * (edge - 1), 1, cout, 4, 256) > 0 and ws(4 * (edge - 1) + 1, 1, cout, 4, 256) == 0
        assert ws(1 << 40, 1 << 30, cout, 1, 256) == 0 and ws(1 << 62, 1 << 62, cout, 8, 256) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """NULL or a misaligned y / dy / workspace -> TK_ERR_BAD_ARG, a short workspace -> TK_ERR_WORKSPACE, a shape outside
    the rule -> TK_ERR_UNSUPPORTED: decided on the host (the pointers are never dereferenced: no GPU in this test)."""
    L = _lib.conv_signal_lib()
    T, N, cout, stride, cus = 23, 3, 96, 5, 256
    need = L.tk_conv_signal_workspace_bytes(T, N, cout, stride, cus)
    assert need > 0
    names = ("dy", "x", "y", "w", "b", "dw", "db", "ws")
    good = {n: ctypes.c_void_p(4096 * (i + 1)) for i, n in enumerate(names)}
    null = ctypes.c_void_p(0)

    def fwd(shape=(T, N, cout, stride), **kw):
        p = dict(good, **kw)
        return L.tk_conv_signal_forward_dev(p["x"], p["w"], p["b"], *shape, cus, p["y"], None)

    def bwd(wsb=need, shape=(T, N, cout, stride), **kw):
        p = dict(good, **kw)
        return L.tk_conv_signal_backward_dev(p["dy"], p["x"], p["y"], *shape, cus, p["dw"], p["db"], p["ws"], wsb, None)

    for call, needs, aligned in ((fwd, ("x", "w", "b", "y"), ("y",)),
                                 (bwd, ("dy", "x", "y", "dw", "db", "ws"), ("dy", "y", "ws"))):
        for name in needs:
            assert call(**{name: null}) == BAD_ARG, name
        for name in aligned:
            assert call(**{name: ctypes.c_void_p(4096 + 4)}) == BAD_ARG, name
        assert call(x=ctypes.c_void_p(4096 + 2)) == BAD_ARG
        for shape in [(0, N, cout, stride), (T, 0, cout, stride), (T, N, cout, 0), (T, N, cout, 9)] \
                + [(T, N, c, stride) for c in (16, 100, 512)]:
            assert call(shape=shape) == UNSUPPORTED, shape
        assert call(shape=(_cdiv(1 << 31, cout), 1, cout, 1)) == UNSUPPORTED
    assert bwd(wsb=need - 1) == WORKSPACE and bwd(wsb=0) == WORKSPACE
    # a misaligned pointer or a NULL is named before the workspace or the shape is
    assert bwd(wsb=0, y=ctypes.c_void_p(4096 + 4)) == BAD_ARG and fwd(shape=(T, N, 100, stride), y=null) == BAD_ARG


def _layer(cout=96, stride=2, fun=torch.tanh):
    torch.manual_seed(3)
    return layers.Convolution(1, cout, WIN, stride=stride, fun=fun)


def _with_switch(value, fn):
    old = layers.USE_HIP_CONV_SIGNAL
    layers.USE_HIP_CONV_SIGNAL = value
    try:
        return fn()
    finally:
        layers.USE_HIP_CONV_SIGNAL = old


def test_the_switch_and_the_counter_exist():
    assert layers.USE_HIP_CONV_SIGNAL is True
    assert layers.conv_signal_calls == {"forward": layers.conv_signal_calls["forward"],
                                        "backward": layers.conv_signal_calls["backward"]}
    assert issubclass(layers.SignalConvolution, torch.autograd.Function)


def test_cpu_tensors_keep_the_gemm_path():
    layer, x = _layer(), torch.randn(23, 3, 1)
    before = dict(layers.conv_signal_calls)
    assert not layer._hip_signal(x)
    on = layer(x)
    off = _with_switch(False, lambda: layer(x))
    assert layers.conv_signal_calls == before
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))
    want = torch.tanh(layer.conv(layer.pad(x.permute(1, 2, 0)))).permute(2, 0, 1)
    assert torch.allclose(on, want, atol=1e-5)


def test_another_activation_and_an_input_that_needs_a_gradient_keep_the_gemm_path(monkeypatch):
    """... also where everything else about the call would take the kernels: the rule is asked about stand-ins that
    look like device tensors, which it then has to refuse on the activation and on `requires_grad` alone."""
    from types import SimpleNamespace as NS
    monkeypatch.setattr(layers, "_cu_count", lambda dev: 256)

    def takes(fun=torch.tanh, shape=(23, 3, 1), requires_grad=False, cout=96, stride=2, **kw):
        dev = dict(is_cuda=True, dtype=torch.float32)
        xs = NS(shape=shape, dim=lambda: len(shape), requires_grad=requires_grad, device=None, **dict(dev, **kw))
        conv = NS(weight=NS(shape=(cout, 1, WIN), **dev), bias=NS(shape=(cout,), **dev))
        return bool(layers.Convolution._hip_signal(NS(conv=conv, activation=fun, winlen=WIN, stride=stride), xs))

    assert takes()
    assert not takes(fun=layers.swish) and not takes(fun=layers.linear) and not takes(fun=torch.sigmoid)
    assert not takes(requires_grad=True)
    with torch.no_grad():
        assert takes(requires_grad=True)        # (no graph is recorded: nobody asks for dx)
    assert not takes(is_cuda=False) and not takes(dtype=torch.float64) and not takes(shape=(23, 3, 2))
    assert not takes(shape=(23, 3)) and not takes(shape=(0, 3, 1)) and not takes(cout=100) and not takes(stride=9)
    assert not _with_switch(False, takes)
    monkeypatch.setattr(layers, "USE_HIP_CONV", False)
    assert not takes()
    monkeypatch.undo()
    # on real (CPU) tensors the bits are those with the switch off, and the counter does not move
    x = torch.randn(23, 3, 1)
    before = dict(layers.conv_signal_calls)
    for fun in (layers.swish, torch.tanh):
        layer = _layer(fun=fun)
        xr = x.clone().requires_grad_(True)
        on = layer(xr)
        on.sum().backward()
        g_on, w_on = xr.grad.clone(), layer.conv.weight.grad.clone()
        xr.grad = layer.conv.weight.grad = None
        off = _with_switch(False, lambda: layer(xr))
        off.sum().backward()
        assert torch.equal(on.view(torch.int32), off.view(torch.int32))
        assert torch.equal(g_on, xr.grad) and torch.equal(w_on, layer.conv.weight.grad)
    assert layers.conv_signal_calls == before

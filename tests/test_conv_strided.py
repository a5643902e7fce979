"""Convolution(16 -> 192 / 256 / 384, window 19, stride 5, swish), the mLstm models' third layer, on the kernels of
csrc/conv_strided.hip (include/taiyaki_amd_conv_strided.h) against nn.Conv1d + swish in float64 on the host, with the
path it replaces (pad + unfold + rocBLAS GEMM + element-wise kernels) as the yardstick: the criterion of
tests/test_rnn_proj.py, the error relative to the largest reference entry at most twice the GEMM path's on the same
inputs, plus 2e-6 -- for each of y, dx, dW and db."""
import copy
import ctypes
import functools

import pytest
import torch
from torch import nn

from taiyaki_amd import _lib, layers, models

CUS = 256
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
CIN, WIN, STRIDE, COUT = 16, 19, 5, 256
KW = CIN * WIN                  # 304 columns of a window
RT, NT, KB = 128, 128, 16       # the GEMMs' tile and k block (csrc/conv_strided.hip)
B_BLOCK = 3 * 4 * 1024          # bytes of the three weight images of one (column tile, k block)
WG_TILE, CHAIN = 128, 8192      # the weight gradient's tile edge and longest accumulation chain
ADMITTED = (192, 256, 384)      # every Cout the rule admits
PLAN_KEYS = ("tiles_m", "f_tiles_n", "f_nkb", "f_grid", "d_tiles_n", "d_nkb", "splits", "nsub", "run_rows", "sub_rows",
             "w_grid", "bytes")


def _cdiv(a, b):
    return -(-a // b)


def _plan_py(T, N, cout=COUT, cus=CUS, splits=0):
    """The plan restated: None where the kernels do not run."""
    if T == 0 or N == 0 or cus <= 0 or cout not in ADMITTED:
        return None
    rows = _cdiv(T, STRIDE) * N
    if rows * max(KW, cout) >= 1 << 31:
        return None
    tm = _cdiv(rows, RT)
    f_tn, d_tn, d_nkb = _cdiv(cout, NT), _cdiv(STRIDE * CIN, NT), 4 * cout // KB
    wm, wn = _cdiv(cout, WG_TILE), _cdiv(KW, WG_TILE)
    G = splits if splits > 0 else max(cus // (wm * wn), 1)
    run = _cdiv(_cdiv(rows, G), KB) * KB
    G = _cdiv(rows, run)
    nsub = _cdiv(run, CHAIN)
    sub = _cdiv(_cdiv(run, nsub), KB) * KB
    slab = (cout * KW + cout + 3) // 4 * 4
    nbytes = (f_tn * WIN + d_tn * d_nkb) * B_BLOCK + G * nsub * slab * 4
    return dict(tiles_m=tm, f_tiles_n=f_tn, f_nkb=WIN, f_grid=_cdiv(tm, 8) * 8 * f_tn, d_tiles_n=d_tn, d_nkb=d_nkb,
                splits=G, nsub=nsub, run_rows=run, sub_rows=sub, w_grid=_cdiv(wm * G, 8) * 8 * wn, bytes=nbytes)


def _plan(L, T, N, cout=COUT, cus=CUS):
    out = (ctypes.c_size_t * 12)()
    if not L.tk_lab_conv_strided_plan(T, N, cout, cus, out):
        return None
    return dict(zip(PLAN_KEYS, out))


def test_header_parses_into_the_binding():
    assert set(_lib.CONV_STRIDED_SIGNATURES) == {"tk_conv_strided_supported", "tk_conv_strided_workspace_bytes",
                                                 "tk_conv_strided_forward_dev", "tk_conv_strided_backward_dev"}
    assert set(_lib.CONV_STRIDED_LAB_SIGNATURES) == {"tk_lab_conv_strided_set_splits", "tk_lab_conv_strided_plan"}
    assert len(_lib.CONV_STRIDED_SIGNATURES["tk_conv_strided_forward_dev"][1]) == 12
    assert len(_lib.CONV_STRIDED_SIGNATURES["tk_conv_strided_backward_dev"][1]) == 15
    L = _lib.conv_strided_lib()         # every symbol resolves
    assert not hasattr(L, "tk_lab_conv_strided_plan") or _lib.is_lab()


def test_the_rule_admits_what_is_documented():
    """cin 16, window 19, stride 5 and Cout 192, 256 or 384 (each measured below the GEMM path,
    profiles/r33_convbench.txt, profiles/r33_convbench_sizes.txt): nothing else; the workspace is 0 for an empty
    input, for no CUs and from rows x max(304, Cout) = 2^31 on (the kernels' 32-bit indices), at every size."""
    L = _lib.conv_strided_lib()
    for cout in (4, 16, 96, 128, 192, 255, 256, 257, 384, 512):
        assert bool(L.tk_conv_strided_supported(CIN, cout, WIN, STRIDE)) == (cout in ADMITTED), cout
        assert (L.tk_conv_strided_workspace_bytes(100, 3, cout, CUS) > 0) == (cout in ADMITTED), cout
    for cin, win, stride in [(1, 19, 2), (1, 19, 5), (4, 5, 1), (16, 5, 1), (16, 19, 1), (16, 19, 2), (16, 17, 5),
                             (16, 21, 5), (32, 19, 5), (8, 19, 5)]:
        assert not L.tk_conv_strided_supported(cin, COUT, win, stride), (cin, win, stride)
    ws = L.tk_conv_strided_workspace_bytes
    assert ws(0, 3, COUT, CUS) == 0 and ws(100, 0, COUT, CUS) == 0 and ws(100, 3, COUT, 0) == 0
    for cout in ADMITTED:       # (the layer's one workspace: up to 8192 rows per run, on 256 and on 304 CUs)
        for cus in (CUS, 304):
            for T, N in [(4000, 128), (8000, 64), (5 * 8192 * (cus // 9), 1)]:
                assert ws(T, N, cout, cus) == _plan_py(T, N, cout, cus)["bytes"] <= layers._CONV_STRIDED_WORKSPACE_BYTES
    for cout in ADMITTED:
        edge = _cdiv(1 << 31, max(KW, cout))    # the first number of rows with rows x max(304, Cout) >= 2^31
        assert (edge - 1) * cout < 1 << 31 and (edge - 1) * KW < 1 << 31
        assert ws(5 * (edge - 1), 1, cout, CUS) > 0 and ws(5 * edge, 1, cout, CUS) == 0
        assert ws(5, edge - 1, cout, CUS) > 0 and ws(5, edge, cout, CUS) == 0 and ws(6, edge - 1, cout, CUS) == 0
        assert ws(1 << 40, 1 << 30, cout, CUS) == 0
    assert _cdiv(1 << 31, 384) < _cdiv(1 << 31, KW)     # (Cout 384 is refused before a window's index would overflow)


def test_plan_hook_agrees_with_the_python_rule(labenv):
    labenv.lib()
    L = _lib.conv_strided_lib()
    assert _lib.is_lab()
    flag = _plan(L, 4000, 128)
    assert (flag["tiles_m"], flag["f_grid"], flag["d_nkb"], flag["splits"], flag["nsub"]) == (800, 1600, 64, 42, 1)
    try:
        for splits in (0, 1, 3):
            L.tk_lab_conv_strided_set_splits(splits)
            for T, N in [(1, 1), (4, 1), (5, 63), (6, 65), (23, 100), (641, 1), (641, 63), (641, 100), (4000, 128),
                         (8000, 64), (20000, 128), (5 * 128, 1), (5 * 129, 1), (0, 4), (4, 0)]:
                for cus in (1, 5, 6, 256, 304):
                    want = _plan_py(T, N, cus=cus, splits=splits)
                    assert _plan(L, T, N, cus=cus) == want, (T, N, cus, splits)
                    assert L.tk_conv_strided_workspace_bytes(T, N, COUT, cus) == (want["bytes"] if want else 0)
            assert _plan(L, 100, 3, cout=128) is None
            for cout in ADMITTED:
                assert _plan(L, 641, 100, cout=cout) == _plan_py(641, 100, cout=cout, splits=splits), cout
    finally:
        L.tk_lab_conv_strided_set_splits(0)


def test_bad_arguments_are_refused_before_any_launch():
    """NULL, a misaligned workspace or tensor -> TK_ERR_BAD_ARG, a workspace one byte short -> TK_ERR_WORKSPACE, a
    shape outside the rule or rows x max(304, Cout) >= 2^31 -> TK_ERR_UNSUPPORTED: decided on the host (the pointers are never
    dereferenced: no GPU in this test)."""
    L = _lib.conv_strided_lib()
    T, N = 23, 3
    need = L.tk_conv_strided_workspace_bytes(T, N, COUT, CUS)
    assert need > 0
    names = ("dy", "x", "z", "w", "b", "y", "dz", "dx", "dw", "db", "ws")
    good = {n: ctypes.c_void_p(4096 * (i + 1)) for i, n in enumerate(names)}
    null = ctypes.c_void_p(0)

    def fwd(wsb=need, shape=(T, N, COUT), **kw):
        p = dict(good, **kw)
        return L.tk_conv_strided_forward_dev(p["x"], p["w"], p["b"], *shape, CUS, p["z"], p["y"], p["ws"], wsb, None)

    def bwd(wsb=need, shape=(T, N, COUT), **kw):
        p = dict(good, **kw)
        return L.tk_conv_strided_backward_dev(p["dy"], p["x"], p["z"], p["w"], *shape, CUS, p["dz"], p["dx"], p["dw"],
                                              p["db"], p["ws"], wsb, None)

    for call, needs, aligned in ((fwd, ("x", "w", "b", "y", "ws"), ("x", "z", "y", "ws")),
                                 (bwd, ("dy", "x", "z", "w", "dz", "dw", "db", "ws"), ("dy", "x", "z", "dz", "dx", "ws"))):
        for name in needs:
            assert call(**{name: null}) == BAD_ARG, name
        for name in aligned:
            assert call(**{name: ctypes.c_void_p(4096 + 4)}) == BAD_ARG, name
        assert call(wsb=need - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
        for shape in [(0, N, COUT), (T, 0, COUT)] + [(T, N, c) for c in (128, 192, 255, 384, 512) if c not in ADMITTED]:
            assert call(shape=shape) == UNSUPPORTED, shape
        for cout in ADMITTED:
            edge = _cdiv(1 << 31, max(KW, cout))
            assert call(shape=(5, edge, cout), wsb=1 << 62) == UNSUPPORTED, cout
            assert call(shape=(5, edge - 1, cout), wsb=0) == WORKSPACE, cout


def _layer(cout=COUT):
    return layers.Convolution(CIN, cout, WIN, stride=STRIDE, fun=layers.swish)


def test_cpu_tensors_keep_the_gemm_path():
    torch.manual_seed(3)
    layer = _layer()
    x = torch.randn(23, 3, CIN)
    assert not layer._hip_strided(x)
    want = layers.swish(layer.conv(layer.pad(x.permute(1, 2, 0)))).permute(2, 0, 1)
    assert torch.allclose(layer(x), want, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 64
SHAPES = [(T, N) for T in (1, 4, 5, 6, 9, 10, 19, 23, 641) for N in (1, 63, 65, 100)] + [(4000, 128)]


def _guarded(numel, dev):
    buf = torch.full((GUARD + numel + GUARD,), 7.0, device=dev)
    out = buf[GUARD:GUARD + numel]
    out.fill_(float("nan"))
    return buf, out


def _run(x, w, b, dy, poison=0xFF, want_dx=True, want_z=True):
    """One forward and one backward call on device tensors.  Every output lies between two guard bands over a sentinel,
    the workspace is poisoned and of exactly the size asked; returns y, dx (or None), dw, db."""
    L = _lib.conv_strided_lib()
    T, N, _ = x.shape
    cout = w.shape[0]
    rows = _cdiv(T, STRIDE) * N
    dev = x.device
    wsb = L.tk_conv_strided_workspace_bytes(T, N, cout, CUS)
    assert wsb > 0
    ws = torch.full((wsb,), poison, dtype=torch.uint8, device=dev)
    sizes = dict(z=rows * cout, y=rows * cout, dz=rows * cout, dx=T * N * CIN, dw=cout * KW, db=cout)
    bufs = {k: _guarded(n, dev) for k, n in sizes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    rc = L.tk_conv_strided_forward_dev(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), T, N, cout, CUS,
                                       _lib.ptr(o["z"] if want_z else None), _lib.ptr(o["y"]), _lib.ptr(ws), wsb,
                                       _lib.stream_ptr())
    assert rc == OK
    if want_z:
        ws.fill_(poison)
        rc = L.tk_conv_strided_backward_dev(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(o["z"]), _lib.ptr(w), T, N, cout, CUS,
                                            _lib.ptr(o["dz"]), _lib.ptr(o["dx"] if want_dx else None), _lib.ptr(o["dw"]),
                                            _lib.ptr(o["db"]), _lib.ptr(ws), wsb, _lib.stream_ptr())
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
    tout = _cdiv(T, STRIDE)
    return dict(y=o["y"].view(tout, N, cout).clone(), dx=o["dx"].view(T, N, CIN).clone() if want_dx and want_z else None,
                dw=o["dw"].view(cout, CIN, WIN).clone(), db=o["db"].clone())


def _ref64(x, w, b, dy):
    """nn.Conv1d + swish and their gradients, float64 on the host"""
    conv = nn.Conv1d(CIN, w.shape[0], WIN, stride=STRIDE).double()
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    x = x.double().requires_grad_(True)
    z = conv(nn.functional.pad(x.permute(1, 2, 0), (WIN // 2, (WIN - 1) // 2)))
    y = (z * torch.sigmoid(z)).permute(2, 0, 1)
    (y * dy.double()).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dw=conv.weight.grad, db=conv.bias.grad)


@functools.lru_cache(maxsize=None)
def _inputs(kind, T, N, cout=COUT):
    """x, w, b, dy on the host (float32) and the float64 results.  `kind`: randn; cancel (x = 1 + 2^-10 randn against
    filters that sum to about 0, as tests/test_rnn_proj.py builds it: away from the padding z is made of the correction
    terms)."""
    g = torch.Generator().manual_seed(11 * T + 5 * N + cout + len(kind))
    tout = _cdiv(T, STRIDE)
    x = torch.randn(T, N, CIN, generator=g)
    w = torch.randn(cout, CIN, WIN, generator=g) / KW ** 0.5
    b = torch.randn(cout, generator=g)
    dy = torch.randn(tout, N, cout, generator=g) / (tout * N) ** 0.5
    if kind == "cancel":
        x = 1 + x * 2.0 ** -10
        w = w - w.mean((1, 2), keepdim=True)
        b = torch.zeros(cout)
    return x, w, b, dy, _ref64(x, w, b, dy)


def _gemm_path(x, w, b, dy):
    """what the layer runs with the switch off, on the same device tensors"""
    layer = _layer(w.shape[0]).to(x.device)
    with torch.no_grad():
        layer.conv.weight.copy_(w)
        layer.conv.bias.copy_(b)
    old = layers.USE_HIP_CONV_STRIDED
    layers.USE_HIP_CONV_STRIDED = False
    try:
        x = x.detach().clone().requires_grad_(True)
        y = layer(x)
        (y * dy).sum().backward()
    finally:
        layers.USE_HIP_CONV_STRIDED = old
    return dict(y=y.detach(), dx=x.grad, dw=layer.conv.weight.grad, db=layer.conv.bias.grad)


def _rel(got, ref):
    return (got.double().cpu() - ref).abs().max().item() / (ref.abs().max().item() or 1.0)


def _check(kind, T, N, dev, cout=COUT):
    make = _inputs if T * N <= 100000 else _inputs.__wrapped__       # (the flagship's tensors are not kept)
    x, w, b, dy, ref = make(kind, T, N, cout)
    x, w, b, dy = (v.to(dev) for v in (x, w, b, dy))
    got, gemm = _run(x, w, b, dy), _gemm_path(x, w, b, dy)
    for k in ("y", "dx", "dw", "db"):
        e_hip, e_gemm = _rel(got[k], ref[k]), _rel(gemm[k], ref[k])
        print("conv %s (T, N, Cout) = %s %s: kernel %.3g, GEMM path %.3g" % (kind, (T, N, cout), k, e_hip, e_gemm))
        assert e_hip <= 2 * e_gemm + 2e-6, (kind, T, N, k, e_hip, e_gemm)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("cout", ADMITTED)
@pytest.mark.parametrize("T,N", SHAPES)
def test_against_float64_with_the_gemm_path_as_yardstick(gpu_device, T, N, cout):
    """Windows that are all padding but the centre (T = 1), halos at both ends, T not a multiple of 5, rows on either
    side of a 128-row tile (641 -> 129 windows), and the flagship's shape; guard bands, every element written, the
    workspace poisoned and of exactly the size asked (_run)."""
    _check("randn", T, N, gpu_device, cout)


@pytest.mark.gpu
@pytest.mark.parametrize("cout", ADMITTED)
def test_the_cancelling_input(gpu_device, cout):
    T, N = 641, 65
    x, w, b, _, ref = _inputs("cancel", T, N, cout)
    # ... cancels: in the interior z is below 1 % of the sum of the magnitudes of its products
    xp = nn.functional.pad(x.permute(1, 2, 0).double(), (WIN // 2, (WIN - 1) // 2))
    mags = nn.functional.conv1d(xp.abs(), w.double().abs(), stride=STRIDE)
    z = nn.functional.conv1d(xp, w.double(), stride=STRIDE)
    assert z[:, :, 2:-2].abs().max().item() < 1e-2 * mags[:, :, 2:-2].max().item()
    _check("cancel", T, N, gpu_device, cout)


@pytest.mark.gpu
def test_two_runs_are_bit_identical_whatever_the_workspace_held(gpu_device):
    x, w, b, dy, _ = _inputs("randn", 641, 65)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    one, two, three = _run(x, w, b, dy), _run(x, w, b, dy), _run(x, w, b, dy, poison=0x3F)
    for k in one:
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k
        assert torch.equal(one[k].view(torch.int32), three[k].view(torch.int32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("T", [23, 641])
def test_a_column_alone_has_the_bits_it_has_in_a_batch(gpu_device, T):
    N = 65
    x, w, b, dy, _ = _inputs("randn", T, N)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    full = _run(x, w, b, dy, want_z=False)["y"]
    for n in (0, 31, 64):
        alone = _run(x[:, n:n + 1].contiguous(), w, b, None, want_z=False)["y"]
        assert torch.equal(alone.view(torch.int32), full[:, n:n + 1].contiguous().view(torch.int32)), n


@pytest.mark.gpu
def test_without_dx_and_without_z(gpu_device):
    """dx NULL: dw and db keep their bits and dx is not touched; z NULL (the forward under no_grad): y keeps its bits."""
    x, w, b, dy, _ = _inputs("randn", 23, 63)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    full, nodx, noz = _run(x, w, b, dy), _run(x, w, b, dy, want_dx=False), _run(x, w, b, dy, want_z=False)
    assert nodx["dx"] is None
    for k in ("y", "dw", "db"):
        assert torch.equal(full[k].view(torch.int32), nodx[k].view(torch.int32)), k
    assert torch.equal(full["y"].view(torch.int32), noz["y"].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,splits,want", [(641, 100, 1, (1, 2)), (641, 65, 3, (3, 1)), (23, 63, 1, (1, 1)),
                                             (641, 100, 5, (5, 1))])
def test_forced_runs_and_chain_parts_of_the_weight_gradient(gpu_device, labenv, T, N, splits, want):
    """The lab hook forces the number of runs: one run of 12900 rows is cut into two chain parts, the last block
    ragged (12900 = 806 x 16 + 4); three runs of 8385 rows; one run and one part at 315 rows; five runs."""
    labenv.lib()
    L = _lib.conv_strided_lib()
    assert _lib.is_lab()
    try:
        L.tk_lab_conv_strided_set_splits(splits)
        plan = _plan(L, T, N)
        assert (plan["splits"], plan["nsub"]) == want and (_cdiv(T, STRIDE) * N) % KB != 0
        forced = _check("randn", T, N, gpu_device)
    finally:
        L.tk_lab_conv_strided_set_splits(0)
    free = _check("randn", T, N, gpu_device)
    for k in ("y", "dx"):       # (the forward and dx do not depend on the runs)
        assert torch.equal(forced[k].view(torch.int32), free[k].view(torch.int32)), k


def _layer_grads(layer, x, dy, switch):
    old = layers.USE_HIP_CONV_STRIDED
    layers.USE_HIP_CONV_STRIDED = switch
    try:
        x = x.detach().clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        y = layer(x)
        (y * dy).sum().backward()
    finally:
        layers.USE_HIP_CONV_STRIDED = old
    return dict(y=y.detach().clone(), dx=x.grad, dw=layer.conv.weight.grad.clone(), db=layer.conv.bias.grad.clone())


@pytest.mark.gpu
def test_the_function_through_the_layer(gpu_device):
    """The autograd Function gives the bits of the C calls; an input that needs no gradient gets None from the backward;
    under no_grad, at any T and N >= 1, y has the bits it has in grad mode; either switch off is the GEMM path."""
    T, N = 23, 63
    x, w, b, dy, _ = _inputs("randn", T, N)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    layer = _layer().to(gpu_device)
    with torch.no_grad():
        layer.conv.weight.copy_(w)
        layer.conv.bias.copy_(b)
    assert layer._hip_strided(x)
    abi, got = _run(x, w, b, dy), _layer_grads(layer, x, dy, True)
    for k in abi:
        assert torch.equal(abi[k].view(torch.int32), got[k].view(torch.int32)), k
    # dx not wanted
    layer.zero_grad(set_to_none=True)
    y = layers.StridedConvolution.apply(x, layer.conv.weight, layer.conv.bias, True)
    assert y.grad_fn is not None and y.grad_fn.needs_input_grad[0] is False
    with torch.no_grad():
        grads = layers.StridedConvolution.backward(y.grad_fn, dy)
    assert len(grads) == 4 and grads[0] is None and grads[3] is None
    assert torch.equal(grads[1].view(torch.int32), abi["dw"].view(torch.int32))
    assert torch.equal(grads[2].view(torch.int32), abi["db"].view(torch.int32))
    # no_grad
    with torch.no_grad():
        assert torch.equal(layer(x).view(torch.int32), abi["y"].view(torch.int32))
        for t, n in [(1, 1), (3, 2), (7, 1), (1, 5)]:
            xs = x[:t, :n].contiguous()
            want = _run(xs, w, b, None, want_z=False)["y"]
            assert torch.equal(layer(xs).view(torch.int32), want.view(torch.int32)), (t, n)
    # either switch off: the GEMM path, bit for bit
    off = _layer_grads(layer, x, dy, False)
    old = layers.USE_HIP_CONV
    layers.USE_HIP_CONV = False
    try:
        assert not layer._hip_strided(x)
        off2 = _layer_grads(layer, x, dy, True)
    finally:
        layers.USE_HIP_CONV = old
    for k in off:
        assert torch.equal(off[k].view(torch.int32), off2[k].view(torch.int32)), k


@pytest.mark.gpu
def test_captured_forward_replays_bit_identical(gpu_device):
    torch.manual_seed(7)
    layer = _layer().to(gpu_device)
    x = torch.randn(23, 3, CIN, device=gpu_device)
    assert layer._hip_strided(x)
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
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32))


@pytest.mark.gpu
def test_captured_training_forward_and_backward_replay_bit_identical(gpu_device):
    """The grad-mode forward (z written and saved) and the backward (dz, dx, dW, db) captured into one graph: the replay,
    on new contents of the same input buffers, has the bits of the eager run."""
    T, N = 23, 63
    x, w, b, dy, _ = _inputs("randn", T, N)
    x, w, b, dy = (v.to(gpu_device) for v in (x, w, b, dy))
    layer = _layer().to(gpu_device)
    with torch.no_grad():
        layer.conv.weight.copy_(w)
        layer.conv.bias.copy_(b)
    eager = _layer_grads(layer, x, dy, True)
    sx = torch.zeros_like(x).requires_grad_(True)       # the graph's static inputs, filled before the replay
    sdy = torch.zeros_like(dy)

    def step():
        y = layer(sx)
        grads = torch.autograd.grad(y, [sx, layer.conv.weight, layer.conv.bias], sdy)
        return (y.detach(),) + grads

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    with torch.no_grad():
        sx.copy_(x)
        sdy.copy_(dy)
        for t in out:
            t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for k, t in zip(("y", "dx", "dw", "db"), out):
        assert torch.equal(t.view(torch.int32), eager[k].view(torch.int32)), k


def _parent_forward(self, x):
    """Convolution.forward as it was before this layer had kernels of its own"""
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
    old = layers.USE_HIP_CONV_STRIDED
    layers.USE_HIP_CONV_STRIDED = switch
    try:
        for p in net.parameters():
            p.grad = None
        out = net(x)
        (out * dy).sum().backward()
    finally:
        layers.USE_HIP_CONV_STRIDED = old
    res = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    res["out"] = out.detach().clone()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("make", [models.mLstm_flipflop, models.mLstm_cat_mod_flipflop])
def test_model_with_the_switch_on_and_off(gpu_device, monkeypatch, make):
    """Size 256 on a chunk of 200 samples, 4 columns.  Switch off: the output and every gradient are the bits of the
    layer's forward as it was.  Switch on: they differ from the switch-off run by at most twice what that run differs
    from float64 by, plus 2e-6 (relative to the largest entry)."""
    torch.manual_seed(5)
    net = make(size=256, stride=5)
    x = torch.randn(200, 4, 1)
    dy = torch.randn(*net(x).shape) / 40 ** 0.5
    n64 = copy.deepcopy(net).double()
    ref = _net_grads(n64, x.double(), dy.double(), True)
    net = net.to(gpu_device)
    x, dy = x.to(gpu_device), dy.to(gpu_device)
    on, off = _net_grads(net, x, dy, True), _net_grads(net, x, dy, False)
    with monkeypatch.context() as mp:
        mp.setattr(layers.Convolution, "forward", _parent_forward)
        parent = _net_grads(net, x, dy, True)
    assert set(on) == set(off) == set(parent) == set(ref)
    for k, r in ref.items():
        assert torch.equal(off[k].view(torch.int32), parent[k].view(torch.int32)), k
        scale = r.abs().max().item() or 1.0
        d_on = (on[k] - off[k]).abs().max().item() / scale
        e_off = (off[k].double().cpu() - r).abs().max().item() / scale
        print("%s %s: kernels - GEMM path %.3g, GEMM path - float64 %.3g" % (make.__name__, k, d_on, e_off))
        assert d_on <= 2 * e_off + 2e-6, (k, d_on, e_off)

"""The output layers on the kernels of csrc/out_layer.hip (include/taiyaki_amd_out_layer.h) through the C ABI, with
guard bands around every output and a poisoned workspace, against float64 on the host.  The yardstick is the library
path -- this repository's layer with layers.USE_HIP_OUT_LAYER off, under autograd, on the same device tensors -- and the
criterion that of tests/test_rnn_proj.py and tests/test_lstm_wgrad.py: the error relative to the largest reference entry
at most twice the library's, plus 2e-6.  The shapes are the smallest at which the kernels can go wrong: rows around the
row tile the plan hook names, one case just over one weight-gradient run, the narrowest and the widest input, every
alphabet of the plain layer and two cat-mod ones."""
import ctypes
import functools

import pytest
import torch

from taiyaki_amd import _lib, layers, models

pytestmark = pytest.mark.gpu

CUS = 256
GUARD = 64
SENTINEL = -77.25


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _plan(rows, I, L, O, cus=CUS):
    _lib.use_lab(True)
    try:
        out = (ctypes.c_size_t * 7)()
        assert _lib.out_layer_lib().tk_lab_out_layer_plan(rows, I, L, O, cus, out)
        return dict(zip(("rt", "nt", "nkb", "grid", "runs", "run_rows", "bytes"), out))
    finally:
        _lib.use_lab(False)


R = 128     # the forward's row tile; test_row_tile_is_the_plans checks it against the plan hook


def test_row_tile_is_the_plans():
    assert _plan(1000, 96, 40, 40)["rt"] == R


def _layer(I, spec, seed=0):
    """spec: an int (the plain layer's nbase) or a tuple (the cat-mod layer's can_nmods); float32 on the device."""
    torch.manual_seed(seed)
    layer = layers.GlobalNormFlipFlop(I, spec) if isinstance(spec, int) else layers.GlobalNormFlipFlopCatMod(I, spec)
    with torch.no_grad():
        layer.linear.bias.copy_(0.5 * torch.randn(layer.linear.bias.shape))
    return layer.to(_dev())


def _tables(layer):
    if isinstance(layer, layers.GlobalNormFlipFlopCatMod):
        return layer.out_src, layer.out_group, layer.nout, 5.0
    return None, None, layer.size, float(layer.scale)


def _ints(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _workspace(rows, I, L, cus, poison):
    P = _lib.out_layer_lib()
    wsb = P.tk_out_layer_workspace_bytes(rows, I, L, cus)
    assert wsb > 0
    return torch.full((wsb,), poison, dtype=torch.uint8, device=_dev()), wsb


def _forward(layer, x2, cus=CUS, poison=0xFF):
    """y (rows, O) of one forward call on x2 (rows, I)."""
    P = _lib.out_layer_lib()
    w, b = layer.linear.weight.detach(), layer.linear.bias.detach()
    src, group, O, scale = _tables(layer)
    rows, I = x2.shape
    ws, wsb = _workspace(rows, I, w.shape[0], cus, poison)
    buf, y = _guarded(rows * O, x2.device)
    rc = P.tk_out_layer_forward_dev(_lib.ptr(x2), _lib.ptr(w), _lib.ptr(b), _ints(src), _ints(group), rows, I,
                                    w.shape[0], O, scale, cus, _lib.ptr(y), _lib.ptr(ws), wsb, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert _intact(buf, rows * O)
    return y.view(rows, O).clone()


def _backward(layer, x2, y2, dy2, cus=CUS, poison=0xFF, want_dx=True):
    """dx (rows, I), dw (L, I), db (L) of one backward call."""
    P = _lib.out_layer_lib()
    w = layer.linear.weight.detach()
    src, group, O, scale = _tables(layer)
    rows, I = x2.shape
    L = w.shape[0]
    ws, wsb = _workspace(rows, I, L, cus, poison)
    bx, dx = _guarded(rows * I, x2.device)
    bw, dw = _guarded(L * I, x2.device)
    bb, db = _guarded(L, x2.device)
    rc = P.tk_out_layer_backward_dev(_lib.ptr(dy2), _lib.ptr(y2), _lib.ptr(x2), _lib.ptr(w), _ints(src), _ints(group),
                                     rows, I, L, O, scale, cus, _lib.ptr(dx) if want_dx else None, _lib.ptr(dw),
                                     _lib.ptr(db), _lib.ptr(ws), wsb, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert _intact(bx, rows * I) and _intact(bw, L * I) and _intact(bb, L)
    if not want_dx:
        assert bool((dx == SENTINEL).all())
    return dx.view(rows, I).clone(), dw.view(L, I).clone(), db.clone()


def _reference(layer, x2, dy2):
    """float64 on the host: y, dx, dw, db."""
    ref = type(layer)(x2.shape[1], layer.nbase if isinstance(layer, layers.GlobalNormFlipFlop) else tuple(layer.can_nmods))
    ref = ref.double()
    with torch.no_grad():
        ref.linear.weight.copy_(layer.linear.weight.double().cpu())
        ref.linear.bias.copy_(layer.linear.bias.double().cpu())
    x = x2.double().cpu()[:, None, :].requires_grad_(True)
    y = ref(x)
    y.backward(dy2.double().cpu()[:, None, :])
    return y.detach()[:, 0], x.grad[:, 0], ref.linear.weight.grad, ref.linear.bias.grad


def _library(layer, x2, dy2, monkeypatch):
    """The library path on the same device tensors: the layer with the switch off, under autograd."""
    monkeypatch.setattr(layers, "USE_HIP_OUT_LAYER", False)
    layer.zero_grad()
    x = x2[:, None, :].detach().clone().requires_grad_(True)
    y = layer(x)
    y.backward(dy2[:, None, :])
    out = y.detach()[:, 0], x.grad[:, 0], layer.linear.weight.grad.clone(), layer.linear.bias.grad.clone()
    layer.zero_grad()
    monkeypatch.setattr(layers, "USE_HIP_OUT_LAYER", True)
    return out


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _inputs(rows, I, O, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = (2 * torch.rand(rows, I, generator=g) - 1).to(_dev())
    dy = torch.randn(rows, O, generator=g).to(_dev())
    return x, dy


def _check_accuracy(layer, x, dy, got, monkeypatch, what=""):
    ref = _reference(layer, x, dy)
    lib = _library(layer, x, dy, monkeypatch)
    for name, g, r, l in zip(("y", "dx", "dw", "db"), got, ref, lib):
        e, el = _err(g, r), _err(l, r)
        print("%s %s: kernel %.3g library %.3g" % (what, name, e, el))
        assert e <= 2 * el + 2e-6, (what, name, e, el)


SPECS = [1, 2, 3, 4, (1, 1, 0, 0), (3, 3, 3, 3)]


@pytest.mark.parametrize("I", [16, 96, 384])
@pytest.mark.parametrize("spec", SPECS, ids=str)
def test_accuracy_around_the_row_tile(I, spec, monkeypatch):
    layer = _layer(I, spec)
    O = _tables(layer)[2]
    for rows in (1, R - 1, R, R + 1, 2 * R + 3):
        plan = _plan(rows, I, layer.linear.weight.shape[0], O)
        assert plan["grid"] == -(-rows // R)
        x, dy = _inputs(rows, I, O, seed=rows)
        y = _forward(layer, x)
        got = (y,) + _backward(layer, x, y, dy)
        _check_accuracy(layer, x, dy, got, monkeypatch, "I %d %s rows %d" % (I, spec, rows))


@pytest.mark.parametrize("spec", [4, (1, 1, 0, 0)], ids=str)
@pytest.mark.parametrize("cus", [1, CUS])
def test_just_over_one_weight_gradient_run(spec, cus, monkeypatch):
    """8193 rows at size 384: on one CU a run is 8192 rows, the longest chain, and the second run is one row; on 256
    CUs the runs are 48 rows and the last one is ragged."""
    I, rows = 384, 8193
    layer = _layer(I, spec)
    O = _tables(layer)[2]
    plan = _plan(rows, I, layer.linear.weight.shape[0], O, cus)
    assert (plan["runs"], plan["run_rows"]) == ((2, 8192) if cus == 1 else (171, 48))
    x, dy = _inputs(rows, I, O)
    y = _forward(layer, x, cus)
    got = (y,) + _backward(layer, x, y, dy, cus)
    _check_accuracy(layer, x, dy, got, monkeypatch, "8193 rows, %d CUs" % cus)


@pytest.mark.parametrize("spec", [4, (3, 3, 3, 3)], ids=str)
def test_misaligned_x_takes_the_guarded_loads(spec, monkeypatch):
    I, rows = 96, R + 1
    layer = _layer(I, spec)
    O = _tables(layer)[2]
    x, dy = _inputs(rows, I, O)
    store = torch.empty(rows * I + 1, device=x.device)
    xm = store[1:].view(rows, I)
    xm.copy_(x)
    assert xm.data_ptr() % 16 == 4
    y = _forward(layer, xm)
    assert torch.equal(y, _forward(layer, x))
    got = (y,) + _backward(layer, xm, y, dy)
    _check_accuracy(layer, x, dy, got, monkeypatch, "misaligned")


@pytest.mark.parametrize("spec", [4, (1, 1, 0, 0), (3, 3, 3, 3)], ids=str)
@pytest.mark.parametrize("I", [16, 384])
def test_row_independence(I, spec):
    """Rows [a, b) of a call on all rows equal a call on those rows alone, bit for bit; the same after permuting the
    rows, and on 8 CUs against 256: y and dx."""
    layer = _layer(I, spec)
    O = _tables(layer)[2]
    rows = 2 * R + 3
    x, dy = _inputs(rows, I, O)
    y = _forward(layer, x)
    dx = _backward(layer, x, y, dy)[0]
    for a, b in [(0, 1), (R - 1, R + 1), (37, 37 + R), (rows - 1, rows)]:
        ya = _forward(layer, x[a:b].contiguous())
        assert torch.equal(ya, y[a:b]), (a, b)
        assert torch.equal(_backward(layer, x[a:b].contiguous(), ya, dy[a:b].contiguous())[0], dx[a:b]), (a, b)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(3)).to(x.device)
    yp = _forward(layer, x[perm].contiguous())
    assert torch.equal(yp, y[perm])
    assert torch.equal(_backward(layer, x[perm].contiguous(), yp, dy[perm].contiguous())[0], dx[perm])
    y8 = _forward(layer, x, cus=8)
    assert torch.equal(y8, y)
    assert torch.equal(_backward(layer, x, y, dy, cus=8)[0], dx)


@pytest.mark.parametrize("spec", [4, (1, 1, 0, 0)], ids=str)
def test_backward_is_reproducible_whatever_the_workspace_held(spec):
    I, rows = 96, 2 * R + 3
    layer = _layer(I, spec)
    O = _tables(layer)[2]
    x, dy = _inputs(rows, I, O)
    y = _forward(layer, x, poison=0x00)
    assert torch.equal(y, _forward(layer, x, poison=0xFF))
    one, two = _backward(layer, x, y, dy, poison=0xFF), _backward(layer, x, y, dy, poison=0x7F)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    # dx not wanted: dw and db are the same bits and dx is not touched
    none = _backward(layer, x, y, dy, poison=0x55, want_dx=False)
    assert torch.equal(none[1], one[1]) and torch.equal(none[2], one[2])


@pytest.mark.parametrize("spec", [4, (1, 1, 0, 0)], ids=str)
def test_a_nan_stays_in_its_row(spec):
    I, rows = 96, R + 5
    layer = _layer(I, spec)
    O = _tables(layer)[2]
    x, _ = _inputs(rows, I, O)
    clean = _forward(layer, x)
    for bad in (0, 40, R - 1, rows - 1):
        xb = x.clone()
        xb[bad, 17] = float("nan")
        y = _forward(layer, xb)
        finite = torch.isfinite(y).all(dim=1)
        assert not bool(torch.isfinite(y[bad]).any())
        keep = torch.ones(rows, dtype=torch.bool, device=x.device)
        keep[bad] = False
        assert bool(finite[keep].all()) and torch.equal(y[keep], clean[keep])


@pytest.mark.parametrize("spec", [4, (1, 1, 0, 0)], ids=str)
def test_saturation_is_exact(spec):
    """The bias shifted by +-30 in two tanh columns: y is exactly +-scale there, dz exactly 0, so dw's rows and db's
    entries of those columns are exactly 0."""
    I, rows = 96, R + 1
    layer = _layer(I, spec)
    O, scale = _tables(layer)[2:]
    with torch.no_grad():
        layer.linear.bias[3] += 30.0
        layer.linear.bias[11] -= 30.0
    x, dy = _inputs(rows, I, O)
    y = _forward(layer, x)
    assert bool((y[:, 3] == scale).all()) and bool((y[:, 11] == -scale).all())
    dx, dw, db = _backward(layer, x, y, dy)
    assert bool((dw[3] == 0).all()) and bool((dw[11] == 0).all()) and float(db[3]) == 0.0 and float(db[11]) == 0.0
    assert bool((dw[4] != 0).any()) and bool(torch.isfinite(dx).all())


@pytest.mark.parametrize("spec", [(1, 1, 0, 0), (3, 3, 3, 3), (2, 0, 1, 0)], ids=str)
def test_cat_mod_groups(spec):
    """Every group of y exponentiates to a sum within 1e-6 of 1, and the canonical column of dz receives from every
    group: with dy 1 on one group's outputs alone db of that column is the sum over rows of (1 - n exp(y canonical))
    of that group, whichever the group."""
    I, rows = 96, R + 1
    layer = _layer(I, spec)
    O = layer.nout
    nt = layer.ntrans_states
    x, _ = _inputs(rows, I, O)
    y = _forward(layer, x)
    off = layer.can_mods_offsets
    for k in range(layer.ncan_base):
        grp = y[:, nt + off[k]:nt + off[k + 1]].double()
        assert float((grp.exp().sum(1) - 1).abs().max()) <= 1e-6, k
        dy = torch.zeros(rows, O, device=x.device)
        dy[:, nt + off[k]:nt + off[k + 1]] = 1.0
        db = _backward(layer, x, y, dy)[2]
        n = int(off[k + 1] - off[k])
        want = float((1.0 - n * grp[:, 0].exp()).sum())
        assert abs(float(db[nt]) - want) <= 1e-4 * max(1.0, abs(want)) + 1e-4, (k, float(db[nt]), want)
        if n == 1:      # log_softmax of one entry: y = 0 and no gradient at all
            assert bool((grp == 0).all()) and float(db[nt]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [4, (1, 1, 0, 0)], ids=str)
def test_module_forward_and_backward(spec, monkeypatch):
    I, T, N = 96, 33, 5
    layer = _layer(I, spec)
    O = _tables(layer)[2]
    x2, dy2 = _inputs(T * N, I, O)
    monkeypatch.setattr(layers, "USE_HIP_OUT_LAYER", True)
    monkeypatch.setattr(layers, "OUT_LAYER_GRAD_MIN_ROWS", 0)
    monkeypatch.setattr(layers, "OUT_LAYER_PLAIN_GRAD_MIN_ROWS", 0)
    calls = dict(layers.out_layer_calls)
    layer.zero_grad()
    x = x2.view(T, N, I).clone().requires_grad_(True)
    y = layer(x)
    assert layers.out_layer_calls == {"forward": calls["forward"] + 1, "backward": calls["backward"]}
    y.backward(dy2.view(T, N, O))
    assert layers.out_layer_calls == {"forward": calls["forward"] + 1, "backward": calls["backward"] + 1}
    got = (y.detach().view(T * N, O), x.grad.view(T * N, I), layer.linear.weight.grad.clone(),
           layer.linear.bias.grad.clone())
    _check_accuracy(layer, x2, dy2, got, monkeypatch, "module")
    with torch.no_grad():
        calls = dict(layers.out_layer_calls)
        full = layer(x2.view(T, N, I))
        assert layers.out_layer_calls["forward"] == calls["forward"] + 1
        assert torch.equal(full, y.detach())
        for n in range(N):
            assert torch.equal(full[:, n:n + 1], layer(x2.view(T, N, I)[:, n:n + 1])), n


@pytest.mark.parametrize("spec", [4, (1, 1, 0, 0)], ids=str)
def test_captured_forward_replays_to_the_eager_bits(spec):
    I, T, N = 96, 33, 5
    layer = _layer(I, spec)
    x = _inputs(T * N, I, 1)[0].view(T, N, I)
    static = torch.zeros_like(x)
    with torch.no_grad():
        eager = layer(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            layer(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = layer(static)
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
def test_a_reads_scores_do_not_depend_on_its_batch():
    """models.mGru_flipflop(size=96, stride=2), T = 64, N = 5, under no_grad: column n of the batch's scores against
    the scores of column n run alone.  Every layer in front of the output layer documents row or column independence;
    where model[:-1] keeps it the whole model must, and from the output layer's input onward it must in any case."""
    torch.manual_seed(5)
    model = models.mGru_flipflop(size=96, stride=2).to(_dev()).eval()
    x = torch.randn(64, 5, 1, device=_dev())
    with torch.no_grad():
        calls = layers.out_layer_calls["forward"]
        head = torch.nn.Sequential(*list(model)[:-1])
        front, whole = head(x), model(x)
        assert layers.out_layer_calls["forward"] == calls + 1
        front_alone = [head(x[:, n:n + 1].contiguous()) for n in range(5)]
        front_holds = all(torch.equal(front[:, n:n + 1], front_alone[n]) for n in range(5))
        for n in range(5):      # from the output layer's input onward, in any case
            assert torch.equal(whole[:, n:n + 1], model[-1](front[:, n:n + 1])), n
        assert front_holds, "a layer in front of the output layer depends on the batch"
        for n in range(5):
            assert torch.equal(whole[:, n:n + 1], model(x[:, n:n + 1].contiguous())), n

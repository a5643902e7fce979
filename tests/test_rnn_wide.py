"""The recurrences at every batch width (include/taiyaki_amd_rnn_wide.h, libtaiyaki_amd_rnn_wide.so): a batch wider than
one launch admits runs as slabs of columns, one admitted launch after the other, in place on the whole-batch tensors.

The rule under test: slab k's rows of every output are, bit for bit, what the existing call with per-column lengths
writes on contiguous copies of that slab's columns at the same cu_count; a batch that one launch admits is the existing
call.  The cut is read from tk_rnn_wide_slab, never inferred from the shape.  cu_count is only ever made SMALLER than the
device's count (to cut small batches): a grid beyond the real count could wait for ever.

Every launch at the C ABI asserts return code 0 and status word 0 behind the synchronise; after a non-zero status this
module launches nothing more (the remaining tests fail at once).  Outputs are NaN before every launch."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from taiyaki_amd import _lib, layers
from tests import test_rnn_instantiations as insts

KIND = {"lstm": 0, "gru": 1}
NG = {"lstm": 4, "gru": 3}
MANY = 1 << 20              # a batch no launch admits at the sizes whose workgroups hand h on
_allowed = insts._allowed


def _real_cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the header, the library, the binding and the two host functions
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = {"tk_rnn_wide_workspace_bytes", "tk_rnn_wide_slab", "tk_lstm_forward_wide_dev", "tk_lstm_backward_wide_dev",
           "tk_gru_forward_wide_dev", "tk_gru_backward_wide_dev"}
# README's admission bounds on 256 CUs: (cell, size) -> the widest admitted batch
BOUNDS_256 = {("lstm", 384): 128, ("lstm", 256): 256, ("lstm", 192): 512, ("lstm", 128): 512,
              ("gru", 384): 256, ("gru", 256): 256, ("gru", 192): 512}


def test_wide_library_exports_exactly_what_its_header_declares():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.WIDE_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^(?:const\s+)?[a-z_0-9]+\s+\*?\s*([a-z_0-9]+)\(", hdr, flags=re.M))
    assert declared == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib.WIDE_LIBNAME)],
                         capture_output=True, text=True, check=True).stdout
    assert {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"} == declared
    assert set(_lib.WIDE_SIGNATURES) == declared


def test_wide_binding_has_the_argument_types_of_its_twins():
    """The four calls take the arguments of their twins in include/taiyaki_amd_rnn_varlen_train.h, in their order."""
    sz, i = ctypes.c_size_t, ctypes.c_int
    twins = {"tk_lstm_forward_wide_dev": "tk_lstm_forward_varlen_save_dev",
             "tk_lstm_backward_wide_dev": "tk_lstm_backward_varlen_dev",
             "tk_gru_forward_wide_dev": "tk_gru_forward_varlen_save_dev",
             "tk_gru_backward_wide_dev": "tk_gru_backward_varlen_dev"}
    want = {wide: _lib.VARLEN_TRAIN_SIGNATURES[twin] for wide, twin in twins.items()}
    want["tk_rnn_wide_workspace_bytes"] = want["tk_rnn_wide_slab"] = (sz, [i, sz, sz, i])
    assert _lib.WIDE_SIGNATURES == want
    assert _lib.rnn_wide_lib() is _lib.rnn_wide_lib()


def test_slab_is_the_admission_bound_on_256_cus():
    W = _lib.rnn_wide_lib()
    for (cell, h), bound in BOUNDS_256.items():
        assert W.tk_rnn_wide_slab(KIND[cell], MANY, h, 256) == bound, (cell, h)
        assert W.tk_rnn_wide_slab(KIND[cell], bound + 1, h, 256) == bound, (cell, h)
        for n in (1, bound - 1, bound):                    # one launch admits the batch: the batch itself
            assert W.tk_rnn_wide_slab(KIND[cell], n, h, 256) == n, (cell, h, n)
    for n in (1, 300, MANY):                                # one workgroup owns every unit: any batch is one launch
        assert W.tk_rnn_wide_slab(KIND["gru"], n, 96, 256) == n
    for kind in (0, 1):
        assert W.tk_rnn_wide_slab(kind, 0, 256, 256) == 0 and W.tk_rnn_wide_slab(kind, 5, 256, 0) == 0
        assert W.tk_rnn_wide_slab(kind, 5, 256, 3) == 0     # a group of the size does not fit 3 CUs
    assert W.tk_rnn_wide_slab(2, 5, 256, 256) == 0 and W.tk_rnn_wide_slab(-1, 5, 256, 256) == 0
    assert W.tk_rnn_wide_slab(0, 5, 96, 256) == 0 and W.tk_rnn_wide_slab(0, 5, 512, 256) == 0


def test_workspace_is_the_training_pairs_at_the_widest_slab():
    W, V, L = _lib.rnn_wide_lib(), _lib.varlen_train_lib(), _lib.lib()
    VL = _lib.varlen_lib()
    q, train = W.tk_rnn_wide_workspace_bytes, V.tk_rnn_varlen_train_workspace_bytes
    for (cell, h), S in list(BOUNDS_256.items()) + [(("gru", 96), MANY)]:
        kind = KIND[cell]
        for n in (1, S, S + 1, 3 * S + 1):
            want = train(kind, min(n, S), h, 256)
            assert want > 0 and q(kind, n, h, 256) == want, (cell, h, n)
        if S == MANY:
            continue
        # the existing queries still refuse the batch one column wider than the bound
        plain = L.tk_lstm_workspace_bytes if cell == "lstm" else L.tk_gru_workspace_bytes
        assert plain(S + 1, h, 256) == 0 and train(kind, S + 1, h, 256) == 0, (cell, h)
        assert VL.tk_rnn_varlen_workspace_bytes(kind, S + 1, h, 256) == 0, (cell, h)
    for h in (96, 512):
        assert q(0, 5, h, 256) == 0 and q(0, MANY, h, 256) == 0
    for kind in (0, 1):
        assert q(kind, 0, 256, 256) == 0 and q(kind, 5, 256, 0) == 0 and q(kind, 5, 256, -1) == 0
        assert q(kind, 5, 256, 3) == 0
    assert q(2, 5, 256, 256) == 0 and q(-1, 5, 256, 256) == 0


def test_entries_check_their_arguments_before_anything_is_launched():
    W = _lib.rnn_wide_lib()
    bad, unsupported, short = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED", "WORKSPACE"))
    p, big = ctypes.c_void_p(4096), 1 << 30
    assert W.tk_lstm_backward_wide_dev(None, None, None, None, None, 4, 300, 256, 0, 256, None, None, 0, None, None) == bad
    assert W.tk_gru_forward_wide_dev(None, None, None, None, 4, 300, 256, 0, 256, None, None, None, None, 0, None,
                                     None) == bad
    # one of the two saved tensors NULL alone
    assert W.tk_lstm_forward_wide_dev(p, p, None, 4, 300, 256, 0, 256, p, p, None, p, big, p, None) == bad
    assert W.tk_lstm_forward_wide_dev(p, p, None, 4, 300, 256, 0, 256, p, None, p, p, big, p, None) == bad
    assert W.tk_gru_forward_wide_dev(p, p, p, None, 4, 300, 256, 0, 256, p, p, None, p, big, p, None) == bad
    # sizes the kernels do not cover, no batch, no CUs; a short workspace
    assert W.tk_lstm_forward_wide_dev(p, p, None, 4, 300, 96, 0, 256, p, p, p, p, big, p, None) == unsupported
    assert W.tk_lstm_forward_wide_dev(p, p, None, 4, 0, 256, 0, 256, p, p, p, p, big, p, None) == unsupported
    assert W.tk_gru_backward_wide_dev(p, p, p, p, p, None, 4, 300, 256, 0, 0, p, p, p, big, p, None) == unsupported
    assert W.tk_lstm_backward_wide_dev(p, p, p, p, None, 4, 300, 256, 0, 256, p, p, 16, p, None) == short
    assert W.tk_gru_backward_wide_dev(p, p, p, p, p, None, 4, 300, 256, 0, 256, p, p, p, 16, p, None) == short
    # nothing to do at nblk = 0, behind the checks
    assert W.tk_lstm_forward_wide_dev(p, p, None, 0, 300, 256, 0, 256, p, p, p, p, big, p, None) == 0


def test_layers_have_the_switch_the_query_and_the_counter():
    assert layers.USE_HIP_RNN_WIDE is True and layers.rnn_wide_calls.keys() == {"saved", "inference"}
    lstm = layers.Lstm(4, 256)
    assert layers.hip_rnn_wide_workspace_bytes(lstm.rnn, torch.zeros(3, 300, 4)) == 0          # a CPU tensor
    assert {k for k in layers._RNN_LAUNCHES if k[0] == "wide"} == {("wide", True), ("wide", False)}


# ---------------------------------------------------------------------------------------------------------------------
# GPU 1: the C ABI, bit for bit against the existing entries slab by slab
# ---------------------------------------------------------------------------------------------------------------------
_stopped = []           # the first non-zero status word or return code of this module's own launches
GUARD = 256             # floats in front of and behind every output of a wide call


@pytest.fixture(autouse=True)
def _nothing_after_a_bad_status():
    if _stopped:
        pytest.fail("not run: an earlier launch of this module ended with %s" % (_stopped[0],))


def _launch(L, name, ins, dims, outs, wsb, dev):
    """One call: the pointers, (T, N, H, reverse, cu_count), the outputs, a workspace of its own and a status word."""
    assert wsb > 0, name
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    P = _lib.ptr
    rc = getattr(L, name)(*[P(t) for t in ins], *dims, *[P(t) for t in outs], P(ws), wsb, P(status),
                          _lib.stream_ptr())
    if rc != 0:
        _stopped.append((name, "rc", rc))
    _lib.check(rc, name)
    torch.cuda.synchronize()
    word = int(status.item())
    if word != 0:
        _stopped.append((name, "status", word))
    assert word == 0, (name, word)


def _guarded(shape, dev):
    """A NaN tensor of `shape` with GUARD NaN floats on both sides -> (the whole buffer, the tensor)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _case(kind, H, N, T, dev, seed):
    g = torch.Generator().manual_seed(seed)
    ng = NG[kind]
    t = {"gx": torch.randn(T, N, ng * H, generator=g), "whh": torch.randn(ng * H, H, generator=g) / H ** 0.5,
         "dy": torch.randn(T, N, H, generator=g)}
    if kind == "gru":
        t["bhh"] = 0.1 * torch.randn(ng * H, generator=g)
    return {k: v.to(dev) for k, v in t.items()}


def _fwd_ins(kind, t, lens):
    return (t["gx"], t["whh"]) + ((t["bhh"],) if kind == "gru" else ()) + (lens,)


def _bwd_ins(kind, t, out, lens):
    saved = (out["gates"], out["c"])
    return (t["whh"],) + (((out["y"],) + saved) if kind == "gru" else saved) + (t["dy"], lens)


def _shapes(kind, T, N, H, save):
    s = {"y": (T, N, H)}
    if save:
        s.update(gates=(T, N, NG[kind] * H), c=(T, N, H), dgates=(T, N, NG[kind] * H))
        if kind == "gru":
            s["dq"] = (T, N, H)
    return s


def _wide(kind, t, lens, rev, cus, save):
    """The wide forward and, with `save`, the wide backward on the whole batch: every output NaN before its launch and
    guarded on both sides; behind the launches no NaN is left inside and every guard is still NaN."""
    T, N, HG = t["gx"].shape
    H, dev, W = HG // NG[kind], t["gx"].device, _lib.rnn_wide_lib()
    wsb = W.tk_rnn_wide_workspace_bytes(KIND[kind], N, H, cus)
    bufs, out = {}, {}
    for k, shape in _shapes(kind, T, N, H, save).items():
        bufs[k], out[k] = _guarded(shape, dev)
    dims = (T, N, H, rev, cus)
    _launch(W, "tk_%s_forward_wide_dev" % kind, _fwd_ins(kind, t, lens), dims,
            (out["y"], out.get("gates"), out.get("c")), wsb, dev)
    if save:
        _launch(W, "tk_%s_backward_wide_dev" % kind, _bwd_ins(kind, t, out, lens), dims,
                (out["dgates"],) + ((out["dq"],) if kind == "gru" else ()), wsb, dev)
    for k, buf in bufs.items():
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), (k, "a guard was written")
        assert bool(torch.isfinite(out[k]).all()), (k, "an element was not written")
    return out


def _existing(kind, t, lens, rev, cus, save):
    """The existing calls on a batch that one launch admits: tk_*_forward_varlen_save_dev and tk_*_backward_varlen_dev
    (`save`), or tk_*_forward_varlen_dev, which saves nothing."""
    T, N, HG = t["gx"].shape
    H, dev = HG // NG[kind], t["gx"].device
    out = {k: torch.full(shape, float("nan"), device=dev) for k, shape in _shapes(kind, T, N, H, save).items()}
    dims = (T, N, H, rev, cus)
    if not save:
        V = _lib.varlen_lib()
        _launch(V, "tk_%s_forward_varlen_dev" % kind, _fwd_ins(kind, t, lens), dims, (out["y"],),
                V.tk_rnn_varlen_workspace_bytes(KIND[kind], N, H, cus), dev)
        return out
    V = _lib.varlen_train_lib()
    wsb = V.tk_rnn_varlen_train_workspace_bytes(KIND[kind], N, H, cus)
    _launch(V, "tk_%s_forward_varlen_save_dev" % kind, _fwd_ins(kind, t, lens), dims,
            (out["y"], out["gates"], out["c"]), wsb, dev)
    _launch(V, "tk_%s_backward_varlen_dev" % kind, _bwd_ins(kind, t, out, lens), dims,
            (out["dgates"],) + ((out["dq"],) if kind == "gru" else ()), wsb, dev)
    return out


def _gru384_cut(S, N, cus):
    """gru_plan at H = 384: the full slabs need 8 columns per workgroup, the remainder fits with 4."""
    return S == 8 * (cus // 8) and S < N and -(-(N % S) // 4) * 8 <= cus < -(-S // 4) * 8


def _lstm256_cut(S, N, cus):
    """the remainder plans another column count than the full slabs (the library's own plan, through its lab hook)"""
    full, rest = insts._lab_lstm_inst(S, 256, cus), insts._lab_lstm_inst(N % S, 256, cus)
    return S < N and full is not None and rest is not None and full[2] != rest[2]


# name -> (cell, size, the cu_count wanted, N from the slab width S of a batch no launch admits, the intended cut)
CASES = {
    "lstm64-two-slabs-and-a-remainder": ("lstm", 64, 4, lambda S: 2 * S + 5, lambda S, N, cus: N // S == 2 and N % S),
    "lstm256-remainder-plans-other-columns": ("lstm", 256, 16, lambda S: S + 5, _lstm256_cut),
    "lstm384-48-units": ("lstm", 384, 8, lambda S: 2 * S + 3, lambda S, N, cus: N // S == 2 and N % S),
    "lstm192-48-units": ("lstm", 192, 4, lambda S: S + 3, lambda S, N, cus: S == 8 * (cus // 4) and N // S == 1),
    "gru256": ("gru", 256, 4, lambda S: 2 * S + 1, lambda S, N, cus: N // S == 2 and N % S == 1),
    "gru384-4-and-8-columns": ("gru", 384, 8, lambda S: S + 3, _gru384_cut),
    "gru96-one-slab": ("gru", 96, 4, lambda S: 7, lambda S, N, cus: S == N),
    "lstm64-batch-is-the-slab": ("lstm", 64, 4, lambda S: S, lambda S, N, cus: S == N),
    "lstm64-narrower-than-the-slab": ("lstm", 64, 4, lambda S: 5, lambda S, N, cus: S == N),
    "gru256-batch-is-the-slab": ("gru", 256, 4, lambda S: S, lambda S, N, cus: S == N),
}


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["null-lengths", "ragged"])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("case", list(CASES))
def test_wide_call_equals_the_existing_calls_slab_by_slab(gpu_device, case, T, rev, ragged):
    kind, H, wanted, batch_of, cut = CASES[case]
    dev, W = gpu_device, _lib.rnn_wide_lib()
    cus = min(wanted, _real_cus(dev))
    N = batch_of(W.tk_rnn_wide_slab(KIND[kind], MANY, H, cus))
    S = W.tk_rnn_wide_slab(KIND[kind], N, H, cus)
    if not (0 < S <= N and cut(S, N, cus)):
        pytest.skip("%d CUs do not cut %d columns as this case intends (slab %d)" % (cus, N, S))
    t = _case(kind, H, N, T, dev, 1000 * H + 10 * T + rev)
    host = insts.lengths_for(N, T) if ragged else None
    assert host is None or {0, T} <= set(host)
    lens = None if host is None else torch.tensor(host, dtype=torch.int32, device=dev)
    for save in (True, False):
        got = _wide(kind, t, lens, rev, cus, save)
        for a in range(0, N, S):
            b = min(a + S, N)
            part = {k: (v if k in ("whh", "bhh") else v[:, a:b].contiguous()) for k, v in t.items()}
            want = _existing(kind, part, None if lens is None else lens[a:b].contiguous(), rev, cus, save)
            assert set(want) == set(got)
            for k, v in want.items():
                assert bool(torch.isfinite(v).all()), (case, k)
                assert torch.equal(got[k][:, a:b], v), (case, "save" if save else "nothing saved", "columns", a, b, k)
        if host is not None:
            beyond = torch.arange(T, device=dev)[:, None] >= lens[None, :]
            assert all(not v[beyond].any() for v in got.values()), "rows at and beyond a length are not exactly 0"


# ---------------------------------------------------------------------------------------------------------------------
# GPU 2: the layers at the device's own CU count, at the narrowest widths its admission refuses
# ---------------------------------------------------------------------------------------------------------------------
def _grads(layer, call, x, dy):
    x = x.detach().clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    y = call(layer, x)
    (y * dy).sum().backward()
    rnn = layer.layer.rnn if isinstance(layer, layers.Reverse) else layer.rnn
    out = {"y": y, "x": x.grad, "w_ih": rnn.weight_ih_l0.grad, "w_hh": rnn.weight_hh_l0.grad, "b_ih": rnn.bias_ih_l0.grad}
    return {k: v.detach().clone() for k, v in out.items()}


def _refused_width(cell, H, dev):
    """S + 5 columns, S the widest batch one launch admits on this device."""
    S = _lib.rnn_wide_lib().tk_rnn_wide_slab(KIND[cell], MANY, H, _real_cus(dev))
    if not 0 < S < MANY:
        pytest.skip("no batch is refused at size %d on %d CUs" % (H, _real_cus(dev)))
    return S + 5


def _existing_queries(rnn, x):
    plain = layers.hip_lstm_workspace_bytes if isinstance(rnn, torch.nn.LSTM) else layers.hip_gru_workspace_bytes
    return (plain(rnn, x), layers.hip_rnn_varlen_workspace_bytes(rnn, x),
            layers.hip_rnn_varlen_train_workspace_bytes(rnn, x))


@pytest.mark.gpu
@pytest.mark.parametrize("with_lengths", [False, True], ids=["plain", "lengths"])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cell,H", [("lstm", 384), ("lstm", 256), ("gru", 384)])
def test_layer_wider_than_one_launch_matches_float64(gpu_device, monkeypatch, cell, H, reverse, with_lengths):
    """y, dx and every parameter gradient of the layer on the slabs against the float64 layer: as close as 2 x the
    nn.LSTM / nn.GRU path's own error + 2e-6, each error over the tensor's largest entry."""
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    dev, T, I = gpu_device, 4, 16
    N = _refused_width(cell, H, dev)
    torch.manual_seed(H + 2 * reverse + with_lengths)
    inner = layers.Lstm(I, H) if cell == "lstm" else layers.GruMod(I, H)
    layer = layers.Reverse(inner) if reverse else inner
    x, dy = torch.randn(T, N, I), torch.randn(T, N, H) / (T * N) ** 0.5
    lens = insts.lengths_for(N, T) if with_lengths else None
    call = (lambda m, v: m(v)) if lens is None else (lambda m, v: m(v, lengths=lens))
    ref = _grads(layer.double(), call, x.double(), dy.double())
    layer = layer.float().to(dev)
    xg, dyg = x.to(dev), dy.to(dev)
    assert _existing_queries(inner.rnn, xg) == (0, 0, 0) and layers.hip_rnn_wide_workspace_bytes(inner.rnn, xg) > 0
    before = dict(layers.rnn_wide_calls)
    hip = _grads(layer, call, xg, dyg)
    assert layers.rnn_wide_calls == dict(before, saved=before["saved"] + 1), "not the wide entries"
    monkeypatch.setattr(layers, "USE_HIP_LSTM" if cell == "lstm" else "USE_HIP_GRU", False)
    assert layers.hip_rnn_wide_workspace_bytes(inner.rnn, xg) == 0
    miopen = _grads(layer, call, xg, dyg)
    assert layers.rnn_wide_calls == dict(before, saved=before["saved"] + 1)
    _lib.raise_if_nonfinite()
    for k, r in ref.items():
        scale = r.abs().max().item()
        assert scale > 0, k
        e_hip = (hip[k].double().cpu() - r).abs().max().item() / scale
        e_mio = (miopen[k].double().cpu() - r).abs().max().item() / scale
        print("%s %d N %d rev %d lengths %d %s: slabs %.3e, nn.%s %.3e, ratio %.3f"
              % (cell, H, N, reverse, with_lengths, k, e_hip, cell.upper(), e_mio, e_hip / _allowed(e_mio)))
        assert e_hip <= _allowed(e_mio), (cell, H, N, reverse, with_lengths, k, e_hip, e_mio)
    if lens is not None:
        beyond = torch.arange(T)[:, None] >= torch.tensor(lens)[None, :]
        assert not hip["y"].cpu()[beyond].any() and not hip["x"].cpu()[beyond].any()


@pytest.mark.gpu
@pytest.mark.parametrize("cell,H", [("lstm", 256), ("gru", 384)])
def test_switch_off_is_the_fallback_and_inference_saves_nothing(gpu_device, monkeypatch, cell, H):
    dev, T, I = gpu_device, 4, 16
    N = _refused_width(cell, H, dev)
    torch.manual_seed(H)
    layer = (layers.Lstm(I, H) if cell == "lstm" else layers.GruMod(I, H)).to(dev)
    x = torch.randn(T, N, I, device=dev)
    lens = insts.lengths_for(N, T)
    with torch.no_grad():
        before = dict(layers.rnn_wide_calls)
        y, yl = layer(x), layer(x, lengths=lens)
        # no lengths: each layer's own choice of what it saves; lengths under no_grad: the forward that saves nothing
        plain = "saved" if cell == "lstm" else "inference"
        want = dict(before)
        want[plain] += 1
        want["inference"] += 1
        assert layers.rnn_wide_calls == want
        monkeypatch.setattr(layers, "USE_HIP_RNN_WIDE", False)
        assert layers.hip_rnn_wide_workspace_bytes(layer.rnn, x) == 0
        off = layer(x)
        assert layers.rnn_wide_calls == want, "the switch is off and the counter moved"
        monkeypatch.setattr(layers, "USE_HIP_LSTM" if cell == "lstm" else "USE_HIP_GRU", False)
        assert torch.equal(off, layer(x)), "with the switch off a wide batch is nn.LSTM / nn.GRU, as before"
    _lib.raise_if_nonfinite()
    assert (y - off).abs().max().item() <= 1e-5 * off.abs().max().item()
    full = torch.tensor(lens, device=dev) == T
    assert torch.equal(yl[:, full], y[:, full]), "a full-length column is the column of the call without lengths"
    assert not yl[torch.arange(T, device=dev)[:, None] >= torch.tensor(lens, device=dev)[None, :]].any()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 3: a captured forward is a linear chain, and replays bit-identical
# ---------------------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime this process has loaded (the one that owns the captured graph)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 is loaded")


def _graph_edges(graph):
    """(number of nodes, [(from, to)]) of a hipGraph_t."""
    hip, vp = _hip_runtime(), ctypes.c_void_p
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = n.value
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(n)) == 0
    src, dst = (vp * max(n.value, 1))(), (vp * max(n.value, 1))()
    assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(n)) == 0
    return nodes, [(src[i], dst[i]) for i in range(n.value)]


@pytest.mark.gpu
def test_captured_wide_forward_is_a_linear_chain_and_replays_bit_identical(gpu_device):
    dev, T, I, H = gpu_device, 4, 16, 256
    N = _refused_width("lstm", H, dev)
    torch.manual_seed(11)
    layer = layers.Lstm(I, H).to(dev)
    x0, x1 = torch.randn(T, N, I, device=dev), torch.randn(T, N, I, device=dev)
    assert layers.hip_lstm_workspace_bytes(layer.rnn, x0) == 0 and layers.hip_rnn_wide_workspace_bytes(layer.rnn, x0) > 0
    strict = _lib.is_strict()
    _lib.set_strict(False)
    try:
        with torch.no_grad():
            eager0, eager1 = layer(x0), layer(x1)
            static = x0.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                layer(static)
            torch.cuda.current_stream().wait_stream(side)
            before = dict(layers.rnn_wide_calls)
            g = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(g):
                out = layer(static)
            assert layers.rnn_wide_calls == dict(before, saved=before["saved"] + 1)
            nodes, edges = _graph_edges(g.raw_cuda_graph())
            slabs = -(-N // _lib.rnn_wide_lib().tk_rnn_wide_slab(0, N, H, _real_cus(dev)))
            print("captured wide forward: %d nodes, %d edges, %d slabs" % (nodes, len(edges), slabs))
            # one stream, one chain: every node but the last has one successor, every node but the first one predecessor
            assert nodes >= 2 * slabs and len(edges) == nodes - 1, (nodes, len(edges))
            assert len({a for a, _ in edges}) == len(edges) == len({b for _, b in edges}), "a node forks or joins"
            for xin, want in ((x0, eager0), (x1, eager1), (x0, eager0)):
                static.copy_(xin)
                out.fill_(float("nan"))
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, want)
        _lib.raise_if_nonfinite()
    finally:
        _lib.set_strict(strict)


# ---------------------------------------------------------------------------------------------------------------------
# GPU 4: the whole model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_wider_than_one_launch_matches_float64(gpu_device):
    """One calculate_loss + backward of mLstm_flipflop(size=384) at chunk length 200 (T = 40) and S + 5 chunks: every
    Lstm layer takes the slabs, and the loss and every parameter gradient are as close to the float64 model as 2 x the
    nn.LSTM path's own error + 2e-6."""
    from taiyaki_amd import models
    from tests import test_lstm_sizes as sizes
    dev, size = gpu_device, 384
    N = _refused_width("lstm", size, dev)
    torch.manual_seed(size)
    net = models.mLstm_flipflop(size=size, stride=5).to(dev)
    batch = sizes._model_batch("flipflop", 200, N, dev)
    lstms = [m for m in net.modules() if isinstance(m, layers.Lstm)]
    probe = torch.zeros(40, N, size, device=dev)
    assert len(lstms) == 5 and all(layers.hip_lstm_workspace_bytes(m.rnn, probe) == 0 for m in lstms)
    assert all(layers.hip_rnn_wide_workspace_bytes(m.rnn, probe) > 0 for m in lstms)
    before = dict(layers.rnn_wide_calls)
    hip = sizes._loss_and_grads(net, batch)
    assert layers.rnn_wide_calls == dict(before, saved=before["saved"] + 5), "a layer did not take the slabs"
    old = layers.USE_HIP_LSTM
    try:
        layers.USE_HIP_LSTM = False
        fallback = sizes._loss_and_grads(net, batch)
    finally:
        layers.USE_HIP_LSTM = old
    assert layers.rnn_wide_calls == dict(before, saved=before["saved"] + 5)
    _lib.raise_if_nonfinite()
    ref = sizes._float64_loss_and_grads(net, batch, dev)
    assert set(ref) == set(hip) == set(fallback) and len(ref) == 1 + 6 + 15 + 2
    for k, r in ref.items():
        scale = r.abs().max().item() or 1.0
        e_hip, e_fb = (hip[k] - r).abs().max().item() / scale, (fallback[k] - r).abs().max().item() / scale
        print("mLstm_flipflop 384 N %d %s: slabs %.3e, nn.LSTM %.3e, ratio %.3f" % (N, k, e_hip, e_fb, e_hip / _allowed(e_fb)))
        assert e_hip <= _allowed(e_fb), (k, e_hip, e_fb)

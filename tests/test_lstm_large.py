"""The LSTM recurrence at hidden size 512 (include/taiyaki_amd_lstm_large.h; csrc/lstm_kernels.hip built -DTK_LSTM_LARGE;
layers.LstmRecurrence with row = "large").

An instantiation is (512, 32, C), named by the library's own plan (tk_lab_lstm_large_geometry) and never only by shape:
C = 4 at N = 7 * 4 + 1 = 29 (eight groups, the last ragged), C = 8 at one column more than C = 4 admits (65 on 256 CUs).

The allowance is the project's own (tests/test_rnn_instantiations.py::_allowed): error over the tensor's largest entry
<= 2 x the nn.LSTM / MIOpen path's own error on the same inputs + 2e-6, both against float64.  The helpers, float64
references and that allowance are those of tests/test_rnn_instantiations.py, test_lstm_fwd_rows.py,
test_rnn_varlen_train.py and test_lstm_hip.py.

Every launch at the C ABI asserts return code 0 and status word 0 behind the synchronise; after a non-zero status this
module launches nothing more (the remaining tests fail at once)."""
import contextlib
import copy
import ctypes

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, layers
from tests import test_lstm_fwd_rows as rows, test_lstm_hip, test_lstm_sizes as sizes, test_rnn_instantiations as insts
from tests import test_rnn_varlen_train as vtrain
from tests.test_lstm_large_host import COLUMNS, H, MEMBERS, UNITS, bound, rule

_cus = rows._cus
_allowed = insts._allowed
_stopped = []           # the first non-zero status word or return code of this module's own launches
POISON = 0xA5           # what the workspace holds in front of a call: every granule's tag is then 0xA5A5A5A5


@pytest.fixture(autouse=True)
def _nothing_after_a_bad_status():
    if _stopped:
        pytest.fail("not run: an earlier launch of this module ended with %s" % (_stopped[0],))


def _finish(rc, status, what):
    """Return code 0, and the status word 0 behind the synchronise."""
    if rc != 0:
        _stopped.append((what, "rc", rc))
    _lib.check(rc, what)
    torch.cuda.synchronize()
    word = int(status.item())
    if word != 0:
        _stopped.append((what, "status", word))
    assert word == 0, (what, word)


def _inst(n, dev, forced=0):
    """(H, U, C) of the launch at n columns on this device, from the library's own plan."""
    L = _lib.use_lab(True) and _lib.lstm_large_lib()
    try:
        L.tk_lab_lstm_large_cols(forced)
        out = (ctypes.c_size_t * 8)()
        if not L.tk_lab_lstm_large_geometry(n, H, _cus(dev), out):
            return None
        assert out[5] <= _cus(dev)
        return (H, int(out[2]), int(out[3]))
    finally:
        L.tk_lab_lstm_large_cols(0)
        _lib.use_lab(False)


def _batch(c, dev):
    """The batch that names (512, 32, c) on this device: 7 c + 1 at the first column count, one column more than the
    count before admits at a later one; eight or more groups, the last ragged."""
    cus = _cus(dev)
    if cus < 8 * MEMBERS:
        pytest.skip("fewer than eight groups of %d workgroups fit %d CUs" % (MEMBERS, cus))
    i = COLUMNS.index(c)
    n = 7 * c + 1 if i == 0 else bound(cus, COLUMNS[:i]) + 1
    assert rule(n, cus) == (c, -(-n // c)) and _inst(n, dev) == (H, UNITS, c), (n, c, cus)
    return n


@contextlib.contextmanager
def _forced(c):
    """The lab build with the columns per group forced to c (0: the release library, nothing forced)."""
    if not c:
        yield
        return
    L = _lib.use_lab(True) and _lib.lstm_large_lib()
    try:
        L.tk_lab_lstm_large_cols(c)
        yield
    finally:
        L.tk_lab_lstm_large_cols(0)
        _lib.use_lab(False)


def _buffers(shapes, dev):
    return {k: rows._guarded(s, dev, 0) for k, s in shapes.items()}


def _checked(bufs, what):
    """Nothing outside and nothing unwritten; -> the tensors."""
    out = {}
    for k, (flat, body) in bufs.items():
        assert rows._guards_intact(flat, 0, body.numel()), (what, k, "a store outside the tensor")
        unwritten = int((body == rows.SENTINEL).sum().item())
        assert unwritten == 0, (what, k, "elements not stored", unwritten)
        assert bool(torch.isfinite(body).all()), (what, k)
        out[k] = body
    return out


def _run(gx, whh, dy, lens, rev, save=True):
    """The forward (save: and the backward) through the C entries into guarded, sentinel-filled buffers, the workspace
    poisoned in front of either call -> dict of y (, gates, cell, dgates).  lens: a list, a device int32 tensor or None."""
    L = _lib.lstm_large_lib()
    T, N, _ = gx.shape
    dev, cus = gx.device, _cus(gx.device)
    gx = gx.contiguous()
    if lens is not None and not torch.is_tensor(lens):
        lens = torch.tensor(lens, dtype=torch.int32, device=dev)
    wsb = L.tk_lstm_large_workspace_bytes(N, H, cus)
    assert wsb > 0
    shapes = {"y": (T, N, H)}
    if save:
        shapes.update(gates=(T, N, 4 * H), cell=(T, N, H))
    bufs = _buffers(shapes, dev)
    P = _lib.ptr
    ws = torch.full((wsb,), POISON, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.tk_lstm_large_forward_dev(P(gx), P(whh), P(lens), T, N, H, rev, cus, P(bufs["y"][1]),
                                     P(bufs["gates"][1] if save else None), P(bufs["cell"][1] if save else None),
                                     P(ws), wsb, P(status), _lib.stream_ptr())
    _finish(rc, status, "tk_lstm_large_forward_dev")
    out = _checked(bufs, "forward")
    if save:
        dbuf = _buffers({"dgates": (T, N, 4 * H)}, dev)
        ws.fill_(POISON)
        rc = L.tk_lstm_large_backward_dev(P(whh), P(out["gates"]), P(out["cell"]), P(dy.contiguous()), P(lens), T, N, H,
                                          rev, cus, P(dbuf["dgates"][1]), P(ws), wsb, P(status), _lib.stream_ptr())
        _finish(rc, status, "tk_lstm_large_backward_dev")
        out.update(_checked(dbuf, "backward"))
    return out


def _equal(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, (a[k] - b[k]).abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------
# the instantiations at the C ABI: y, gates, cell and dgates against float64, inside their bounds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", insts.STEPS)
@pytest.mark.parametrize("c", COLUMNS)
def test_saved_tensors_and_dgates_match_float64_inside_their_bounds(gpu_device, c, T, rev):
    dev = gpu_device
    n = _batch(c, dev)
    rnn, x, ref, gx, w_hh = rows._inputs(H, n, T, dev)
    dy = insts._dy(H, n, T).to(dev)
    got = _run(gx, w_hh, dy, None, rev)
    e_mio = rows._rel(rows._miopen_y(rnn, x, rev, dev), ref[rev][0])
    for name, r in zip(("y", "gates", "cell"), ref[rev]):
        e = rows._rel(got[name], r)
        print("large fwd C %d N %d T %d rev %d %s: error %.3e, MIOpen's y %.3e, ratio %.3f"
              % (c, n, T, rev, name, e, e_mio, e / _allowed(e_mio)))
        assert e <= _allowed(e_mio), (c, n, T, rev, name, e, e_mio)
    dref = insts._dgates64(H, n, T, gx, w_hh)[rev]
    assert dref.abs().max().item() > 0
    e, e_mio = rows._rel(got["dgates"], dref), rows._rel(insts._miopen_dgates(gx, w_hh, dy, rev), dref)
    print("large bwd C %d N %d T %d rev %d dgates: error %.3e, MIOpen's %.3e, ratio %.3f"
          % (c, n, T, rev, e, e_mio, e / _allowed(e_mio)))
    assert e <= _allowed(e_mio), (c, n, T, rev, e, e_mio)


# ---------------------------------------------------------------------------------------------------------------------
# the layer against float64
# ---------------------------------------------------------------------------------------------------------------------
class _nn_lstm:
    """USE_HIP_LSTM_LARGE = False inside: nn.LSTM on the same device."""

    def __enter__(self):
        self.old, layers.USE_HIP_LSTM_LARGE = layers.USE_HIP_LSTM_LARGE, False

    def __exit__(self, *exc):
        layers.USE_HIP_LSTM_LARGE = self.old


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T", [1, 2, 37])
@pytest.mark.parametrize("I", [7, 512])
def test_layer_matches_float64(gpu_device, I, T, reverse):
    """y, dx, dW_ih, dW_hh and db of one layer, tests/test_lstm_hip.py::_compare written on its _grads (that function
    asserts the old query, which answers 0 here).  T = 1: the epilogue alone; T = 2: one hand-off; T = 37: the step
    parity turns over many times.  N = 5: two groups, the second ragged."""
    dev, N = gpu_device, 5
    torch.manual_seed(T + I)
    lstm = layers.Lstm(I, H)
    layer = layers.Reverse(lstm) if reverse else lstm
    x = torch.randn(T, N, I)
    dy = torch.randn(T, N, H) / (T * N) ** 0.5
    ref = test_lstm_hip._grads(layer.double(), x.double(), dy.double())
    layer = layer.float().to(dev)
    xd = x.to(dev)
    assert layers.hip_lstm_workspace_bytes(lstm.rnn, xd) == 0 and layers.hip_rnn_wide_workspace_bytes(lstm.rnn, xd) == 0
    assert layers.hip_lstm_large_workspace_bytes(lstm.rnn, xd) == 2 * 2 * 16 * 4 * 512 * 8
    before = dict(layers.lstm_large_calls)
    hip = test_lstm_hip._grads(layer, xd, dy.to(dev))
    assert layers.lstm_large_calls == {"saved": before["saved"] + 1, "inference": before["inference"]}
    with _nn_lstm():
        assert layers.hip_lstm_large_workspace_bytes(lstm.rnn, xd) == 0
        miopen = test_lstm_hip._grads(layer, xd, dy.to(dev))
    assert layers.lstm_large_calls["saved"] == before["saved"] + 1, "the switch"
    _lib.raise_if_nonfinite()
    for k, r in ref.items():
        e_hip, e_mio = rows._rel(hip[k], r), rows._rel(miopen[k], r)
        print("layer I %d T %d rev %d %s: HIP %.3e, nn.LSTM %.3e, ratio %.3f"
              % (I, T, reverse, k, e_hip, e_mio, e_hip / _allowed(e_mio)))
        assert e_hip <= _allowed(e_mio), (I, T, reverse, k, e_hip, e_mio)
    # under no_grad nothing is saved, and y is the same bits
    with torch.no_grad():
        assert torch.equal(layer(xd), hip["y"])
    assert layers.lstm_large_calls == {"saved": before["saved"] + 1, "inference": before["inference"] + 1}


# ---------------------------------------------------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", insts.STEPS)
@pytest.mark.parametrize("c", COLUMNS)
def test_lengths_match_the_masked_float64_recurrence(gpu_device, c, T, rev):
    """lengths_for(N, T) has 0, 1, T - 1 and T among its values.  y against the masked float64 recurrence; exact zeros at
    and beyond every length in y, gates, cell and dgates; NaN in gx and dy beyond the lengths changes nothing; sampled
    columns are, bit for bit, the column run alone over its own length at the same (U, C)."""
    dev = gpu_device
    n = _batch(c, dev)
    rnn, x, ref, gx, w_hh = rows._inputs(H, n, T, dev)
    dy = insts._dy(H, n, T).to(dev)
    lens_host = insts.lengths_for(n, T)
    assert {0, 1, T - 1, T} <= set(lens_host)
    lens = torch.tensor(lens_host, dtype=torch.int32, device=dev)
    got = _run(gx, w_hh, dy, lens, rev)
    beyond = torch.arange(T, device=dev)[:, None] >= lens[None, :]
    assert int(beyond.sum().item()) > 0
    for k, v in got.items():
        assert bool((v[beyond] == 0).all()), (k, "rows at and beyond the length are not exactly 0")
    e_mio = rows._rel(rows._miopen_y(rnn, x, rev, dev), ref[rev][0])
    e = rows._rel(got["y"], insts._lstm_masked64(H, n, T)[rev])
    print("large VL C %d N %d T %d rev %d y: error %.3e, MIOpen's y %.3e, ratio %.3f"
          % (c, n, T, rev, e, e_mio, e / _allowed(e_mio)))
    assert e <= _allowed(e_mio), (c, n, T, rev, e, e_mio)
    # what gx and dy hold beyond the lengths is never used
    gxp, dyp = gx.clone(), dy.clone()
    gxp[beyond], dyp[beyond] = float("nan"), float("nan")
    assert bool(torch.isnan(gxp).any()) and bool(torch.isnan(dyp).any())
    _equal(_run(gxp, w_hh, dyp, lens, rev), got, "NaN beyond the lengths")
    assert torch.equal(_run(gxp, w_hh, dyp, lens, rev, save=False)["y"], got["y"]), "nothing saved"
    # sampled columns alone, at the batch's own column count (one column alone takes the first count by the rule)
    cols = vtrain._sample(n)
    assert {lens_host[i] for i in cols} == set(lens_host)
    force = 0 if c == COLUMNS[0] else c
    assert _inst(1, dev, force) == (H, UNITS, c)
    with _forced(force):
        for i in cols:
            ln = lens_host[i]
            if ln:
                alone = _run(gx[:ln, i:i + 1], w_hh, dy[:ln, i:i + 1], None, rev)
                for k, v in alone.items():
                    assert torch.equal(v[:, 0], got[k][:ln, i]), (k, i, ln)


# ---------------------------------------------------------------------------------------------------------------------
# bitwise identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("c", COLUMNS)
def test_bitwise_identities(gpu_device, c, rev):
    """lengths = NULL and lengths = [T] * N; y with and without the saves; two launches."""
    dev, T = gpu_device, 7
    n = _batch(c, dev)
    gx, whh, _, dy = vtrain._abi_case("lstm", H, n, T, dev, 900 + c + rev)
    a = _run(gx, whh, dy, None, rev)
    assert a["y"].abs().max().item() > 0.1 and a["dgates"].abs().max().item() > 1e-4
    _equal(_run(gx, whh, dy, None, rev), a, "two launches")
    _equal(_run(gx, whh, dy, [T] * n, rev), a, "lengths = [T] * N")
    assert torch.equal(_run(gx, whh, dy, None, rev, save=False)["y"], a["y"]), "nothing saved, lengths NULL"
    assert torch.equal(_run(gx, whh, dy, [T] * n, rev, save=False)["y"], a["y"]), "nothing saved, lengths [T] * N"


# ---------------------------------------------------------------------------------------------------------------------
# slabs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("with_lengths", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("extra", ["bound+1", "2bound+3"])
def test_slab_rows_are_the_call_on_a_copy_of_its_columns(gpu_device, extra, with_lengths, rev):
    """A batch wider than one launch admits, saved and not: slab k's rows are bit for bit what the call writes on a
    copy of slab k's columns alone.  The workspace holds a poison pattern in front of every call (`_run`)."""
    dev, T = gpu_device, 3
    cus = _cus(dev)
    S = bound(cus)
    n = S + 1 if extra == "bound+1" else 2 * S + 3
    L = _lib.lstm_large_lib()
    assert S > 0 and L.tk_lstm_large_slab(n, H, cus) == S and _inst(n, dev) is None
    gx, whh, _, dy = vtrain._abi_case("lstm", H, n, T, dev, 950 + rev)
    lens = insts.lengths_for(n, T) if with_lengths else None
    got = _run(gx, whh, dy, lens, rev)
    y_only = _run(gx, whh, dy, lens, rev, save=False)["y"]
    assert torch.equal(y_only, got["y"]), "nothing saved"
    for first in range(0, n, S):
        last = min(first + S, n)
        sl = None if lens is None else lens[first:last]
        part = _run(gx[:, first:last].contiguous(), whh, dy[:, first:last].contiguous(), sl, rev)
        for k, v in part.items():
            assert torch.equal(v, got[k][:, first:last]), (k, first, last)


# ---------------------------------------------------------------------------------------------------------------------
# a captured forward, the model, the basecaller
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_forward_replays_bit_identical(gpu_device):
    """tests/test_lstm_hip.py's captured forward at size 512: a single stream, three replays."""
    torch.manual_seed(7)
    layer = layers.Serial([layers.Reverse(layers.Lstm(32, H)), layers.Lstm(H, H)]).to(gpu_device)
    x = torch.randn(30, 21, 32, device=gpu_device)
    before = layers.lstm_large_calls["inference"]
    strict = _lib.is_strict()
    _lib.set_strict(False)              # (the status word is read by raise_if_nonfinite, not inside the capture)
    try:
        with torch.no_grad():
            eager = layer(x)
            assert layers.lstm_large_calls["inference"] == before + 2
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                layer(x)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = layer(x)
            for _ in range(3):
                out.fill_(float("nan"))
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager)
        _lib.raise_if_nonfinite()
    finally:
        _lib.set_strict(strict)


@pytest.mark.gpu
def test_model_loss_and_gradients_match_the_fallback(gpu_device):
    """models.mLstm_flipflop(size=512) at chunk_len 200 (T = 40), N = 5, one calculate_loss + backward, by the procedure
    of tests/test_lstm_sizes.py: all five layers run the new path, and the loss and every parameter gradient are as
    close to the float64 model as 2 x the USE_HIP_LSTM_LARGE = False run's own error + 2e-6."""
    from taiyaki_amd import models
    dev = gpu_device
    torch.manual_seed(H)
    net = models.mLstm_flipflop(size=H, stride=5).to(dev)
    batch = sizes._model_batch("flipflop", 200, 5, dev)
    lstms = [m for m in net.modules() if isinstance(m, layers.Lstm)]
    probe = torch.zeros(40, 5, H, device=dev)
    assert len(lstms) == 5 and all(layers.hip_lstm_large_workspace_bytes(m.rnn, probe) > 0 for m in lstms)
    before = dict(layers.lstm_large_calls)
    hip = sizes._loss_and_grads(net, batch)
    assert layers.lstm_large_calls == {"saved": before["saved"] + 5, "inference": before["inference"]}
    with _nn_lstm():
        assert all(layers.hip_lstm_large_workspace_bytes(m.rnn, probe) == 0 for m in lstms)
        fallback = sizes._loss_and_grads(net, batch)
    assert layers.lstm_large_calls["saved"] == before["saved"] + 5, "the switch"
    _lib.raise_if_nonfinite()
    ref = sizes._float64_loss_and_grads(net, batch, dev)
    assert set(ref) == set(hip) == set(fallback) and len(ref) == 1 + 6 + 15 + 2
    for k, r in ref.items():
        scale = r.abs().max().item() or 1.0
        e_hip, e_fb = (hip[k] - r).abs().max().item() / scale, (fallback[k] - r).abs().max().item() / scale
        print("mLstm_flipflop 512 %s: HIP %.3e, nn.LSTM %.3e, ratio %.3f" % (k, e_hip, e_fb, e_hip / _allowed(e_fb)))
        assert e_hip <= _allowed(e_fb), (k, e_hip, e_fb)


@pytest.mark.gpu
def test_basecaller_short_reads_call_the_same_sequences_as_the_fallback(gpu_device):
    """Basecaller(batch_short=True) on three reads shorter than a chunk, at size 512: the same sequences from the new
    path (variable-length columns, nothing saved) and from nn.LSTM, as tests/test_lstm_sizes.py asks at size 192."""
    from taiyaki_amd import basecall, models, synth
    torch.manual_seed(15)
    net = synth.excite_network(models.mLstm_flipflop(size=H, stride=5)).to(gpu_device).eval()
    rs = np.random.RandomState(4)
    sigs = [(90 + 12 * rs.standard_normal(n) + 3 * np.sin(np.arange(n) / 50.0)).astype(np.float32) for n in (400, 333, 777)]
    before = dict(layers.lstm_large_calls)
    calls = basecall.Basecaller(net, stride=5, chunk_size=200, overlap=20, batch_short=True).call(sigs)
    assert layers.lstm_large_calls["inference"] > before["inference"], "the short reads did not take the new path"
    assert layers.lstm_large_calls["saved"] == before["saved"]
    after = dict(layers.lstm_large_calls)
    with _nn_lstm():
        fallback = basecall.Basecaller(net, stride=5, chunk_size=200, overlap=20, batch_short=True).call(sigs)
    assert layers.lstm_large_calls == after, "the switch"
    _lib.raise_if_nonfinite()
    assert [c[2] for c in calls] == [400, 333, 777] and all(len(c[0]) > 0 and set(c[0]) <= set("ACGT") for c in calls)
    assert [c[0] for c in calls] == [c[0] for c in fallback]

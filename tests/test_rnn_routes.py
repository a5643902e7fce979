"""Which kernel library runs the recurrence of an `Lstm` or a `GruMod`: layers._rnn_route, the one place that decides,
on the host alone.  The six queries are stubs that admit a call or not in every combination; the seam behind the route
(layers._rnn_apply) records what would be launched and launches nothing.  The order that must hold:

Lstm, no lengths: the main library -> (False, save True always); slabs of columns, asked only on a 3-d tensor with
  steps and columns -> ("wide", True always); size 96 -> ("local", needs); size 512 -> ("large", needs); else nn.LSTM,
  flipped for `reverse`.
GruMod, no lengths: the main library -> (False, needs); slabs, under the same guard -> ("wide", needs); else nn.GRU,
  flipped for `reverse`.
Either, with lengths: raise if needs and not TRAIN_VARLEN, before any query.  On a tensor with steps and columns the
  training pair if needs, else the inference launch -> (True, needs); then slabs -> ("wide", needs); the LSTM only:
  size 96 -> ("local", needs), then size 512 -> ("large", needs); else every column alone, at its own length.
needs: grad mode is on and x or a parameter of the layer requires a gradient.
"""
import contextlib
import itertools

import pytest
import torch

from taiyaki_amd import _lib, layers

# the stubs' answers: a workspace size by which a record shows which query admitted (the local query answers True)
ANSWERS = {"hip_lstm_workspace_bytes": 11, "hip_gru_workspace_bytes": 11, "hip_rnn_varlen_workspace_bytes": 12,
           "hip_rnn_varlen_train_workspace_bytes": 13, "hip_rnn_wide_workspace_bytes": 14, "hip_lstm_local_takes": True,
           "hip_lstm_large_workspace_bytes": 16}
SHAPES = ((5, 3, 12), (0, 3, 12), (5, 0, 12))
SIZE = 12           # the hidden size is the input's, so the stand-in for nn.LSTM / nn.GRU below can hand back 2 x


class _Seam:
    """The stubs and what they saw on the batch itself (a column run alone, one column wide, is never admitted)."""

    def __init__(self, monkeypatch):
        self.admit, self.asked, self.applied, self.cell_inputs = set(), [], [], []
        self.launched = object()
        for name in ANSWERS:
            monkeypatch.setattr(layers, name, self._query(name))
        monkeypatch.setattr(layers, "_rnn_apply", self._apply)
        # the tensors are on the CPU: there is no device to make current around the launch with lengths
        monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)

    def _query(self, name):
        def query(rnn, x):
            if x.dim() == 3 and x.shape[1] == 1:
                return 0
            self.asked.append(name)
            return ANSWERS[name] if name in self.admit else 0
        return query

    def _apply(self, layer, x, reverse, row, wsb, lens, save):
        if lens is not None:
            assert lens.dtype == torch.int32 and lens.device == x.device and lens.is_contiguous()
            lens = lens.tolist()
        self.applied.append((type(layer.rnn), row, wsb, lens, save, reverse))
        return self.launched

    def cell(self, inp):
        self.cell_inputs.append(inp)
        return 2 * inp, None


def _candidates(lstm, lengths_given, needs, full):
    """The order of the module's docstring: (query, asked at all, row, save)."""
    if not lengths_given:
        rows = [("hip_lstm_workspace_bytes" if lstm else "hip_gru_workspace_bytes", True, False, lstm or needs),
                ("hip_rnn_wide_workspace_bytes", full, "wide", lstm or needs)]
    else:
        rows = [("hip_rnn_varlen_train_workspace_bytes" if needs else "hip_rnn_varlen_workspace_bytes", full, True, needs),
                ("hip_rnn_wide_workspace_bytes", full, "wide", needs)]
    if lstm:
        rows += [("hip_lstm_local_takes", True, "local", needs), ("hip_lstm_large_workspace_bytes", True, "large", needs)]
    return rows


@pytest.mark.parametrize("lengths_given", (False, True))
@pytest.mark.parametrize("cls", (layers.Lstm, layers.GruMod))
def test_every_line_of_the_order(monkeypatch, cls, lengths_given):
    seam = _Seam(monkeypatch)
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    lstm = cls is layers.Lstm
    kinds = ("first", "hip_rnn_wide_workspace_bytes", "hip_lstm_local_takes", "hip_lstm_large_workspace_bytes")
    firsts = {"hip_lstm_workspace_bytes", "hip_gru_workspace_bytes", "hip_rnn_varlen_workspace_bytes",
              "hip_rnn_varlen_train_workspace_bytes"}
    ncases = 0
    for shape, x_grad, frozen, no_grad, reverse in itertools.product(SHAPES, *[(False, True)] * 4):
        T, N, _ = shape
        torch.manual_seed(3)
        layer = cls(12, SIZE).requires_grad_(not frozen)
        monkeypatch.setattr(layer.rnn, "forward", seam.cell)
        x = torch.randn(*shape, requires_grad=x_grad)
        needs = not no_grad and (x_grad or not frozen)
        lengths = [T, min(T, 3), 0][:N] if lengths_given else None
        want = _candidates(lstm, lengths_given, needs, bool(T and N))
        for picked in itertools.product((False, True), repeat=len(kinds)):
            seam.admit = set().union(*[firsts if k == "first" else {k} for k, p in zip(kinds, picked) if p])
            seam.asked, seam.applied, seam.cell_inputs = [], [], []
            with torch.no_grad() if no_grad else contextlib.nullcontext():
                y = (layers.Reverse(layer) if reverse else layer)(x, **({"lengths": lengths} if lengths_given else {}))
            hit = [i for i, (query, asked, _, _) in enumerate(want) if asked and query in seam.admit]
            upto = want[:hit[0] + 1] if hit else want
            # the same queries in the same order, none behind the first that admitted, none on an empty tensor
            assert seam.asked == [query for query, asked, _, _ in upto if asked], (shape, needs, picked)
            ncases += 1
            if hit:
                query, _, row, save = want[hit[0]]
                wsb = 0 if row == "local" else ANSWERS[query]
                assert y is seam.launched and not seam.cell_inputs
                assert seam.applied == [(type(layer.rnn), row, wsb, lengths, save, reverse)], (shape, needs, picked)
            elif not lengths_given:     # nn.LSTM / nn.GRU, flipped for `reverse`
                assert not seam.applied and len(seam.cell_inputs) == 1
                assert torch.equal(seam.cell_inputs[0], torch.flip(x, (0,)) if reverse else x) and torch.equal(y, 2 * x)
            else:                       # every column alone, at its own length
                assert not seam.applied
                assert [tuple(c.shape) for c in seam.cell_inputs] == [(ln, 1, 12) for ln in lengths if ln]
                for n, ln in enumerate(lengths):
                    assert torch.equal(y[:ln, n], 2 * x[:ln, n]) and not y[ln:, n].any()
    assert ncases == len(SHAPES) * 16 * 16


@pytest.mark.parametrize("cls", (layers.Lstm, layers.GruMod))
def test_the_lstm_alone_saves_whatever_the_grad_mode_on_its_main_and_wide_rows(monkeypatch, cls):
    seam = _Seam(monkeypatch)
    layer, x = cls(12, SIZE), torch.randn(5, 3, 12)
    for query, row in ((("hip_lstm_workspace_bytes", "hip_gru_workspace_bytes"), False),
                       (("hip_rnn_wide_workspace_bytes",), "wide")):
        seam.admit, seam.applied = set(query), []
        with torch.no_grad():
            layer(x)
        assert [(a[1], a[4]) for a in seam.applied] == [(row, cls is layers.Lstm)]
    for query, row in (("hip_lstm_local_takes", "local"), ("hip_lstm_large_workspace_bytes", "large")):
        seam.admit, seam.applied = {query}, []
        with torch.no_grad():
            layer(x)
        layer(x)
        assert [(a[1], a[4]) for a in seam.applied] == ([(row, False), (row, True)] if cls is layers.Lstm else [])


@pytest.mark.parametrize("cls", (layers.Lstm, layers.GruMod))
def test_the_train_varlen_error_precedes_every_query(monkeypatch, cls):
    seam = _Seam(monkeypatch)
    assert layers.TRAIN_VARLEN is False
    seam.admit = set(ANSWERS)
    layer = cls(12, SIZE)
    for shape in SHAPES:
        x = torch.randn(*shape)
        with pytest.raises(RuntimeError, match="TRAIN_VARLEN"):
            layer(x, lengths=[0] * shape[1])
        with pytest.raises(RuntimeError, match="TRAIN_VARLEN"):
            layers.Reverse(layer.requires_grad_(False))(x.clone().requires_grad_(), lengths=[0] * shape[1])
        layer.requires_grad_(True)
        assert not seam.asked and not seam.applied
    with torch.no_grad():
        assert layer(torch.randn(5, 3, 12), lengths=[5, 3, 0]) is seam.launched
    assert seam.asked == ["hip_rnn_varlen_workspace_bytes"]


SIGNATURES = {"lib": _lib.SIGNATURES, "varlen_lib": _lib.VARLEN_SIGNATURES, "varlen_train_lib": _lib.VARLEN_TRAIN_SIGNATURES,
              "rnn_wide_lib": _lib.WIDE_SIGNATURES, "lstm_large_lib": _lib.LSTM_LARGE_SIGNATURES,
              "lstm_local_lib": _lib.LSTM_LOCAL_SIGNATURES}


def test_the_table_of_launches_has_these_rows_and_every_entry_is_declared():
    assert set(layers._RNN_LAUNCHES) == {(row, save) for row in (False, True, "wide", "large", "local")
                                         for save in (True, False)}
    for (row, save), (libname, fwd, bwd, tag) in layers._RNN_LAUNCHES.items():
        assert (bwd is not None) == save, (row, save)
        for cell in ("lstm",) if row in ("large", "local") else ("lstm", "gru"):
            for name in (fwd, bwd) if save else (fwd,):
                assert name % cell in SIGNATURES[libname], (row, save, cell)
    # the LSTM has no launch without lengths that saves nothing: that key is the GRU's alone
    with pytest.raises(RuntimeError, match="saves nothing"):
        layers.LstmRecurrence.apply(torch.zeros(5, 3, 12), *layers.Lstm(12, SIZE).rnn.parameters(), False, False, 11, None,
                                    False)
    # the bare rows' entries: the arguments of the wide ones less the workspace, its size and the status word
    assert layers._RNN_BARE_ROWS == {"local"}
    for local, wide in (("tk_lstm_local_forward_dev", "tk_lstm_forward_wide_dev"),
                        ("tk_lstm_local_backward_dev", "tk_lstm_backward_wide_dev")):
        args, wide_args = _lib.LSTM_LOCAL_SIGNATURES[local][1], _lib.WIDE_SIGNATURES[wide][1]
        assert args == wide_args[:-4] + wide_args[-1:]
    # every row but the main one has a counter of its own
    assert set(layers._RNN_CALLS) == {True, "wide", "local", "large"}
    assert all(layers._RNN_CALLS[row] is getattr(layers, name) for row, name in (
        (True, "rnn_varlen_calls"), ("wide", "rnn_wide_calls"), ("local", "lstm_local_calls"), ("large", "lstm_large_calls")))

"""include/taiyaki_amd_lstm_matrix.h on the host: the header, the library and the binding, the two queries, the argument
checks in front of a launch, and what the route never does with the row."""
import ctypes
import os
import subprocess

import pytest
import torch

from taiyaki_amd import _lib, layers

ENTRIES = {"tk_lstm_matrix_supported", "tk_lstm_matrix_columns", "tk_lstm_matrix_forward_dev"}


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.LSTM_MATRIX_SIGNATURES) == ENTRIES
    for libname in (_lib.LSTM_MATRIX_LIBNAME, _lib.LSTM_MATRIX_LAB_LIBNAME):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                             capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if line.strip()} == ENTRIES, libname
    sz, i, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    assert _lib.LSTM_MATRIX_SIGNATURES["tk_lstm_matrix_forward_dev"] == (i, [vp, vp, vp, sz, sz, sz, i, vp, vp])
    # the arguments of the local forward less the CU count and the two saved tensors
    local = _lib.LSTM_LOCAL_SIGNATURES["tk_lstm_local_forward_dev"][1]
    assert _lib.LSTM_MATRIX_SIGNATURES["tk_lstm_matrix_forward_dev"][1] == local[:7] + local[8:9] + local[11:]
    L = _lib.lstm_matrix_lib()                          # resolves every symbol
    try:
        assert _lib.use_lab(True) and _lib.lstm_matrix_lib() is not L
    finally:
        _lib.use_lab(False)
    assert _lib.lstm_matrix_lib() is L


def test_supported_sizes_and_columns():
    L = _lib.lstm_matrix_lib()
    assert L.tk_lstm_matrix_supported(96) == 1 and L.tk_lstm_matrix_columns(96) == 16
    for h in (0, 16, 48, 64, 95, 97, 128, 192, 256, 384, 512):
        assert L.tk_lstm_matrix_supported(h) == 0 and L.tk_lstm_matrix_columns(h) == 0, h


def test_the_entry_checks_its_arguments_before_anything_is_launched():
    fwd = _lib.lstm_matrix_lib().tk_lstm_matrix_forward_dev
    bad, unsupported = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED"))
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    # a required pointer NULL or misaligned (w_hh needs a float's alignment), in front of the size
    assert fwd(None, p, None, 4, 3, 96, 0, p, None) == bad
    assert fwd(p, None, None, 4, 3, 96, 0, p, None) == bad
    assert fwd(p, p, None, 4, 3, 256, 0, None, None) == bad
    assert fwd(odd, p, None, 4, 3, 256, 0, p, None) == bad
    assert fwd(p, p, None, 4, 0, 96, 0, odd, None) == bad
    # nblk or nbatch beyond int32, in front of the size
    assert fwd(p, p, None, 1 << 31, 3, 256, 0, p, None) == bad
    assert fwd(p, p, None, 4, 1 << 31, 256, 0, p, None) == bad
    # a size the kernel does not cover, no batch: behind the pointer checks, in front of nblk = 0
    assert fwd(p, p, None, 4, 3, 256, 0, p, None) == unsupported
    assert fwd(p, p, None, 0, 3, 95, 0, p, None) == unsupported
    assert fwd(p, p, None, 0, 0, 96, 0, p, None) == unsupported
    # nothing to do at nblk = 0, behind the checks
    assert fwd(p, p, None, 0, 3, 96, 0, p, None) == 0
    assert fwd(p, p, p, 0, 5000, 96, 1, p, None) == 0


@pytest.mark.parametrize("lengths_given", (False, True))
def test_the_route_never_takes_the_row_to_save_or_below_the_threshold(monkeypatch, lengths_given):
    """Every query in front of the row refuses and the layer's own admission is granted, so the row's three conditions
    alone decide: the switch, `save`, the width."""
    assert layers.LSTM_MATRIX_MIN_COLUMNS >= 2 * 256 + 1        # two columns per CU of an MI355X: one round of the local kernel
    assert layers.lstm_matrix_calls.keys() == {"inference"}
    monkeypatch.setattr(layers, "_hip_lstm_takes", lambda rnn, x: True)
    for name in ("hip_lstm_workspace_bytes", "hip_rnn_varlen_workspace_bytes", "hip_rnn_varlen_train_workspace_bytes",
                 "hip_rnn_wide_workspace_bytes"):
        monkeypatch.setattr(layers, name, lambda rnn, x: 0)
    layer, gru = layers.Lstm(4, 96), layers.GruMod(4, 96)
    at = layers.LSTM_MATRIX_MIN_COLUMNS
    for n, save, on, want in ((at, False, True, "matrix"), (at + 5000, False, True, "matrix"), (at, True, True, "local"),
                              (at - 1, False, True, "local"), (1, False, True, "local"), (at, False, False, "local")):
        monkeypatch.setattr(layers, "USE_HIP_LSTM_MATRIX", on)
        x = torch.empty(2, n, 4)
        assert layers._rnn_route(layer, x, lengths_given, save) == (want, 0), (n, save, on)
        assert layers._rnn_route(gru, x, lengths_given, save) is None
    monkeypatch.setattr(layers, "USE_HIP_LSTM_MATRIX", True)
    assert layers._rnn_route(layers.Lstm(4, 256), torch.empty(2, at, 4), lengths_given, False) is None
    assert layers._rnn_route(layer, torch.empty(0, at, 4), lengths_given, False) is None
    assert ("matrix", True) not in layers._RNN_MATRIX_LAUNCHES and ("matrix", True) not in layers._RNN_LAUNCHES

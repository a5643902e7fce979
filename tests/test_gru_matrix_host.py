"""include/taiyaki_amd_gru_matrix.h on the host: the header, the library and the binding, the two queries, the argument
checks in front of a launch, and when the route takes the row."""
import ctypes
import os
import subprocess

import pytest
import torch

from taiyaki_amd import _lib, layers

ENTRIES = {"tk_gru_matrix_supported", "tk_gru_matrix_columns", "tk_gru_matrix_forward_dev"}


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.GRU_MATRIX_SIGNATURES) == ENTRIES
    for libname in (_lib.GRU_MATRIX_LIBNAME, _lib.GRU_MATRIX_LAB_LIBNAME):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                             capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if line.strip()} == ENTRIES, libname
    sz, i, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    assert _lib.GRU_MATRIX_SIGNATURES["tk_gru_matrix_forward_dev"] == (i, [vp, vp, vp, vp, sz, sz, sz, i, vp, vp])
    L = _lib.gru_matrix_lib()                           # resolves every symbol
    try:
        assert _lib.use_lab(True) and _lib.gru_matrix_lib() is not L
    finally:
        _lib.use_lab(False)
    assert _lib.gru_matrix_lib() is L


def test_supported_sizes_and_columns():
    L = _lib.gru_matrix_lib()
    for h in (0, 16, 48, 64, 95, 96, 97, 128, 192, 256, 384):
        assert (L.tk_gru_matrix_supported(h), L.tk_gru_matrix_columns(h)) == ((1, 16) if h == 96 else (0, 0)), h


def test_the_entry_checks_its_arguments_before_anything_is_launched():
    fwd = _lib.gru_matrix_lib().tk_gru_matrix_forward_dev
    bad, unsupported = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED"))
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    # a required pointer NULL or misaligned (w_hh and b_hh need a float's alignment), in front of the size
    for k in (0, 1, 2, 8):
        args = [p, p, p, None, 4, 3, 256, 0, p, None]
        args[k] = None
        assert fwd(*args) == bad, k
    assert fwd(odd, p, p, None, 4, 3, 256, 0, p, None) == bad
    assert fwd(p, p, p, None, 4, 0, 96, 0, odd, None) == bad
    assert fwd(p, odd, odd, None, 0, 3, 96, 0, p, None) == 0
    # nblk or nbatch beyond int32, in front of the size
    assert fwd(p, p, p, None, 1 << 31, 3, 256, 0, p, None) == bad
    assert fwd(p, p, p, None, 4, 1 << 31, 256, 0, p, None) == bad
    # a size the kernel does not cover, no batch: behind the pointer checks, in front of nblk = 0
    assert fwd(p, p, p, None, 4, 3, 256, 0, p, None) == unsupported
    assert fwd(p, p, p, None, 0, 3, 95, 0, p, None) == unsupported
    assert fwd(p, p, p, None, 0, 0, 96, 0, p, None) == unsupported
    # nothing to do at nblk = 0, behind the checks
    assert fwd(p, p, p, None, 0, 3, 96, 0, p, None) == 0
    assert fwd(p, p, p, p, 0, 5000, 96, 1, p, None) == 0


@pytest.mark.parametrize("lengths_given", (False, True))
def test_the_route_takes_the_row_only_to_save_nothing_from_the_threshold_on(monkeypatch, lengths_given):
    """The layer's own admission is granted, so the row's conditions alone decide: the switch, `save`, the width, the
    size, a tensor with steps.  What refuses it goes on to the main library (or the one with lengths), stubbed to say 7."""
    assert layers.GRU_MATRIX_MIN_COLUMNS >= 2 * 256 + 1         # two columns per CU of an MI355X: one round of the main kernel
    assert layers.gru_matrix_calls.keys() == {"inference"}
    assert layers._RNN_MATRIX_LAUNCHES["gru_matrix", False] == ("gru_matrix_lib", "tk_%s_matrix_forward_dev", None, None)
    assert not any(row == "gru_matrix" for row, _ in list(layers._RNN_LAUNCHES) + [(r, 0) for r in layers._RNN_CALLS])
    monkeypatch.setattr(layers, "_hip_gru_takes", lambda rnn, x: True)
    monkeypatch.setattr(layers, "_hip_lstm_takes", lambda rnn, x: True)
    monkeypatch.setattr(layers, "hip_lstm_matrix_group_workspace_bytes", lambda rnn, x, save: 0)
    monkeypatch.setattr(layers, "hip_rnn_wide_workspace_bytes", lambda rnn, x: 0)
    for name in ("hip_gru_workspace_bytes", "hip_lstm_workspace_bytes", "hip_rnn_varlen_workspace_bytes",
                 "hip_rnn_varlen_train_workspace_bytes"):
        monkeypatch.setattr(layers, name, lambda rnn, x: 7)
    gru = layers.GruMod(4, 96)
    at = layers.GRU_MATRIX_MIN_COLUMNS
    behind = (lengths_given, 7)
    for n, save, on, want in ((at, False, True, ("gru_matrix", 0)), (at + 5000, False, True, ("gru_matrix", 0)),
                              (at, True, True, behind), (at - 1, False, True, behind), (1, False, True, behind),
                              (at, False, False, behind)):
        monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX", on)
        assert layers._rnn_route(gru, torch.empty(2, n, 4), lengths_given, save) == want, (n, save, on)
    monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX", True)
    assert layers._rnn_route(gru, torch.empty(0, at, 4), lengths_given, False) != ("gru_matrix", 0)
    assert layers._rnn_route(layers.GruMod(4, 256), torch.empty(2, at, 4), lengths_given, False) == behind
    assert layers._rnn_route(layers.Lstm(4, 96), torch.empty(2, at, 4), lengths_given, False) == behind

"""include/taiyaki_amd_gru_matrix_group.h on the host: the header, the libraries and the binding, the four queries, the
argument checks in front of a launch, and when the route takes the row."""
import ctypes
import os
import subprocess

import pytest
import torch

from taiyaki_amd import _lib, layers

ENTRIES = {"tk_gru_matrix_group_" + n for n in ("supported", "columns", "slab", "workspace_bytes", "forward_dev")}
H = 256


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.GRU_MATRIX_GROUP_SIGNATURES) == ENTRIES
    for libname in (_lib.GRU_MATRIX_GROUP_LIBNAME, _lib.GRU_MATRIX_GROUP_LAB_LIBNAME):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                             capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if line.strip()} == ENTRIES, libname
    # the LSTM group entry's arguments with b_hh behind w_hh
    lstm = _lib.LSTM_MATRIX_GROUP_SIGNATURES["tk_lstm_matrix_group_forward_dev"][1]
    assert _lib.GRU_MATRIX_GROUP_SIGNATURES["tk_gru_matrix_group_forward_dev"] == (
        ctypes.c_int, lstm[:2] + [ctypes.c_void_p] + lstm[2:])
    L = _lib.gru_matrix_group_lib()                     # resolves every symbol
    try:
        assert _lib.use_lab(True) and _lib.gru_matrix_group_lib() is not L
    finally:
        _lib.use_lab(False)
    assert _lib.gru_matrix_group_lib() is L


def test_the_queries():
    L = _lib.gru_matrix_group_lib()
    C = L.tk_gru_matrix_group_columns(H)
    assert L.tk_gru_matrix_group_supported(H) == 1 and C > 0 and C % 16 == 0
    G = 256 // (L.tk_gru_matrix_group_slab(H, 256) // C)
    for h in (96, 128, 192, 384, 512):
        assert L.tk_gru_matrix_group_supported(h) == 0 and L.tk_gru_matrix_group_columns(h) == 0, h
        assert L.tk_gru_matrix_group_slab(h, 256) == 0 and L.tk_gru_matrix_group_workspace_bytes(2048, h, 256) == 0, h
    for cus in (0, 1, G - 1):
        assert L.tk_gru_matrix_group_slab(H, cus) == 0 and L.tk_gru_matrix_group_workspace_bytes(64, H, cus) == 0
    for cus in (G, 64, 256, 304):
        S = L.tk_gru_matrix_group_slab(H, cus)
        assert S == cus // G * C
        at = L.tk_gru_matrix_group_workspace_bytes(S, H, cus)
        # grows by the group up to one slab, the same from there on
        assert 0 < L.tk_gru_matrix_group_workspace_bytes(1, H, cus) <= at and at % 16 == 0
        assert L.tk_gru_matrix_group_workspace_bytes(1, H, cus) == L.tk_gru_matrix_group_workspace_bytes(C, H, cus)
        assert all(L.tk_gru_matrix_group_workspace_bytes(n, H, cus) == at for n in (S + 1, 2 * S + 3, 100 * S))
    assert L.tk_gru_matrix_group_workspace_bytes(0, H, 256) == 0


def test_the_entry_checks_its_arguments_before_anything_is_launched():
    L = _lib.gru_matrix_group_lib()
    fwd = L.tk_gru_matrix_group_forward_dev
    bad, unsupported, small = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED", "WORKSPACE"))
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    big = 1 << 30
    # a required pointer NULL (b_hh among them) or misaligned (w_hh and b_hh need a float's alignment), in front of the
    # size; then the workspace and the status word
    for k in (0, 1, 2, 9, 10, 12):
        args = [p, p, p, None, 4, 3, 96, 0, 256, p, p, big, p, None]
        args[k] = None
        assert fwd(*args) == bad, k
    # ... gx, y or the workspace misaligned, nblk or nbatch beyond int32, in front of the size
    for k, v in ((0, odd), (9, odd), (10, odd), (4, 1 << 31), (5, 1 << 31)):
        args = [p, p, p, None, 4, 3, 96, 0, 256, p, p, big, p, None]
        args[k] = v
        assert fwd(*args) == bad, k
    # a size the kernel does not cover, no batch, no launch that fits: behind the pointer checks, in front of nblk = 0
    assert fwd(p, p, p, None, 4, 3, 96, 0, 256, p, p, big, p, None) == unsupported
    assert fwd(p, p, p, None, 0, 3, 512, 0, 256, p, p, big, p, None) == unsupported
    assert fwd(p, p, p, None, 0, 0, H, 0, 256, p, p, big, p, None) == unsupported
    assert fwd(p, p, p, None, 0, 3, H, 0, 3, p, p, big, p, None) == unsupported
    # a workspace below the query's answer, in front of nblk = 0
    need = L.tk_gru_matrix_group_workspace_bytes(5000, H, 256)
    assert fwd(p, p, p, None, 0, 5000, H, 0, 256, p, p, need - 1, p, None) == small
    assert fwd(p, p, p, None, 0, 3, H, 0, 256, p, p, 0, p, None) == small
    # nothing to do at nblk = 0, behind the checks
    assert fwd(p, p, p, None, 0, 5000, H, 0, 256, p, p, need, p, None) == 0
    assert fwd(p, odd, odd, p, 0, 3, H, 1, 8, p, p, need, p, None) == 0


@pytest.mark.parametrize("lengths_given", (False, True))
def test_the_route_takes_the_row_only_to_save_nothing_from_the_threshold_on(monkeypatch, lengths_given):
    """The layer's own admission and a GPU tensor are granted (a stand-in for the tensor: nothing here touches a
    device), so the row's own conditions decide: the switch, `save`, the width, the size.  It stands in front of the main
    library, which admits here."""
    assert layers.GRU_MATRIX_GROUP_MIN_COLUMNS >= 2 * 256 + 1       # up to two slabs of the main library stay
    assert layers.gru_matrix_group_calls.keys() == {"inference"}
    assert layers._RNN_MATRIX_LAUNCHES["gru_matrix_group", False] == (
        "gru_matrix_group_lib", "tk_%s_matrix_group_forward_dev", None, "gru_matrix_group")
    assert "gru_matrix_group" not in layers._RNN_MATRIX_BARE_ROWS | layers._RNN_BARE_ROWS | set(layers._RNN_CALLS)
    monkeypatch.setattr(layers, "_hip_gru_takes", lambda rnn, x: True)
    monkeypatch.setattr(layers, "_cu_count", lambda dev: 256)
    for name in ("hip_lstm_workspace_bytes", "hip_gru_workspace_bytes", "hip_rnn_varlen_workspace_bytes",
                 "hip_rnn_varlen_train_workspace_bytes"):
        monkeypatch.setattr(layers, name, lambda rnn, x: 11)
    main = (lengths_given, 11)

    class OnGpu(torch.Tensor):
        is_cuda = True

    layer, lstm, small = layers.GruMod(4, H), layers.Lstm(4, H), layers.GruMod(4, 128)
    at = layers.GRU_MATRIX_GROUP_MIN_COLUMNS
    L = _lib.gru_matrix_group_lib()
    for n, save, on, group in ((at, False, True, True), (at + 5000, False, True, True), (at, True, True, False),
                               (at - 1, False, True, False), (1, False, True, False), (at, False, False, False)):
        monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX_GROUP", on)
        x = torch.empty(2, n, 4).as_subclass(OnGpu)
        want = ("gru_matrix_group", L.tk_gru_matrix_group_workspace_bytes(n, H, 256)) if group else main
        assert layers._rnn_route(layer, x, lengths_given, save) == want, (n, save, on)
        assert layers._rnn_route(lstm, x, lengths_given, save) == main
        assert layers._rnn_route(small, x, lengths_given, save) == main
        # never on a CPU tensor
        assert layers._rnn_route(layer, torch.empty(2, n, 4), lengths_given, save) == main
    monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX_GROUP", True)
    assert layers._rnn_route(layer, torch.empty(0, at, 4).as_subclass(OnGpu), lengths_given, False) == (None if lengths_given else main)

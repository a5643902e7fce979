"""include/taiyaki_amd_lstm_matrix_sizes.h on the host: the header, the libraries and the binding, the four queries and
the argument checks in front of a launch."""
import ctypes
import os
import subprocess

import pytest

from taiyaki_amd import _lib

ENTRIES = {"tk_lstm_matrix_sizes_" + n for n in ("supported", "columns", "slab", "workspace_bytes", "forward_dev")}
SIZES = (192, 384)


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.LSTM_MATRIX_SIZES_SIGNATURES) == ENTRIES
    for libname in (_lib.LSTM_MATRIX_SIZES_LIBNAME, _lib.LSTM_MATRIX_SIZES_LAB_LIBNAME):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                             capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if line.strip()} == ENTRIES, libname
    # the prototypes of the size-256 header
    group = {n.replace("_group_", "_sizes_"): v for n, v in _lib.LSTM_MATRIX_GROUP_SIGNATURES.items()}
    assert _lib.LSTM_MATRIX_SIZES_SIGNATURES == group
    L = _lib.lstm_matrix_sizes_lib()                    # resolves every symbol
    try:
        assert _lib.use_lab(True) and _lib.lstm_matrix_sizes_lib() is not L
    finally:
        _lib.use_lab(False)
    assert _lib.lstm_matrix_sizes_lib() is L


@pytest.mark.parametrize("H", SIZES)
def test_the_queries(H):
    L = _lib.lstm_matrix_sizes_lib()
    G, C = H // 32, L.tk_lstm_matrix_sizes_columns(H)
    assert L.tk_lstm_matrix_sizes_supported(H) == 1 and C in ((16,) if H == 384 else (16, 32))
    for h in (96, 128, 256, 512):
        assert L.tk_lstm_matrix_sizes_supported(h) == 0 and L.tk_lstm_matrix_sizes_columns(h) == 0, h
        assert L.tk_lstm_matrix_sizes_slab(h, 256) == 0 and L.tk_lstm_matrix_sizes_workspace_bytes(2048, h, 256) == 0, h
    for cus in (0, 1, G - 1):
        assert L.tk_lstm_matrix_sizes_slab(H, cus) == 0 and L.tk_lstm_matrix_sizes_workspace_bytes(64, H, cus) == 0
    for cus in (G, 64, 256, 304):
        S = L.tk_lstm_matrix_sizes_slab(H, cus)
        assert S == cus // G * C
        at = L.tk_lstm_matrix_sizes_workspace_bytes(S, H, cus)
        # both slots of a group's granules; grows by the group up to one slab, the same from there on
        assert L.tk_lstm_matrix_sizes_workspace_bytes(1, H, cus) == 2 * G * C * 32 * 8
        assert at == cus // G * L.tk_lstm_matrix_sizes_workspace_bytes(C, H, cus)
        assert all(L.tk_lstm_matrix_sizes_workspace_bytes(n, H, cus) == at for n in (S + 1, 2 * S + 3, 100 * S))
    assert L.tk_lstm_matrix_sizes_workspace_bytes(0, H, 256) == 0


@pytest.mark.parametrize("H", SIZES)
def test_the_entry_checks_its_arguments_before_anything_is_launched(H):
    L = _lib.lstm_matrix_sizes_lib()
    fwd = L.tk_lstm_matrix_sizes_forward_dev
    bad, unsupported, small = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED", "WORKSPACE"))
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    big = 1 << 30
    # a required pointer NULL or misaligned (w_hh needs a float's alignment), in front of the size
    assert fwd(None, p, None, 4, 3, H, 0, 256, p, p, big, p, None) == bad
    assert fwd(p, None, None, 4, 3, H, 0, 256, p, p, big, p, None) == bad
    assert fwd(p, p, None, 4, 3, 96, 0, 256, None, p, big, p, None) == bad
    assert fwd(odd, p, None, 4, 3, 96, 0, 256, p, p, big, p, None) == bad
    assert fwd(p, p, None, 4, 0, H, 0, 256, odd, p, big, p, None) == bad
    # nblk or nbatch beyond int32, in front of the size
    assert fwd(p, p, None, 1 << 31, 3, 96, 0, 256, p, p, big, p, None) == bad
    assert fwd(p, p, None, 4, 1 << 31, 96, 0, 256, p, p, big, p, None) == bad
    # the workspace and the status word: NULL, misaligned, in front of the size
    assert fwd(p, p, None, 4, 3, 96, 0, 256, p, None, big, p, None) == bad
    assert fwd(p, p, None, 4, 3, 96, 0, 256, p, odd, big, p, None) == bad
    assert fwd(p, p, None, 4, 3, 96, 0, 256, p, p, big, None, None) == bad
    # a size the kernel does not cover, no batch, no launch that fits: behind the pointer checks, in front of nblk = 0
    assert fwd(p, p, None, 4, 3, 96, 0, 256, p, p, big, p, None) == unsupported
    assert fwd(p, p, None, 0, 3, 256, 0, 256, p, p, big, p, None) == unsupported
    assert fwd(p, p, None, 0, 0, H, 0, 256, p, p, big, p, None) == unsupported
    assert fwd(p, p, None, 0, 3, H, 0, H // 32 - 1, p, p, big, p, None) == unsupported
    # a workspace below the query's answer, in front of nblk = 0
    need = L.tk_lstm_matrix_sizes_workspace_bytes(5000, H, 256)
    assert fwd(p, p, None, 0, 5000, H, 0, 256, p, p, need - 1, p, None) == small
    assert fwd(p, p, None, 0, 3, H, 0, 256, p, p, 0, p, None) == small
    # nothing to do at nblk = 0, behind the checks
    assert fwd(p, p, None, 0, 5000, H, 0, 256, p, p, need, p, None) == 0
    assert fwd(p, p, p, 0, 3, H, 1, H // 32, p, p, need, p, None) == 0

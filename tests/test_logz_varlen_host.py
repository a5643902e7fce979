"""CPU-only: include/taiyaki_amd_logz_varlen.h is the ABI of libtaiyaki_amd_logz_varlen.so, its checks come before a launch."""
import ctypes
import os
import re
import subprocess

from taiyaki_amd import _lib

ENTRIES = {"tk_flipflop_logz_varlen_workspace_bytes", "tk_flipflop_logz_varlen_dev", "tk_flipflop_loss_varlen_blocks_aux_bytes",
           "tk_flipflop_loss_fused_varlen_blocks_labels_dev"}
BAD_ARG, WORKSPACE = _lib.DEFINES["TK_ERR_BAD_ARG"], _lib.DEFINES["TK_ERR_WORKSPACE"]


def test_library_exports_exactly_what_its_header_declares():
    _lib.build()
    V = _lib.logz_varlen_lib()          # resolves every symbol with the header's types
    header = _lib._blank_comments(open(_lib.LOGZ_VARLEN_HEADER).read())
    assert set(re.findall(r"\b(tk_\w+)\s*\(", header)) == ENTRIES == set(_lib.LOGZ_VARLEN_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib.LOGZ_VARLEN_LIBNAME)],
                         capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"}
    assert exported == ENTRIES, exported ^ ENTRIES
    # the binding has the header's argument types
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    sigs = _lib.LOGZ_VARLEN_SIGNATURES
    assert V.tk_flipflop_logz_varlen_dev.argtypes == sigs["tk_flipflop_logz_varlen_dev"][1]
    assert sigs["tk_flipflop_logz_varlen_workspace_bytes"] == (sz, [sz, sz, sz])
    assert sigs["tk_flipflop_loss_varlen_blocks_aux_bytes"] == (sz, [sz, sz, sz, sz, i])
    # the contract, and so the arguments, of the one-wave posterior with lengths; the fused entry point's of its twin
    assert sigs["tk_flipflop_logz_varlen_dev"] == (i, [vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp]) == _lib.DECODE_VARLEN_SIGNATURES["tk_flipflop_posterior_varlen_dev"]
    assert sigs["tk_flipflop_loss_fused_varlen_blocks_labels_dev"] == _lib.LOSS_VARLEN_SIGNATURES["tk_flipflop_loss_fused_varlen_labels_dev"]


def test_workspace_is_the_fixed_length_operators():
    V, L, W = _lib.logz_varlen_lib(), _lib.lib(), _lib.loss_varlen_lib()
    for shape in ((800, 128), (800, 512), (131, 70), (7210, 275), (1, 1)):
        for nbase in (1, 2, 3, 4):
            want = L.tk_flipflop_logz_workspace_bytes(*shape, nbase)
            assert want > 0 and V.tk_flipflop_logz_varlen_workspace_bytes(*shape, nbase) == want
            assert V.tk_flipflop_loss_varlen_blocks_aux_bytes(*shape, nbase, 2 * nbase * (nbase + 1), 1) == want
    assert V.tk_flipflop_logz_varlen_workspace_bytes(800, 128, 0) == 0 and V.tk_flipflop_logz_varlen_workspace_bytes(800, 128, 5) == 0
    for ntrans in (40, 46, 39):         # the compact buffers are the one-wave entry point's
        assert V.tk_flipflop_loss_varlen_blocks_aux_bytes(800, 128, 4, ntrans, 0) == W.tk_flipflop_loss_varlen_aux_bytes(800, 128, 4, ntrans, 0)
    assert V.tk_flipflop_loss_varlen_blocks_aux_bytes(800, 128, 4, 40, 2) == 0 and V.tk_flipflop_loss_varlen_blocks_aux_bytes(800, 128, 5, 60, 0) == 0


def test_bad_arguments_are_refused_before_a_launch():
    """No pointer here is ever dereferenced: `one` is any non-NULL, 16-byte aligned value."""
    V, one, odd = _lib.logz_varlen_lib(), ctypes.c_void_p(16), ctypes.c_void_p(20)
    good = [one, one, 10, 2, 4, one, one, one, 1 << 20, None, None]
    for at, bad in ((0, None), (6, None), (7, None), (2, 0), (3, 0), (0, odd), (5, odd)):
        args = list(good)
        args[at] = bad
        assert V.tk_flipflop_logz_varlen_dev(*args) == BAD_ARG, (at, bad)
    assert V.tk_flipflop_logz_varlen_dev(one, None, 10, 2, 4, None, one, one, 16, None, None) == WORKSPACE
    assert V.tk_flipflop_logz_varlen_dev(one, None, 10, 2, 5, None, one, one, 1 << 20, None, None) == _lib.DEFINES["TK_ERR_UNSUPPORTED"]
    # the fused entry point: the checks of its twin, in their order (NULL lengths refused, then the size of `aux`), then
    # the launcher's own refusal of a shape with too many chunks for the middle kernel
    labels = _lib.SeqLabels(one, 3, 4, None, None, None, 0)
    args = [one, 10, 2, 40, ctypes.byref(labels), one, one, one, one, None, None, 2, 1.0, 1.0, None, one, one, one, one, 1 << 20,
            one, 1 << 20, one, 1 << 20, None, None]
    assert V.tk_flipflop_loss_fused_varlen_blocks_labels_dev(*args, None) == BAD_ARG
    args[23] = 16
    assert V.tk_flipflop_loss_fused_varlen_blocks_labels_dev(*args, one) == WORKSPACE
    args[1], args[23] = 40000, 1 << 40
    assert V.tk_flipflop_loss_fused_varlen_blocks_labels_dev(*args, one) == _lib.DEFINES["TK_ERR_UNSUPPORTED"]
    assert V.tk_flipflop_logz_varlen_dev(one, one, 40000, 2, 4, one, one, one, 1 << 40, None, None) == _lib.DEFINES["TK_ERR_UNSUPPORTED"]

"""CPU-only tests of the loss with a time length per column: include/taiyaki_amd_loss_varlen.h parses into its binding and
names exactly what libtaiyaki_amd_loss_varlen.so exports, `lengths` is validated before anything is launched or loaded,
tk_crf_varlen_plan is the launch rule (tests/test_crf_instantiations.py restates it in Python), and a call without lengths
never touches the new library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, ctc, layers, train
from tests.test_crf_instantiations import COLW, PLAIN, PLAN_FIELDS, plan_rule

ENTRIES = {"tk_crf_flipflop_varlen_labels_dev", "tk_flipflop_loss_fused_varlen_labels_dev", "tk_flipflop_loss_varlen_aux_bytes",
           "tk_crf_varlen_plan"}


def test_header_parses_and_names_the_librarys_exports():
    _lib.build()
    assert set(_lib.LOSS_VARLEN_SIGNATURES) == ENTRIES
    header = _lib._blank_comments(open(_lib.LOSS_VARLEN_HEADER).read())
    assert set(re.findall(r"\b(tk_\w+)\s*\(", header)) == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib.LOSS_VARLEN_LIBNAME)],
                         capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"}
    assert exported == ENTRIES, exported ^ ENTRIES
    V = _lib.loss_varlen_lib()      # resolves every symbol with the header's types
    # the entry points take the fixed-length ones' arguments, then lengths
    for ours, theirs in (("tk_crf_flipflop_varlen_labels_dev", "tk_crf_flipflop_labels_dev"),
                         ("tk_flipflop_loss_fused_varlen_labels_dev", "tk_flipflop_loss_fused_labels_dev")):
        res, args = _lib.LOSS_VARLEN_SIGNATURES[ours]
        assert (res, args[:-1]) == _lib.SIGNATURES[theirs] and args[-1] is ctypes.c_void_p
    # the compact buffers: the log-partition's gradient on the canonical columns, and for cat-mod a copy of them in front
    one = (800 * 128 * 40 * 4 + 255) // 256 * 256
    assert V.tk_flipflop_loss_varlen_aux_bytes(800, 128, 4, 40, 0) == one
    assert V.tk_flipflop_loss_varlen_aux_bytes(800, 128, 4, 46, 0) == 2 * one
    assert V.tk_flipflop_loss_varlen_aux_bytes(800, 128, 4, 40, 1) == _lib.decode_varlen_lib().tk_decode_varlen_workspace_bytes(800, 128, 4)
    assert V.tk_flipflop_loss_varlen_aux_bytes(800, 128, 4, 40, 2) == 0 and V.tk_flipflop_loss_varlen_aux_bytes(800, 128, 5, 60, 1) == 0
    # NULL arguments are refused before anything is launched
    assert V.tk_crf_flipflop_varlen_labels_dev(None, 40, 10, 2, None, None, None, None, None, None, None, 0, 40, 1.0, 1.0, 1.0,
                                               None, None, None, 0, None, None, None) == _lib.DEFINES["TK_ERR_BAD_ARG"]
    assert V.tk_flipflop_loss_fused_varlen_labels_dev(None, 10, 2, 40, None, None, None, None, None, None, None, 0, 1.0, 1.0, None,
                                                      None, None, None, None, 0, None, 0, None, 0, None, None,
                                                      None) == _lib.DEFINES["TK_ERR_BAD_ARG"]


def test_fused_entry_refuses_null_lengths():
    """The fused entry point has no log-partition half without lengths (kernel B is the flip-flop library's): an otherwise
    valid call with lengths == NULL is TK_ERR_BAD_ARG, before anything is launched -- no pointer here is ever dereferenced.
    (The CRF entry point takes NULL: tests/test_loss_varlen.py.)"""
    V, one = _lib.loss_varlen_lib(), ctypes.c_void_p(16)        # (any non-NULL, 16-byte aligned value)
    labels = _lib.SeqLabels(one, 3, 4, None, None, None, 0)
    args = [one, 10, 2, 40, ctypes.byref(labels), one, one, one, one, None, None, 2, 1.0, 1.0, None, one, one, one, one, 1 << 20,
            one, 1 << 20, one, 1 << 20, None, None]
    assert V.tk_flipflop_loss_fused_varlen_labels_dev(*args, None) == _lib.DEFINES["TK_ERR_BAD_ARG"]
    # ... and it is the NULL lengths that is refused: with them the checks go on to the next one, the size of `aux`
    args[23] = 16
    assert V.tk_flipflop_loss_fused_varlen_labels_dev(*args, one) == _lib.DEFINES["TK_ERR_WORKSPACE"]


def _calls(x, lengths):
    seqs, seqlens = torch.tensor([0, 1, 2]), torch.tensor([2, 1])
    cmo, mcw = np.array([0, 2, 4, 5, 6], dtype=np.int32), np.full(6, 8.0, dtype=np.float32)
    yield lambda: ctc.crf_flipflop_loss(x[:, :, :40], seqs, seqlens, 1.0, lengths=lengths)
    yield lambda: ctc.cat_mod_flipflop_loss(x, seqs, seqlens, torch.zeros(3, dtype=torch.int64), cmo, mcw, 1.0, lengths=lengths)
    yield lambda: ctc.flipflop_loss(x[:, :, :40], seqs, seqlens, 1.0, lengths=lengths)
    yield lambda: ctc.flipflop_mean_loss(x[:, :, :40], seqs, seqlens, 1.0, lengths=lengths)
    yield lambda: layers.flipflop_logpartition(x[:, :, :40], lengths=lengths)


@pytest.mark.parametrize("bad", [[6], [6, 6, 6], [-1, 3], [7, 3], [3.0, 2.0], np.array([1.5, 2.0]), "ab", [[6, 6]]])
def test_lengths_are_validated_before_anything_runs(bad):
    """Wrong size, negative, above nblk, a float dtype: a ValueError from every operator, on the host, before the tensor's
    device is even looked at."""
    x = torch.zeros(6, 2, 46)
    for call in _calls(x, bad):
        with pytest.raises(ValueError, match="lengths must hold one integer"):
            call()
    with pytest.raises(ValueError, match="lengths must hold one integer"):
        ctc.crf_flipflop_loss(x[:, :, :40], torch.tensor([0]), torch.tensor([1, 0]), 1.0, lengths=torch.tensor([1.0, 2.0]))


def test_valid_lengths_reach_the_no_fallback_error_and_none_never_loads_the_library(monkeypatch):
    """Valid lengths on a CPU tensor: the operators' own error (no CPU fallback).  Without lengths nothing asks for the new
    library -- its loader is replaced by one that fails."""
    x = torch.zeros(6, 2, 46)
    for lengths in ([6, 0], np.array([3, 6]), torch.tensor([1, 2], dtype=torch.int32)):
        for call in _calls(x, lengths):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()

    def refuse():
        raise AssertionError("a call without lengths asked for libtaiyaki_amd_loss_varlen.so")
    monkeypatch.setattr(_lib, "loss_varlen_lib", refuse)
    for call in _calls(x, None):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()

    class Net(torch.nn.Module):
        def forward(self, indata):
            return x[:, :, :40]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.calculate_loss(Net(), None, torch.tensor([0, 1, 2]), torch.tensor([2, 1]))


def _lib_plan(ntrans, nblk, nbatch, max_seqlen, bulk, form, want_grad, sharp):
    wsb = _lib.lib().tk_crf_flipflop_workspace_bytes_sharp(ntrans, nblk, nbatch, max_seqlen, int(want_grad), float(sharp))
    out = (ctypes.c_size_t * 20)()
    if not _lib.loss_varlen_lib().tk_crf_varlen_plan(ntrans, nblk, nbatch, max_seqlen, bulk, form, int(want_grad), float(sharp), wsb, out):
        return None
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def test_plan_is_the_launch_rule_at_the_gpu_tests_shapes():
    """tk_crf_varlen_plan == tests/test_crf_instantiations.py's plan_rule (the rule of crf_choose restated in Python) at the
    shapes tests/test_loss_varlen.py runs, and the block lengths, cells per lane and waves its cases are named by."""
    shapes = []
    for form, S in ((PLAIN, 40), (COLW, 46)):
        for sharp in (1.0, 1.5, 2.5):
            for nblk in (61, 37, 90, 200):
                shapes += [(S, nblk, 7, L, bulk, form, g, sharp) for L, bulk in ((30, 30), (18, 16), (1, 0), (190, 60)) if L <= nblk + 1
                           for g in (0, 1)]
    shapes += [(40, 2100, 2, L, 500, PLAIN, g, 1.0) for L in (600, 1100, 2080) for g in (0, 1)]
    for args in shapes:
        assert _lib_plan(*args) == plan_rule(*args), args
    at61 = {(f, s): _lib_plan(S, 61, 7, 30, 30, f, 1, s)["BK"] for f, S in ((PLAIN, 40), (COLW, 46)) for s in (1.0, 1.5, 2.5)}
    assert at61 == {(PLAIN, 1.0): 12, (PLAIN, 1.5): 8, (PLAIN, 2.5): 4, (COLW, 1.0): 8, (COLW, 1.5): 8, (COLW, 2.5): 4}
    long_ = {L: _lib_plan(40, 2100, 2, L, 500, PLAIN, 1, 1.0) for L in (600, 1100, 2080)}
    assert long_[600]["W"] > 1 and long_[1100]["R"] == 2 and long_[2080]["R"] == 4 and all(p["log_domain"] == 0 for p in long_.values())
    # refused: a form the labels entry points do not run, no workspace
    out = (ctypes.c_size_t * 20)()
    V = _lib.loss_varlen_lib()
    assert not V.tk_crf_varlen_plan(46, 61, 7, 30, 30, 2, 1, 1.0, 1 << 30, out) and not V.tk_crf_varlen_plan(40, 61, 7, 30, 30, 0, 1, 1.0, 0, out)
    assert not V.tk_crf_varlen_plan(40, 61, 7, 30, 30, 0, 1, 1.0, 1 << 30, None)

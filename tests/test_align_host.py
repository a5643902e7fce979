"""include/taiyaki_amd_align.h on the host: the definition (tests/align_support.py against hand-worked cases), the band
rule and tk_align_band, the header, the library and the binding, the limits, CPU tensors."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, accuracy, train
from tests import align_support as support

ENTRIES = {"tk_align_band", "tk_align_pairs_dev", "tk_align_calls_dev"}
MAX_LEN, MAX_BAND = _lib.ALIGN_DEFINES["TK_ALIGN_MAX_LEN"], _lib.ALIGN_DEFINES["TK_ALIGN_MAX_BAND"]


def _band(m, n, t):
    out = [ctypes.c_int(-99) for _ in range(3)]
    rc = _lib.align_lib().tk_align_band(m, n, -1 if t is None else t, *[ctypes.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


@pytest.mark.parametrize("query, ref, want", [
    ("ACGT", "ACGT", (0, 4)), ("AAAA", "AAA", (1, 3)), ("", "ACG", (3, 0)), ("", "", (0, 0)),
    ("AAC", "ACA", (2, 2)),         # A-AC / ACA-: two gaps keep two matches; two substitutions would keep one
    # the transposition likewise: A-CGT / AGC-T has D = 2 with M = 3.  (The substitutions alone, ACGT / AGCT column by
    # column, give D = 2, M = 2; by the definition -- the most matches at the least distance -- that is not the answer.)
    ("ACGT", "AGCT", (2, 3)),
])
def test_definition_on_hand_worked_cases(query, ref, want):
    assert support.align_plain(query, ref) == want
    assert support.align_rows(query, ref) == want
    assert support.align_banded(query, ref, None) == want + (1,)
    assert support.align_plain(ref, query) == want          # (the recurrence is symmetric)


def test_row_form_of_the_support_code_is_the_plain_one():
    rng = np.random.RandomState(1)
    for _ in range(60):
        r = rng.randint(0, rng.choice([1, 2, 4]) + 1, size=rng.randint(0, 40))
        q = support.mutate(r, rng.choice([0.0, 0.1, 0.5]), rng) if rng.rand() < 0.6 else rng.randint(0, 3, size=rng.randint(0, 40))
        assert support.align_rows(q, r) == support.align_plain(q, r)


def test_band_query_follows_the_rule():
    for m, n in itertools.product(range(13), repeat=2):
        for t in [None] + list(range(15)):
            rc, (first, last, cells) = _band(m, n, t)
            assert rc == 0
            if t is not None and t < abs(n - m):
                assert (first, last, cells) == (1, 0, 0)
                assert support.band_rule(m, n, t) is None
                continue
            # section "Band": j - i in [-p, (n - m) + p] for n >= m, mirrored for n < m, p = floor((t - |n - m|) / 2) ...
            if t is None:
                lo, hi = -m, n
            else:
                p = (t - abs(n - m)) // 2
                lo, hi = (-p, n - m + p) if n >= m else (n - m - p, p)
            # ... of which the table has -m .. n
            assert (first, last) == (max(lo, -m), min(hi, n)) == support.band_rule(m, n, t), (m, n, t)
            assert cells == 1 == support.cells_per_lane(last - first + 1)


def test_banded_sweep_is_the_full_one_wherever_it_says_so():
    rng = np.random.RandomState(2)
    seen = {0: 0, 1: 0}
    for m, n in itertools.product(range(13), repeat=2):
        q, r = rng.randint(0, 2, size=m), rng.randint(0, 2, size=n)
        full = support.align_plain(q, r)
        for t in range(15):
            d, mt, exact = support.align_banded(q, r, t)
            assert exact == int(t >= abs(n - m) and d <= t)
            assert exact == int(full[0] <= t), (m, n, t)        # every alignment of cost <= t lies inside the band
            if exact:
                assert (d, mt) == full, (m, n, t)
            elif t < abs(n - m):
                assert (d, mt) == (max(m, n), 0)
            seen[exact] += 1
    assert min(seen.values()) > 200


def test_cells_per_lane_boundaries():
    for width, want in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8), (513, 16), (1024, 16),
                        (1025, 17), (1088, 17), (1089, 19), (1216, 19), (1217, 21), (MAX_BAND, 255)):
        assert support.cells_per_lane(width) == want
        rc, (first, last, cells) = _band(width - 1, 0, None)        # every diagonal of a (width - 1) x 0 table
        assert rc == 0 and (first, last, cells) == (-(width - 1), 0, want), width
    rc, band = _band(700, 650, 90)
    assert rc == 0 and band == (-70, 20, 2)


def _exported(libname):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                         capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.ALIGN_SIGNATURES) == ENTRIES == _exported(_lib.ALIGN_LIBNAME)
    _lib.align_lib()                                    # resolves every symbol
    sz, i, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    assert _lib.ALIGN_SIGNATURES["tk_align_band"] == (i, [sz, sz, i, vp, vp, vp])
    assert _lib.ALIGN_SIGNATURES["tk_align_pairs_dev"] == (i, [vp, vp, vp, vp, sz, vp, vp, i, sz, vp, vp, vp, vp])
    assert _lib.ALIGN_SIGNATURES["tk_align_calls_dev"] == (i, [vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp])
    assert _lib.ALIGN_DEFINES == dict(TK_ALIGN_MAX_LEN=65534, TK_ALIGN_REG_BAND=1024, TK_ALIGN_MAX_BAND=16320,
                                      TK_ALIGN_MAX_CALL=4096, TK_ALIGN_MAX_CALL_BAND=8128)


def test_flipflop_library_exports_are_what_they_were():
    assert not any("align" in name for name in _exported(_lib.LIBNAME))
    assert not any("align" in name for name in _lib.SIGNATURES)


def test_limits_are_refused_with_the_right_code():
    L = _lib.align_lib()
    bad, unsupported = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED"))
    p = ctypes.c_void_p(4096)
    # the band query: lengths, then the band's width
    assert _band(MAX_LEN + 1, 5, 3)[0] == unsupported and _band(5, MAX_LEN + 1, None)[0] == unsupported
    assert _band(MAX_LEN, MAX_LEN, 8) == (0, (-4, 4, 1))
    assert _band(MAX_BAND - 1, 0, None)[0] == 0 and _band(MAX_BAND, 0, None)[0] == unsupported
    assert _band(MAX_LEN, MAX_LEN, MAX_BAND - 1)[0] == 0 and _band(MAX_LEN, MAX_LEN, MAX_BAND + 1)[0] == unsupported
    assert L.tk_align_band(3, 3, 1, None, p, p) == bad
    # the launches: nothing to do first, then pointers, then limits -- nothing is launched by any of these
    pairs, calls = L.tk_align_pairs_dev, L.tk_align_calls_dev
    assert pairs(None, None, None, None, 0, None, None, -1, 0, None, None, None, None) == 0
    assert pairs(None, p, p, p, 3, None, None, -1, 0, p, p, p, None) == bad
    assert pairs(p, p, p, p, 3, None, None, -1, 0, p, p, None, None) == bad
    assert pairs(p, p, p, p, 1 << 31, None, None, -1, 0, p, p, p, None) == unsupported
    assert pairs(p, p, p, p, 3, None, None, -1, MAX_BAND + 1, p, p, p, None) == unsupported
    assert calls(None, None, 50, 0, 4, None, None, None, 0, None, None, None, None) == 0
    assert calls(None, None, 50, 9, 4, p, p, p, 0, p, p, p, None) == bad
    assert calls(p, None, 50, 9, 4, p, None, p, 0, p, p, p, None) == bad
    assert calls(p, None, _lib.ALIGN_DEFINES["TK_ALIGN_MAX_CALL"], 9, 4, p, p, p, 0, p, p, p, None) == unsupported
    assert calls(p, None, 50, 9, 0, p, p, p, 0, p, p, p, None) == unsupported
    assert calls(p, None, 50, 9, 128, p, p, p, 0, p, p, p, None) == unsupported
    assert calls(p, None, 50, 9, 4, p, p, p, _lib.ALIGN_DEFINES["TK_ALIGN_MAX_CALL_BAND"] + 1, p, p, p, None) == unsupported


def test_python_refuses_what_the_host_can_see_and_cpu_tensors():
    # (checked before any device is touched)
    with pytest.raises(ValueError, match="longer than"):
        accuracy.align_pairs([np.zeros(MAX_LEN + 1, dtype=np.uint8)], ["A"])
    with pytest.raises(ValueError, match="longer than"):
        accuracy.align_pairs_exact(["A"], [np.zeros(MAX_LEN + 1, dtype=np.uint8)])
    with pytest.raises(ValueError, match="diagonals"):
        accuracy.align_pairs([np.zeros(MAX_BAND, dtype=np.uint8)], ["A"])           # every diagonal: m + n + 1 of them
    with pytest.raises(ValueError, match="one entry per pair"):
        accuracy.align_pairs(["A", "C"], ["A", "C"], max_distance=[1, 2, 3])
    cpu_pairs = (torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 2, 4]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        accuracy.align_pairs(cpu_pairs, cpu_pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        accuracy.align_pairs_exact(cpu_pairs, cpu_pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        accuracy.call_accuracy(torch.zeros(5, 2, 40), torch.zeros(4, dtype=torch.int64), torch.tensor([2, 2]))
    with pytest.raises(ValueError, match="both"):
        accuracy.align_pairs(cpu_pairs, ["AC", "GT"])
    assert callable(train.validation_accuracy)


def test_summary():
    acc = np.array([0.95, 0.951, 0.958, 0.91, 0.5, np.nan, 0.899], dtype=np.float32)
    s = accuracy.summary(torch.from_numpy(acc))
    good = acc[~np.isnan(acc)].astype(np.float64)
    assert s["n"] == 6 and s["mean"] == pytest.approx(good.mean()) and s["median"] == pytest.approx(np.median(good))
    assert s["mode"] == pytest.approx(0.955) and s["above_90"] == pytest.approx(4 / 6)
    assert accuracy.summary([1.0])["mode"] == pytest.approx(0.995)
    assert accuracy.summary([])["n"] == 0 and np.isnan(accuracy.summary([np.nan])["mean"])

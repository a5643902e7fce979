"""include/taiyaki_amd_conv_window.h (libtaiyaki_amd_conv_window.so: csrc/conv_strided.hip built -DTK_CONV_WINDOW), what
the host decides: the header, the binding and the exports name the same entries; the rule; the plan; bad arguments.  No
GPU: the pointers of these calls are never dereferenced."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from taiyaki_amd import _lib, layers

CUS = 256
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
CIN = 16
GEOMETRIES = ((19, 5), (31, 10), (31, 12))          # (winlen, stride) the rule admits
OTHER_GEOMETRIES = ((19, 2), (19, 10), (31, 5), (29, 10))
ADMITTED = (96, 128, 192, 256, 384)                 # every Cout the rule admits
COUTS = (16, 64, 96, 128, 192, 255, 256, 384, 512)
RT, NT, KB = 128, 128, 16       # the GEMMs' tile and k block (csrc/conv_strided.hip)
B_BLOCK = 3 * 4 * 1024          # bytes of the three weight images of one (column tile, k block)
WG_TILE, CHAIN = 128, 8192      # the weight gradient's tile edge and longest accumulation chain
PLAN_KEYS = ("tiles_m", "f_tiles_n", "f_nkb", "f_grid", "d_tiles_n", "d_nkb", "splits", "nsub", "run_rows", "sub_rows",
             "w_grid", "bytes")
ENTRIES = {"tk_conv_window_supported", "tk_conv_window_workspace_bytes", "tk_conv_window_forward_dev",
           "tk_conv_window_backward_dev"}
LAB_ENTRIES = {"tk_lab_conv_window_set_splits", "tk_lab_conv_window_plan"}


def _cdiv(a, b):
    return -(-a // b)


def plan_py(T, N, cout, win, stride, cus=CUS, splits=0):
    """The plan restated: None where the kernels do not run."""
    if T == 0 or N == 0 or cus <= 0 or cout not in ADMITTED or (win, stride) not in GEOMETRIES:
        return None
    kw = CIN * win
    rows = _cdiv(T, stride) * N
    if rows * max(kw, cout) >= 1 << 31:
        return None
    tm = _cdiv(rows, RT)
    f_tn, d_tn, d_nkb = _cdiv(cout, NT), _cdiv(stride * CIN, NT), 4 * cout // KB
    wm, wn = _cdiv(cout, WG_TILE), _cdiv(kw, WG_TILE)
    G = splits if splits > 0 else max(cus // (wm * wn), 1)
    run = _cdiv(_cdiv(rows, G), KB) * KB
    G = _cdiv(rows, run)
    nsub = _cdiv(run, CHAIN)
    sub = _cdiv(_cdiv(run, nsub), KB) * KB
    slab = (cout * kw + cout + 3) // 4 * 4
    nbytes = (f_tn * win + d_tn * d_nkb) * B_BLOCK + G * nsub * slab * 4
    return dict(tiles_m=tm, f_tiles_n=f_tn, f_nkb=win, f_grid=_cdiv(tm, 8) * 8 * f_tn, d_tiles_n=d_tn, d_nkb=d_nkb,
                splits=G, nsub=nsub, run_rows=run, sub_rows=sub, w_grid=_cdiv(wm * G, 8) * 8 * wn, bytes=nbytes)


def plan(L, T, N, cout, win, stride, cus=CUS):
    out = (ctypes.c_size_t * 12)()
    if not L.tk_lab_conv_window_plan(T, N, cout, win, stride, cus, out):
        return None
    return dict(zip(PLAN_KEYS, out))


def _exports(libname):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                         capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.CONV_WINDOW_SIGNATURES) == ENTRIES
    assert set(_lib.CONV_WINDOW_LAB_SIGNATURES) == LAB_ENTRIES
    assert len(_lib.CONV_WINDOW_SIGNATURES["tk_conv_window_supported"][1]) == 4
    assert len(_lib.CONV_WINDOW_SIGNATURES["tk_conv_window_workspace_bytes"][1]) == 6
    assert len(_lib.CONV_WINDOW_SIGNATURES["tk_conv_window_forward_dev"][1]) == 14
    assert len(_lib.CONV_WINDOW_SIGNATURES["tk_conv_window_backward_dev"][1]) == 17
    declared = set(re.findall(r"\b(tk_\w+)\s*\(", _lib._blank_comments(open(_lib.CONV_WINDOW_HEADER).read())))
    assert declared == ENTRIES | LAB_ENTRIES
    assert _exports(_lib.CONV_WINDOW_LIBNAME) == ENTRIES
    assert _exports(_lib.CONV_WINDOW_LAB_LIBNAME) == ENTRIES | LAB_ENTRIES
    L = _lib.conv_window_lib()          # every symbol resolves
    assert not hasattr(L, "tk_lab_conv_window_plan") or _lib.is_lab()


def test_the_strided_library_keeps_its_entries():
    """the second build of the source adds nothing to libtaiyaki_amd_conv_strided.so"""
    assert _exports(_lib.CONV_STRIDED_LIBNAME) == set(_lib.CONV_STRIDED_SIGNATURES)
    assert _exports(_lib.CONV_STRIDED_LAB_LIBNAME) == set(_lib.CONV_STRIDED_SIGNATURES) | set(
        _lib.CONV_STRIDED_LAB_SIGNATURES)


def test_the_rule_admits_what_is_documented():
    """cin 16, (winlen, stride) one of (19, 5), (31, 10), (31, 12) and Cout 96, 128, 192, 256 or 384: nothing else; the
    workspace is 0 for an empty input, for no CUs and from rows x max(16 winlen, Cout) = 2^31 on (the kernels' 32-bit
    indices), at every size and geometry."""
    L = _lib.conv_window_lib()
    ws = L.tk_conv_window_workspace_bytes
    for cout in COUTS:
        for win, stride in GEOMETRIES + OTHER_GEOMETRIES:
            want = cout in ADMITTED and (win, stride) in GEOMETRIES
            assert bool(L.tk_conv_window_supported(CIN, cout, win, stride)) == want, (cout, win, stride)
            assert (ws(100, 3, cout, win, stride, CUS) > 0) == want, (cout, win, stride)
            if want:
                assert ws(100, 3, cout, win, stride, CUS) == plan_py(100, 3, cout, win, stride)["bytes"]
    for cin in (1, 4, 8, 15, 17, 32):
        for win, stride in GEOMETRIES:
            assert not L.tk_conv_window_supported(cin, 256, win, stride), (cin, win, stride)
    for win, stride in GEOMETRIES:
        kw = CIN * win
        for cout in ADMITTED:
            assert ws(0, 3, cout, win, stride, CUS) == 0 and ws(100, 0, cout, win, stride, CUS) == 0
            assert ws(100, 3, cout, win, stride, 0) == 0 and ws(100, 3, cout, win, stride, -1) == 0
            edge = _cdiv(1 << 31, max(kw, cout))    # the first number of rows with rows x max(16 winlen, Cout) >= 2^31
            assert ws(stride * (edge - 1), 1, cout, win, stride, CUS) > 0
            assert ws(stride * edge, 1, cout, win, stride, CUS) == 0
            assert ws(stride, edge - 1, cout, win, stride, CUS) > 0 and ws(stride, edge, cout, win, stride, CUS) == 0
            assert ws(stride + 1, edge - 1, cout, win, stride, CUS) == 0
            assert ws(1 << 40, 1 << 30, cout, win, stride, CUS) == 0


def test_the_layers_workspace_covers_the_trainers_shapes():
    """one cached size for the DNA fast shapes; the RNA shapes with two partial results per run regrow it"""
    ws = _lib.conv_window_lib().tk_conv_window_workspace_bytes
    for cout in (96, 128):
        for T, N in [(4000, 128), (2000, 256)]:
            assert 0 < ws(T, N, cout, 19, 5, CUS) <= layers._CONV_WINDOW_WORKSPACE_BYTES
    assert 0 < ws(20000, 128, 96, 31, 12, CUS) <= layers._CONV_WINDOW_WORKSPACE_BYTES


def test_plan_hook_agrees_with_the_python_rule(labenv):
    labenv.lib()
    L = _lib.conv_window_lib()
    assert _lib.is_lab()
    rna = plan(L, 20000, 128, 256, 31, 10)
    assert (rna["tiles_m"], rna["f_tiles_n"], rna["f_nkb"], rna["d_tiles_n"], rna["d_nkb"]) == (2000, 2, 31, 2, 64)
    assert (rna["splits"], rna["nsub"]) == (32, 1)
    fast = plan(L, 4000, 128, 96, 19, 5)
    assert (fast["f_tiles_n"], fast["d_tiles_n"], fast["d_nkb"], fast["splits"]) == (1, 1, 24, 85)
    try:
        for splits in (0, 1, 3):
            L.tk_lab_conv_window_set_splits(splits)
            for win, stride in GEOMETRIES:
                for T, N in [(1, 1), (stride - 1, 1), (stride, 63), (stride + 1, 65), (47, 100), (128 * stride + 1, 1),
                             (128 * stride + 1, 100), (4000, 128), (20000, 128), (0, 4), (4, 0)]:
                    for cus in (1, 4, 8, 256, 304):
                        for cout in (96, 256):
                            want = plan_py(T, N, cout, win, stride, cus=cus, splits=splits)
                            assert plan(L, T, N, cout, win, stride, cus=cus) == want, (T, N, cout, win, stride, cus, splits)
                            assert L.tk_conv_window_workspace_bytes(T, N, cout, win, stride, cus) == (
                                want["bytes"] if want else 0)
                for cout in ADMITTED:
                    assert plan(L, 641, 100, cout, win, stride) == plan_py(641, 100, cout, win, stride, splits=splits)
            assert plan(L, 100, 3, 64, 31, 10) is None and plan(L, 100, 3, 256, 31, 5) is None
    finally:
        L.tk_lab_conv_window_set_splits(0)


def test_bad_arguments_are_refused_before_any_launch():
    """NULL, a misaligned workspace or tensor -> TK_ERR_BAD_ARG, a workspace one byte short -> TK_ERR_WORKSPACE, a
    shape outside the rule or rows x max(16 winlen, Cout) >= 2^31 -> TK_ERR_UNSUPPORTED: decided on the host."""
    L = _lib.conv_window_lib()
    T, N = 47, 3
    names = ("dy", "x", "z", "w", "b", "y", "dz", "dx", "dw", "db", "ws")
    good = {n: ctypes.c_void_p(4096 * (i + 1)) for i, n in enumerate(names)}
    null = ctypes.c_void_p(0)
    for win, stride in GEOMETRIES:
        for cout in (96, 256):
            need = L.tk_conv_window_workspace_bytes(T, N, cout, win, stride, CUS)
            assert need > 0

            def fwd(wsb=need, shape=(T, N, cout, win, stride), **kw):
                p = dict(good, **kw)
                return L.tk_conv_window_forward_dev(p["x"], p["w"], p["b"], *shape, CUS, p["z"], p["y"], p["ws"], wsb,
                                                    None)

            def bwd(wsb=need, shape=(T, N, cout, win, stride), **kw):
                p = dict(good, **kw)
                return L.tk_conv_window_backward_dev(p["dy"], p["x"], p["z"], p["w"], *shape, CUS, p["dz"], p["dx"],
                                                     p["dw"], p["db"], p["ws"], wsb, None)

            for call, needs, aligned in (
                    (fwd, ("x", "w", "b", "y", "ws"), ("x", "z", "y", "ws")),
                    (bwd, ("dy", "x", "z", "w", "dz", "dw", "db", "ws"), ("dy", "x", "z", "dz", "dx", "ws"))):
                for name in needs:
                    assert call(**{name: null}) == BAD_ARG, name
                for name in aligned:
                    assert call(**{name: ctypes.c_void_p(4096 + 4)}) == BAD_ARG, name
                assert call(wsb=need - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
                outside = [(0, N, cout, win, stride), (T, 0, cout, win, stride), (T, N, 64, win, stride),
                           (T, N, 255, win, stride), (T, N, 512, win, stride), (T, N, cout, win, stride + 1),
                           (T, N, cout, win - 2, stride), (T, N, cout, 31, 5), (T, N, cout, 19, 10)]
                for shape in outside:
                    assert call(shape=shape, wsb=1 << 62) == UNSUPPORTED, shape
                edge = _cdiv(1 << 31, max(CIN * win, cout))
                assert call(shape=(stride, edge, cout, win, stride), wsb=1 << 62) == UNSUPPORTED
                assert call(shape=(stride, edge - 1, cout, win, stride), wsb=0) == WORKSPACE


@pytest.mark.parametrize("win,stride", GEOMETRIES)
def test_cpu_tensors_keep_the_gemm_path(win, stride):
    torch.manual_seed(3)
    layer = layers.Convolution(CIN, 96, win, stride=stride, fun=layers.swish)
    x = torch.randn(47, 3, CIN)
    before = dict(layers.conv_window_calls)
    with torch.no_grad():
        assert not layer._hip_window(x)
        want = layers.swish(layer.conv(layer.pad(x.permute(1, 2, 0)))).permute(2, 0, 1)
        got = layer(x)
    assert got.shape == (_cdiv(47, stride), 3, 96) and torch.allclose(got, want, atol=1e-5)
    assert layers.conv_window_calls == before


def test_the_grad_mode_table_names_only_shapes_of_the_rule():
    L = _lib.conv_window_lib()
    assert layers.USE_HIP_CONV_WINDOW is True and set(layers.conv_window_calls) == {"forward", "backward"}
    for size, win, stride in layers.CONV_WINDOW_GRAD_SHAPES:
        assert L.tk_conv_window_supported(CIN, size, win, stride), (size, win, stride)
        assert not _lib.conv_strided_lib().tk_conv_strided_supported(CIN, size, win, stride), (size, win, stride)

"""The output layer's C ABI (include/taiyaki_amd_out_layer.h, csrc/out_layer.hip) as far as the host decides it: the
binding, the `supported` and workspace rules, the refusal of bad arguments before any launch, the plan hook against a
Python restatement of the tile rule, the cat-mod tables, and the dispatch's switch.  No GPU: no pointer is dereferenced."""
import ctypes

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, layers

CUS = 256
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
WIDTHS = (16, 32, 64, 96, 128, 192, 256, 384)
RT, KB, FRAG, CHAIN = 128, 16, 1024, 8192   # the forward's row tile, k per block, bytes of a fragment, the longest chain
WG_WAVES = 8                                # waves of a weight-gradient workgroup at most


def _plan_py(rows, I, L, O, cus):
    """The tile rule restated: None where the kernels do not run."""
    if rows == 0 or cus <= 0 or I not in WIDTHS or not 1 <= L <= 64 or not L <= O <= 64:
        return None
    if rows * max(I, 64) >= 1 << 31:
        return None
    nb, nkb, klb, cb = -(-L // 32), I // KB, -(-L // KB), -(-I // 32)
    nw = -(-(I + 1) // 32)              # a run's waves: 32-column blocks of [x | 1]; with few of them, more runs per CU
    per_run = -(-rows // (cus * -(-WG_WAVES // nw)))
    run = min(-(-per_run // KB) * KB, CHAIN)
    runs = -(-rows // run)
    slab = (L * I + L + 3) // 4 * 4
    nbytes = (nkb * nb + klb * cb + -(-rows // 32) * 2 * nb) * 3 * FRAG + runs * slab * 4
    return dict(rt=RT, nt=32 * nb, nkb=nkb, grid=-(-rows // RT), runs=runs, run_rows=run, bytes=nbytes)


def _plan(P, rows, I, L, O, cus=CUS):
    out = (ctypes.c_size_t * 7)()
    if not P.tk_lab_out_layer_plan(rows, I, L, O, cus, out):
        return None
    return dict(zip(("rt", "nt", "nkb", "grid", "runs", "run_rows", "bytes"), out))


def test_header_parses_into_the_binding():
    assert set(_lib.OUT_LAYER_SIGNATURES) == {"tk_out_layer_supported", "tk_out_layer_workspace_bytes",
                                              "tk_out_layer_forward_dev", "tk_out_layer_backward_dev"}
    assert set(_lib.OUT_LAYER_LAB_SIGNATURES) == {"tk_lab_out_layer_plan"}
    res, args = _lib.OUT_LAYER_SIGNATURES["tk_out_layer_supported"]
    assert res is ctypes.c_int and args == [ctypes.c_size_t] * 3
    res, args = _lib.OUT_LAYER_SIGNATURES["tk_out_layer_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_size_t] * 3 + [ctypes.c_int]
    res, args = _lib.OUT_LAYER_SIGNATURES["tk_out_layer_forward_dev"]
    assert res is ctypes.c_int and len(args) == 15 and args[:5] == [ctypes.c_void_p] * 5 and args[9] is ctypes.c_float
    res, args = _lib.OUT_LAYER_SIGNATURES["tk_out_layer_backward_dev"]
    assert res is ctypes.c_int and len(args) == 18 and args[10] is ctypes.c_float
    P = _lib.out_layer_lib()        # every symbol resolves
    assert not hasattr(P, "tk_lab_out_layer_plan") or _lib.is_lab()


def test_supported_rule():
    P = _lib.out_layer_lib()
    for I in range(0, 400):
        assert P.tk_out_layer_supported(I, 40, 40) == (I in WIDTHS), I
    for L in range(0, 70):
        for O in (L - 1, L, L + 1, 64, 65):
            if O >= 0:
                assert P.tk_out_layer_supported(96, L, O) == (1 <= L <= 64 and L <= O <= 64), (L, O)
    assert P.tk_out_layer_supported(512, 40, 40) == 0 and P.tk_out_layer_supported(1 << 40, 40, 40) == 0


def test_workspace_rule():
    """0 for a zero size, an unsupported width or rows x max(I, 64) at 2^31; otherwise the restated sum, a function of
    the four arguments only (asked twice, in another order, the answers are the same)."""
    ws = _lib.out_layer_lib().tk_out_layer_workspace_bytes
    assert ws(0, 96, 40, CUS) == 0 and ws(5, 0, 40, CUS) == 0 and ws(5, 96, 0, CUS) == 0 and ws(5, 96, 40, 0) == 0
    assert ws(5, 100, 40, CUS) == 0 and ws(5, 96, 65, CUS) == 0 and ws(5, 512, 40, CUS) == 0
    assert ws((1 << 31) // 384, 384, 40, CUS) == 0 and ws((1 << 31) // 384 - 1, 384, 40, CUS) > 0
    assert ws((1 << 31) // 64, 16, 40, CUS) == 0 and ws((1 << 31) // 64 - 1, 16, 40, CUS) > 0
    assert ws(1 << 40, 16, 8, CUS) == 0
    shapes = [(rows, I, L, cus) for rows in (1, 127, 128, 129, 8192, 8193, 102400) for I in (16, 96, 256, 384)
              for L in (4, 32, 33, 40, 48, 64) for cus in (1, 8, 256, 304)]
    first = [ws(*s) for s in shapes]
    for s, got in zip(shapes, first):
        assert got == _plan_py(s[0], s[1], s[2], s[2], s[3])["bytes"], s
        assert got % 16 == 0
    assert [ws(*s) for s in reversed(shapes)] == first[::-1]


def test_plan_hook_agrees_with_the_python_rule(labenv):
    labenv.lib()
    P = _lib.out_layer_lib()
    assert _lib.is_lab()
    got = _plan(P, 800 * 128, 256, 40, 40)
    assert (got["rt"], got["nt"], got["nkb"], got["grid"], got["runs"], got["run_rows"]) == (128, 64, 16, 800, 256, 400)
    for rows in (1, RT - 1, RT, RT + 1, 8 * RT + 1, 8192, 8193, 102400):
        for I in (16, 96, 256, 384, 100):
            for L, O in [(4, 4), (12, 12), (24, 24), (40, 40), (43, 46), (53, 56), (64, 64), (40, 39), (65, 65)]:
                for cus in (1, 8, 256, 304):
                    assert _plan(P, rows, I, L, O, cus) == _plan_py(rows, I, L, O, cus), (rows, I, L, O, cus)
    assert _plan(P, 8193, 384, 40, 40, 1)["runs"] == 2 and _plan(P, 8192, 384, 40, 40, 1)["runs"] == 1
    assert _plan(P, 8193, 96, 40, 40, 1)["run_rows"] == 4112 and _plan(P, 102400, 96, 40, 40)["runs"] == 493
    assert max(_plan(P, rows, 96, 40, 40, 1)["run_rows"] for rows in (8193, 102400, 1 << 22)) == CHAIN


def test_bad_arguments_are_refused_before_any_launch():
    """NULL, a misaligned workspace, one table without the other, a table entry out of range or a group in two pieces ->
    TK_ERR_BAD_ARG; a workspace one byte short -> TK_ERR_WORKSPACE; sizes outside the rule -> TK_ERR_UNSUPPORTED:
    decided on the host (the pointers are never dereferenced: no GPU in this test)."""
    P = _lib.out_layer_lib()
    shape = (33, 96, 43, 46)
    need = P.tk_out_layer_workspace_bytes(33, 96, 43, CUS)
    assert need > 0
    ptrs = {n: ctypes.c_void_p(4096 * (i + 1)) for i, n in enumerate(("x", "w", "b", "y", "dy", "dx", "dw", "db", "ws"))}
    null = ctypes.c_void_p(0)
    src, group = layers.out_layer_tables(40, (1, 1, 0, 0))
    ints = lambda v: (ctypes.c_int * len(v))(*v)    # noqa: E731

    def fwd(src=src, group=group, wsb=need, shape=shape, **over):
        p = dict(ptrs, **over)
        return P.tk_out_layer_forward_dev(p["x"], p["w"], p["b"], src and ints(src), group and ints(group), *shape, 5.0,
                                          CUS, p["y"], p["ws"], wsb, None)

    def bwd(src=src, group=group, wsb=need, shape=shape, **over):
        p = dict(ptrs, **over)
        return P.tk_out_layer_backward_dev(p["dy"], p["y"], p["x"], p["w"], src and ints(src), group and ints(group),
                                           *shape, 5.0, CUS, p["dx"], p["dw"], p["db"], p["ws"], wsb, None)

    for call, names in ((fwd, ("x", "w", "b", "y", "ws")), (bwd, ("dy", "y", "x", "w", "dw", "db", "ws"))):
        for name in names:
            assert call(**{name: null}) == BAD_ARG, name
        assert call(ws=ctypes.c_void_p(4096 + 4)) == BAD_ARG
        assert call(wsb=need - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
        assert call(shape=(0, 96, 43, 46)) == UNSUPPORTED and call(shape=(33, 100, 43, 46)) == UNSUPPORTED
        assert call(shape=(33, 96, 65, 65)) == UNSUPPORTED and call(shape=(33, 96, 43, 42)) == UNSUPPORTED
        assert call(shape=(33, 96, 43, 65)) == UNSUPPORTED
        assert call(src=None) == BAD_ARG and call(group=None) == BAD_ARG
        assert call(src=None, group=None) == BAD_ARG            # the plain layer has O = L
        assert call(src=src[:-1] + [43]) == BAD_ARG and call(src=[-1] + src[1:]) == BAD_ARG
        assert call(group=group[:-1] + [-2]) == BAD_ARG and call(group=group[:-1] + [64]) == BAD_ARG
        assert call(group=group[:40] + [0, 1, 0, 1, 2, 3]) == BAD_ARG


@pytest.mark.parametrize("can_nmods", [(1, 1, 0, 0), (0, 0, 0, 0), (2, 0, 1, 0), (3, 3, 3, 3)])
def test_cat_mod_tables_match_the_layers_indices(can_nmods):
    layer = layers.GlobalNormFlipFlopCatMod(32, can_nmods)
    nt = layer.ntrans_states
    src, group = layer.out_src, layer.out_group
    assert (src, group) == layers.out_layer_tables(nt, can_nmods)
    assert len(src) == len(group) == layer.nout and max(src) == layer.size - 1
    assert src[:nt] == list(range(nt)) and group[:nt] == [-1] * nt
    off = layer.can_mods_offsets
    for k in range(layer.ncan_base):
        lo, hi = nt + int(off[k]), nt + int(off[k + 1])
        assert group[lo:hi] == [k] * (hi - lo)
        assert src[lo:hi] == [nt + int(i) for i in layer.can_indices[k]]
        assert src[lo] == nt        # the single canonical column opens every group
    # the tables reproduce the layer on the host: gather, then tanh or log_softmax by group
    x = torch.randn(3, 2, 32)
    z = layer.linear(x)
    want = layer(x)
    got = torch.empty_like(want)
    for o, (s, g) in enumerate(zip(src, group)):
        if g < 0:
            got[..., o] = 5.0 * torch.tanh(z[..., s])
        else:
            members = [src[q] for q in range(len(src)) if group[q] == g]
            got[..., o] = z[..., s] - torch.logsumexp(z[..., members], dim=-1)
    assert torch.allclose(got, want, atol=1e-6)
    assert list(layer.state_dict()) == ["linear.weight", "linear.bias"]


def test_without_the_switch_or_on_the_cpu_the_library_is_never_touched(monkeypatch):
    def boom():
        raise AssertionError("the output layer's library was asked for")

    monkeypatch.setattr(_lib, "out_layer_lib", boom)
    plain, cat = layers.GlobalNormFlipFlop(32, 4), layers.GlobalNormFlipFlopCatMod(32, (1, 1, 0, 0))
    x = torch.randn(5, 3, 32, requires_grad=True)
    calls = dict(layers.out_layer_calls)
    for flag in (True, False):
        monkeypatch.setattr(layers, "USE_HIP_OUT_LAYER", flag)
        for layer in (plain, cat):
            assert not layers.hip_out_layer_takes(layer, x)
            layer(x).sum().backward()
    y = plain(x)
    assert torch.equal(y, plain.scale * torch.tanh(plain.linear(x)))
    assert y.shape == (5, 3, 40) and cat(x).shape == (5, 3, cat.nout) and cat.nout == 46
    assert layers.out_layer_calls == calls
    # with the switch off a CUDA tensor is not asked about either (a meta tensor stands in: no GPU here)
    monkeypatch.setattr(layers, "USE_HIP_OUT_LAYER", False)

    class _Cuda:
        is_cuda, dtype, shape = True, torch.float32, (5, 3, 32)

        def dim(self):
            return 3

    assert not layers.hip_out_layer_takes(plain, _Cuda())
    assert np.array_equal(cat.can_mods_offsets, [0, 2, 4, 5, 6])

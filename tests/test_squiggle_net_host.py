"""The squiggle predictor network without a GPU: the C ABI of include/taiyaki_amd_squiggle_net.h as far as the host
answers it (exports, signatures, the supported set, the workspace size), the layers and the model of
`models.squiggle_predictor` on the CPU against the reference's own answers (tests/golden/squiggle_net.npz, written by
make_golden_squiggle_net.py from the genuine taiyaki.layers), and the table of bin/predict_squiggle.py."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.golden import make_golden_squiggle_net as G


@pytest.fixture(scope="module")
def gold():
    return load_golden("squiggle_net.npz")


def _dynsyms(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def _lab_lib():
    from taiyaki_amd import _lib
    return _lib._load(os.path.join(_lib.CSRC, _lib.SQUIGGLE_NET_LAB_LIBNAME),
                      dict(_lib.SQUIGGLE_NET_SIGNATURES, **_lib.SQUIGGLE_NET_LAB_SIGNATURES))


def test_both_libraries_export_the_header_and_nothing_else():
    from taiyaki_amd import _lib
    declared = set(re.findall(r"\b(tk_\w+)\s*\(", _lib._blank_comments(open(_lib.SQUIGGLE_NET_HEADER).read())))
    release = {n for n in declared if not n.startswith("tk_lab_")}
    assert release == set(_lib.SQUIGGLE_NET_SIGNATURES) == {
        "tk_squiggle_net_supported", "tk_squiggle_net_workspace_bytes", "tk_squiggle_net_forward_dev",
        "tk_squiggle_net_backward_dev"}
    assert declared - release == set(_lib.SQUIGGLE_NET_LAB_SIGNATURES) == {"tk_lab_squiggle_net_plan"}
    assert _dynsyms(os.path.join(_lib.CSRC, _lib.SQUIGGLE_NET_LIBNAME)) == release
    assert _dynsyms(os.path.join(_lib.CSRC, _lib.SQUIGGLE_NET_LAB_LIBNAME)) == declared


def test_signatures_parse_from_the_header():
    from taiyaki_amd import _lib
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    pp = ctypes.POINTER(vp)
    sigs = _lib.SQUIGGLE_NET_SIGNATURES
    assert sigs["tk_squiggle_net_supported"] == (i, [sz, sz, sz])
    assert sigs["tk_squiggle_net_workspace_bytes"] == (sz, [sz, sz, sz, sz, sz, i])
    assert sigs["tk_squiggle_net_forward_dev"] == (i, [vp, pp, vp, sz, sz, sz, sz, sz, i, vp, vp, vp])
    assert sigs["tk_squiggle_net_backward_dev"] == (i, [vp, vp, vp, pp, vp, sz, sz, sz, sz, sz, i, vp, pp, vp, sz, vp])
    assert _lib.SQUIGGLE_NET_LAB_SIGNATURES["tk_lab_squiggle_net_plan"] == (i, [sz, sz, sz, sz, sz, i, vp])
    L = _lib.squiggle_net_lib()
    assert L.tk_squiggle_net_forward_dev.argtypes == sigs["tk_squiggle_net_forward_dev"][1]


def test_supported_is_what_the_header_names():
    from taiyaki_amd import _lib
    text = open(_lib.SQUIGGLE_NET_HEADER).read()
    m = re.search(r"tk_squiggle_net_supported: 1 for size ([\d, or]+), winlen ([\d or]+) and depth (\d+) \.\.\. (\d+); 0 otherwise",
                  text)
    sizes, wins = [int(v) for v in re.findall(r"\d+", m.group(1))], [int(v) for v in re.findall(r"\d+", m.group(2))]
    depths = range(int(m.group(3)), int(m.group(4)) + 1)
    assert set(sizes) >= {16, 32, 64} and set(wins) >= {5, 9} and set(depths) >= set(range(1, 9))
    L = _lib.squiggle_net_lib()
    for size in (8, 16, 24, 32, 48, 64, 128):
        for win in (3, 5, 7, 8, 9, 11):
            for depth in range(0, 11):
                want = int(size in sizes and win in wins and depth in depths)
                assert L.tk_squiggle_net_supported(size, depth, win) == want, (size, depth, win)
    for size, depth, win in ((48, 4, 9), (32, 4, 8), (32, 0, 9), (32, 9, 9)):
        assert L.tk_squiggle_net_supported(size, depth, win) == 0


def test_workspace_bytes_is_a_function_of_its_arguments():
    from taiyaki_amd import _lib
    L, lab = _lib.squiggle_net_lib(), _lab_lib()
    assert L.tk_squiggle_net_workspace_bytes(0, 100, 32, 4, 9, 256) == 0
    assert L.tk_squiggle_net_workspace_bytes(300, 0, 32, 4, 9, 256) == 0
    for shape in ((48, 4, 9), (32, 4, 8), (32, 0, 9), (32, 9, 9)):
        assert L.tk_squiggle_net_workspace_bytes(300, 100, *shape, 256) == 0
    out = (ctypes.c_size_t * 8)()
    for P, N, size, depth, win, cus in ((300, 100, 32, 4, 9, 256), (1, 1, 16, 1, 5, 256), (1000, 64, 64, 8, 9, 304),
                                        (53, 3, 32, 4, 9, 8)):
        a = L.tk_squiggle_net_workspace_bytes(P, N, size, depth, win, cus)
        assert a > 0 and a == L.tk_squiggle_net_workspace_bytes(P, N, size, depth, win, cus)
        assert a == lab.tk_squiggle_net_workspace_bytes(P, N, size, depth, win, cus)
        assert lab.tk_lab_squiggle_net_plan(P, N, size, depth, win, cus, out) == 1
        tile, halo_f, halo_b, tiles, fgrid, bgrid, slab, nbytes = list(out)
        radius = (depth + 2) * (win // 2)
        assert halo_f == halo_b == radius and tile >= 1 and tiles == -(-P // tile) and fgrid == tiles * N
        assert 1 <= bgrid <= min(fgrid, 2 * cus) and nbytes == a == bgrid * slab * 4
        # a partial result holds every gradient once
        assert slab >= 2 * (3 * size * win) + depth * size * size * win + (depth + 1) * size + 3
    assert lab.tk_lab_squiggle_net_plan(300, 100, 48, 4, 9, 256, out) == 0


def test_null_and_misaligned_arguments_are_refused_before_any_launch():
    """(host-side checks: nothing here touches a device)"""
    from taiyaki_amd import _lib
    L = _lib.squiggle_net_lib()
    bad_arg, unsupported = _lib.DEFINES["TK_ERR_BAD_ARG"], _lib.DEFINES["TK_ERR_UNSUPPORTED"]
    vp = ctypes.c_void_p
    params = (vp * 12)(*[4096 + 64 * i for i in range(12)])
    assert L.tk_squiggle_net_forward_dev(vp(0), params, vp(0), 10, 1, 32, 4, 9, 256, vp(0), vp(4096), vp(0)) == bad_arg
    assert L.tk_squiggle_net_forward_dev(vp(4096), None, vp(0), 10, 1, 32, 4, 9, 256, vp(0), vp(4096), vp(0)) == bad_arg
    params[5] = None
    assert L.tk_squiggle_net_forward_dev(vp(4096), params, vp(0), 10, 1, 32, 4, 9, 256, vp(0), vp(4096), vp(0)) == bad_arg
    params[5] = 8192
    assert L.tk_squiggle_net_forward_dev(vp(4096), params, vp(0), 10, 1, 32, 4, 9, 256, vp(4100), vp(4096), vp(0)) == bad_arg
    assert L.tk_squiggle_net_forward_dev(vp(4098), params, vp(0), 10, 1, 32, 4, 9, 256, vp(0), vp(4096), vp(0)) == bad_arg
    assert L.tk_squiggle_net_forward_dev(vp(4096), params, vp(0), 10, 1, 48, 4, 9, 256, vp(0), vp(4096), vp(0)) == unsupported
    assert L.tk_squiggle_net_backward_dev(vp(4096), vp(4096), vp(4096), params, vp(0), 10, 1, 32, 4, 9, 256, vp(0), params,
                                          vp(4096), 0, vp(0)) == _lib.DEFINES["TK_ERR_WORKSPACE"]
    assert L.tk_squiggle_net_backward_dev(vp(4096), vp(4096), vp(4096), params, vp(0), 10, 1, 32, 4, 9, 256, vp(0), None,
                                          vp(4096), 1 << 30, vp(0)) == bad_arg
    assert L.tk_squiggle_net_backward_dev(vp(4096), vp(4096), vp(4096), params, vp(0), 10, 1, 32, 4, 9, 256, vp(0), params,
                                          vp(4104), 1 << 30, vp(0)) == bad_arg


def test_residual_linear_and_the_predictor_have_the_reference_names_and_shapes():
    from taiyaki_amd import layers, models
    x = torch.randn(5, 2, 3)
    assert layers.linear(x) is x
    res = layers.Residual(layers.Convolution(3, 3, 5, fun=layers.linear))
    assert [n for n, _ in res.named_parameters()] == ["layer.conv.weight", "layer.conv.bias"]
    assert torch.equal(res(x), x + res.layer(x))
    net = models.squiggle_predictor()
    assert isinstance(net, layers.SquigglePredictor) and isinstance(net, layers.Serial) and net.fused_shape() == (32, 4, 9)
    want = {"0.conv.weight": (32, 3, 9), "0.conv.bias": (32,), "5.conv.weight": (3, 32, 9), "5.conv.bias": (3,)}
    for k in range(1, 5):
        want["%d.layer.conv.weight" % k], want["%d.layer.conv.bias" % k] = (32, 32, 9), (32,)
    assert {n: tuple(p.shape) for n, p in net.named_parameters()} == want
    assert [type(m) for m in net] == [layers.Convolution] + [layers.Residual] * 4 + [layers.Convolution]
    assert net[0].activation is torch.tanh and net[1].layer.activation is torch.tanh and net[5].activation is layers.linear
    assert len({id(m) for m in net}) == 6        # (depth layers of their own, not one repeated)
    small = models.squiggle_predictor(size=16, depth=1, winlen=5)
    assert small.fused_shape() == (16, 1, 5) and small(x).shape == (5, 2, 3)
    # what is not the pattern runs per layer
    assert layers.SquigglePredictor([layers.Convolution(3, 16, 5), layers.Convolution(16, 3, 5, fun=layers.linear)]).fused_shape() is None
    odd = models.squiggle_predictor(size=16, depth=2, winlen=5)
    odd[2] = layers.Residual(layers.Convolution(16, 16, 5, fun=layers.swish))
    assert odd.fused_shape() is None


def _rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("case", G.CASES, ids=G.case_name)
def test_cpu_model_reproduces_the_reference(gold, case):
    """Per layer on the CPU: in float32 as close to the reference's float64 numbers as the reference's own float32
    numbers are (the allowance below), and the float64 copy of the model the float64 numbers to 1e-12."""
    from taiyaki_amd import models
    size, depth, winlen, P, N = case
    d = G.load_case(gold, case)
    for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        net = models.squiggle_predictor(size, depth, winlen).to(dtype)
        net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in d["params"].items()})
        x = torch.from_numpy(d["x"]).to(dtype).requires_grad_(True)
        y = net(x)
        y.backward(torch.from_numpy(d["dy"]).to(dtype))
        got = {"y": y.detach().numpy(), "dx": x.grad.numpy()}
        got.update({k: p.grad.numpy() for k, p in net.named_parameters()})
        want = {"y": d["f64"]["y"], "dx": d["f64"]["dx"], **d["f64"]["grad"]}
        ref32 = {"y": d["f32"]["y"], "dx": d["f32"]["dx"], **d["f32"]["grad"]}
        assert set(got) == set(want)
        for k in want:
            if prec == "f64":
                # (the stored float64 weight gradients are good to 1e-10: make_golden_squiggle_net.py)
                assert _rel(got[k], want[k]) < (1e-9 if k.endswith("weight") else 1e-12), k
            else:
                # the allowance of the GPU tests (tests/test_squiggle_net.py): four times the reference's own float32
                # distance from float64, floor 1e-6 = float32 epsilon x sqrt(576) -- this path sums in another order
                # (unfold + GEMM) than the reference's conv1d, so it is as far from float64, not equal to it
                own = _rel(ref32[k], want[k])
                assert _rel(got[k], want[k]) <= max(4 * own, 1e-6), (k, own)


def test_lengths_zero_every_layer_beyond_a_column_and_match_the_column_alone(gold):
    """The per-layer path with lengths, float64 on the CPU: each column's rows are what the column gives alone."""
    from taiyaki_amd import models
    case = G.CASES[0]
    d = G.load_case(gold, case)
    net = models.squiggle_predictor(*case[:3]).double()
    net.load_state_dict({k: torch.from_numpy(v).double() for k, v in d["params"].items()})
    x = torch.from_numpy(d["x"]).double()
    lens = [53, 0, 17]
    with torch.no_grad():
        y = net(x, lengths=lens)
        for n, m in enumerate(lens):
            assert torch.equal(y[m:, n], torch.zeros(53 - m, 3, dtype=torch.float64))
            if m:
                alone = net(x[:m, n:n + 1].contiguous())
                assert float((y[:m, n] - alone[:, 0]).abs().max()) < 1e-13
    with pytest.raises(ValueError, match="lengths"):
        net(x, lengths=[54, 0, 17])
    with pytest.raises(ValueError, match="lengths"):
        net(x, lengths=[53, 17])


def test_write_predicted_squiggle_is_the_reference_table(gold):
    from taiyaki_amd import squiggle_match as sm
    seq = bytes(gold["table/seq"]).decode()
    y = G.load_case(gold, G.CASES[0])["f32"]["y"][:, 0]
    fh = io.StringIO()
    sm.write_predicted_squiggle(fh, seq, y)
    assert fh.getvalue().encode() == bytes(gold["table/text"])
    fh = io.StringIO()
    sm.write_predicted_squiggle(fh, seq.encode(), y.astype(np.float64))
    assert fh.getvalue().encode() == bytes(gold["table/text"])
    assert fh.getvalue().startswith("base\tcurrent\tsd\tdwell\n") and fh.getvalue().count("\n") == len(seq) + 1


def test_predict_squiggle_batches_sequences_as_padded_columns(gold):
    """(on the CPU the model runs per layer: the batching, the lengths and the return values are the same code)"""
    from taiyaki_amd import models, squiggle_match as sm
    torch.manual_seed(3)
    net = models.squiggle_predictor(16, 2, 5).double()
    seqs = ["ACGTTGCA" * 3, "A", "GATTACA", b"CCGT"]
    got = sm.predict_squiggle(net, seqs)
    assert [g.shape for g in got] == [(24, 3), (1, 3), (7, 3), (4, 3)]
    for s, g in zip(seqs, got):
        with torch.no_grad():
            alone = net(torch.from_numpy(sm.embed_sequence(s)[:, None]).double())[:, 0].numpy()
        assert g.dtype == np.float32 and np.abs(alone - g).max() < 1e-6
    assert sm.predict_squiggle(net, []) == []

"""The squiggle predictor network as one fused HIP operator (layers.SquiggleNet, csrc/squiggle_net.hip) on the GPU:
against float64 (the reference's own answers in tests/golden/squiggle_net.npz and a restatement written here with
torch.nn.functional), column by column bit for bit, with lengths, twice over a poisoned workspace, beside the per-layer
path, through the squiggle-match loss, through `predict_squiggle` and captured into a graph.

Every shape comes from the lab build's `tk_lab_squiggle_net_plan`.

ALLOWANCE (every accuracy check here): errors are taken relative to the result's largest entry; the operator may be
four times as far from float64 as the float32 per-layer path (this project's layers in float32 on the CPU, or the
reference's float32 numbers of the fixture) is on the same inputs, with a floor of 1e-6 = float32 epsilon (1.2e-7) x
sqrt(K) for K = size x winlen <= 576 products per sum, rounded down.  It is computed from the reference side only.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import load_golden
from tests.golden import make_golden_squiggle_net as G
from tests.golden import squiggle_cases as C

pytestmark = pytest.mark.gpu
FLOOR = 1e-6
SHAPES = [(s, w, d) for s in (16, 32, 64) for w in (5, 9) for d in (1, 4)] + [(32, 9, 8)]


@pytest.fixture(scope="module")
def gold():
    return load_golden("squiggle_net.npz")


@pytest.fixture(autouse=True)
def every_built_size(monkeypatch):
    """The model keeps size 64 off its kernels (layers.SQUIGGLE_NET_64_MAX_ROWS: they measured slower than the per-layer
    path); here that limit is lifted, so that every built kernel is run.  The rule as shipped has a test of its own."""
    from taiyaki_amd import layers
    monkeypatch.setattr(layers, "SQUIGGLE_NET_64_MAX_ROWS", None)


def plan(P, N, size, depth, winlen, dev):
    """tile, radius, tiles, backward grid of the launch at a shape, from the lab build"""
    from taiyaki_amd import _lib, layers
    lab = _lib._load(os.path.join(_lib.CSRC, _lib.SQUIGGLE_NET_LAB_LIBNAME),
                     dict(_lib.SQUIGGLE_NET_SIGNATURES, **_lib.SQUIGGLE_NET_LAB_SIGNATURES))
    out = (ctypes.c_size_t * 8)()
    assert lab.tk_lab_squiggle_net_plan(P, N, size, depth, winlen, layers._cu_count(dev), out) == 1
    assert out[1] == out[2] == (depth + 2) * (winlen // 2)
    return dict(tile=int(out[0]), radius=int(out[1]), tiles=int(out[3]), bwd_grid=int(out[5]), bytes=int(out[7]))


def make_net(size, depth, winlen, state, dev, dtype=torch.float32):
    from taiyaki_amd import models
    net = models.squiggle_predictor(size, depth, winlen).to(dtype)
    net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in state.items()})
    return net.to(dev)


def run(net, x, dy, lengths=None, want_dx=True):
    """y, dx, {name: gradient} (numpy) of one forward + backward, and the tensors the operator saved (or None)"""
    net.zero_grad()
    dev = next(net.parameters()).device
    xt = torch.as_tensor(x).to(dev).requires_grad_(want_dx)
    y = net(xt, lengths=lengths)
    saved = y.grad_fn.saved_tensors[1].clone() if type(y.grad_fn).__name__.startswith("SquiggleNetBackward") else None
    y.backward(torch.as_tensor(dy).to(dev))
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}
    return y.detach().cpu().numpy(), (xt.grad.cpu().numpy() if want_dx else None), grads, saved


def ref64(state, depth, x, dy):
    """The network restated in float64 with torch.nn.functional on the CPU: y, dx, {name: gradient}"""
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in state.items()}
    xt = torch.from_numpy(np.asarray(x)).double().requires_grad_(True)

    def conv(a, name):
        w = p[name + "weight"]
        return F.conv1d(a, w, p[name + "bias"], padding=w.shape[2] // 2)

    a = torch.tanh(conv(xt.permute(1, 2, 0), "0.conv."))
    for k in range(1, depth + 1):
        a = a + torch.tanh(conv(a, "%d.layer.conv." % k))
    y = conv(a, "%d.conv." % (depth + 1)).permute(2, 0, 1)
    y.backward(torch.from_numpy(np.asarray(dy)).double())
    return y.detach().numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()}


def rel(a, b):
    scale = np.abs(b).max()
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / (scale if scale > 0 else 1.0))


def flat(y, dx, grads):
    return dict(grads, y=y, dx=dx)


def check_against(got, want64, ref32, what, factor=1):
    """`got` within the ALLOWANCE of want64, the allowance taken from ref32 (the float32 reference side)"""
    worst = {}
    for k in want64:
        allow = factor * max(4 * rel(ref32[k], want64[k]), FLOOR)
        err = rel(got[k], want64[k])
        worst[k] = (err, allow)
        print("%s %-20s error %.3g allowance %.3g" % (what, k, err, allow))
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, (what, bad)


def launches():
    from taiyaki_amd import layers
    return dict(layers.SQUIGGLE_NET_LAUNCHES)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=G.case_name)
def test_operator_matches_the_reference_fixture(gold, gpu_device, case):
    size, depth, winlen, P, N = case
    d = G.load_case(gold, case)
    net = make_net(size, depth, winlen, d["params"], gpu_device)
    before = launches()
    y, dx, grads, saved = run(net, d["x"], d["dy"])
    assert launches() == {"forward": before["forward"] + 1, "backward": before["backward"] + 1} and saved is not None
    check_against(flat(y, dx, grads), flat(d["f64"]["y"], d["f64"]["dx"], d["f64"]["grad"]),
                  flat(d["f32"]["y"], d["f32"]["dx"], d["f32"]["grad"]), G.case_name(case))
    want = ref64(d["params"], depth, d["x"], d["dy"])       # (the restatement is the fixture's float64 model)
    for k, v in flat(*want).items():
        assert rel(v, flat(d["f64"]["y"], d["f64"]["dx"], d["f64"]["grad"])[k]) < 1e-9, k


@pytest.mark.parametrize("size,winlen,depth", SHAPES)
def test_operator_matches_float64_at_every_tile_edge(gpu_device, size, winlen, depth):
    """P on both sides of every size at which a row's window, the receptive radius or the tile changes what is read"""
    tile, radius = (plan(1, 1, size, depth, winlen, gpu_device)[k] for k in ("tile", "radius"))
    lengths = sorted({1, 2, winlen // 2, winlen // 2 + 1, radius, radius + 1, tile - 1, tile, tile + 1, 2 * tile + 1})
    _, _, state = G.make_inputs((size, depth, winlen, 1, 1), 100)
    net = make_net(size, depth, winlen, state, gpu_device)
    cpu32 = make_net(size, depth, winlen, state, torch.device("cpu"))
    for P in lengths:
        for N in (1, 3):
            x, dy, _ = G.make_inputs((size, depth, winlen, P, N), 200 + P)
            assert plan(P, N, size, depth, winlen, gpu_device)["tiles"] == -(-P // tile)
            before = launches()["forward"]
            got = flat(*run(net, x, dy)[:3])
            assert launches()["forward"] == before + 1
            check_against(got, flat(*ref64(state, depth, x, dy)), flat(*run(cpu32, x, dy)[:3]),
                          "P %d N %d" % (P, N))


def test_a_row_depends_on_its_own_column_only(gpu_device):
    """Bit for bit: a column in a batch with lengths is that column run alone at P = its length, whatever N and P are,
    and everything at and beyond a length is +0 (y and the saved rows)."""
    size, depth, winlen = 32, 4, 9
    tile, radius = (plan(1, 1, size, depth, winlen, gpu_device)[k] for k in ("tile", "radius"))
    P = 2 * tile + 5
    lens = [P, 0, 1, tile + 1, radius]
    x, dy, state = G.make_inputs((size, depth, winlen, P, 5), 300)
    net = make_net(size, depth, winlen, state, gpu_device)
    y, _, _, saved = run(net, x, dy, lengths=lens)
    saved = saved.cpu().numpy()
    assert saved.shape == (depth + 1, P, 5, size)
    for n, m in enumerate(lens):
        assert not bits(y[m:, n]).any() and not bits(saved[:, m:, n]).any()        # +0, not -0
        if m == 0:
            continue
        alone = np.ascontiguousarray(x[:m, n:n + 1])
        ya, _, _, sa = run(net, alone, dy[:m, n:n + 1])
        assert np.array_equal(bits(y[:m, n]), bits(ya[:, 0])), n
        assert np.array_equal(bits(saved[:, :m, n]), bits(sa.cpu().numpy()[:, :, 0])), n
        # the same column at P = len + 37 (rows beyond the length hold anything), with and without neighbours
        longer = np.concatenate([alone, np.full((37, 1, 3), 7.0, dtype=np.float32)])
        yl, _, _, sl = run(net, longer, np.ones((m + 37, 1, 3), dtype=np.float32), lengths=[m])
        assert np.array_equal(bits(yl[:m, 0]), bits(ya[:, 0])) and not bits(yl[m:]).any()
        assert np.array_equal(bits(sl.cpu().numpy()[:, :m, 0]), bits(sa.cpu().numpy()[:, :, 0]))
    with torch.no_grad():       # the form that saves nothing writes the same y
        yn = net(torch.from_numpy(x).to(gpu_device), lengths=lens)
    assert yn.grad_fn is None and np.array_equal(bits(yn.cpu().numpy()), bits(y))


def test_gradients_with_lengths_are_the_sums_over_the_columns(gpu_device):
    size, depth, winlen = 32, 4, 9
    tile, radius = (plan(1, 1, size, depth, winlen, gpu_device)[k] for k in ("tile", "radius"))
    P = 2 * tile + 5
    lens = [P, 0, 1, tile + 1, radius]
    x, dy, state = G.make_inputs((size, depth, winlen, P, 5), 300)
    net = make_net(size, depth, winlen, state, gpu_device)
    cpu32 = make_net(size, depth, winlen, state, torch.device("cpu"))
    poisoned = dy.copy()
    for n, m in enumerate(lens):
        poisoned[m:, n] = 1e30
    _, dx, grads, _ = run(net, x, poisoned, lengths=lens)
    total64 = {k: np.zeros(v.shape) for k, v in state.items()}
    total32 = {k: np.zeros(v.shape, dtype=np.float32) for k, v in state.items()}
    for n, m in enumerate(lens):
        assert not bits(dx[m:, n]).any()
        if m == 0:
            continue
        xa, da = np.ascontiguousarray(x[:m, n:n + 1]), np.ascontiguousarray(dy[:m, n:n + 1])
        _, dxa, ga, _ = run(net, xa, da)
        assert np.array_equal(bits(dx[:m, n]), bits(dxa[:, 0])), n
        _, _, g64 = ref64(state, depth, xa, da)
        _, _, g32, _ = run(cpu32, xa, da)
        for k in state:
            total64[k] += g64[k]
            total32[k] += g32[k]
    check_against(grads, total64, total32, "lengths")


def test_two_calls_give_the_same_bits_whatever_the_workspace_held(gpu_device):
    from taiyaki_amd import _lib
    size, depth, winlen = 32, 4, 9
    tile = plan(1, 1, size, depth, winlen, gpu_device)["tile"]
    P, N = 2 * tile + 1, 3
    x, dy, state = G.make_inputs((size, depth, winlen, P, N), 400)
    net = make_net(size, depth, winlen, state, gpu_device)
    ws = _lib.workspace(plan(P, N, size, depth, winlen, gpu_device)["bytes"], gpu_device, "squiggle_net")
    outs = []
    for fill in (255, 0):
        ws.fill_(fill)
        y, dx, grads, saved = run(net, x, dy)
        assert _lib.workspace(1, gpu_device, "squiggle_net") is ws       # (the call used this very buffer)
        outs.append(dict(flat(y, dx, grads), saved=saved.cpu().numpy()))
    for k in outs[0]:
        assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), k
    # several tiles per workgroup (a device of two CUs, as the plan sees it): the same sums in another order
    from taiyaki_amd import layers
    layers._CU_COUNT[gpu_device.index], keep = 1, layers._CU_COUNT[gpu_device.index]
    try:
        assert plan(P, N, size, depth, winlen, gpu_device)["bwd_grid"] == 2 < 3 * N
        ws.fill_(255)
        few = flat(*run(net, x, dy)[:3])
    finally:
        layers._CU_COUNT[gpu_device.index] = keep
    want = flat(*ref64(state, depth, x, dy))
    cpu32 = flat(*run(make_net(size, depth, winlen, state, torch.device("cpu")), x, dy)[:3])
    check_against(few, want, cpu32, "two workgroups")
    assert np.array_equal(bits(few["y"]), bits(outs[0]["y"])) and np.array_equal(bits(few["dx"]), bits(outs[0]["dx"]))


def test_switch_and_unsupported_shapes_take_the_per_layer_path(gpu_device, monkeypatch):
    from taiyaki_amd import layers
    size, depth, winlen, P, N = 32, 4, 9, 90, 3
    x, dy, state = G.make_inputs((size, depth, winlen, P, N), 500)
    net = make_net(size, depth, winlen, state, gpu_device)
    xt = torch.from_numpy(x).to(gpu_device)
    assert net.takes_operator(xt) and not net.takes_operator(xt.double()) and not net.takes_operator(xt.cpu())
    before = launches()
    fused = flat(*run(net, x, dy)[:3])
    assert launches()["forward"] == before["forward"] + 1
    monkeypatch.setattr(layers, "USE_HIP_SQUIGGLE_NET", False)
    assert not net.takes_operator(xt)
    before = launches()
    y, dx, grads, saved = run(net, x, dy)
    assert launches() == before and saved is None
    want = flat(*ref64(state, depth, x, dy))
    cpu32 = flat(*run(make_net(size, depth, winlen, state, torch.device("cpu")), x, dy)[:3])
    check_against(flat(y, dx, grads), want, cpu32, "per layer")
    for k in want:      # the two paths, each within the allowance of float64: within twice that of each other
        allow = 2 * max(4 * rel(cpu32[k], want[k]), FLOOR)
        assert rel(fused[k], np.asarray(flat(y, dx, grads)[k], dtype=np.float64)) <= allow, k
    monkeypatch.setattr(layers, "USE_HIP_SQUIGGLE_NET", True)
    for shape in ((48, 2, 9), (32, 2, 7)):      # not built: per layer, and right
        x, dy, state = G.make_inputs(shape + (40, 2), 600)
        odd = make_net(*shape, state, gpu_device)
        assert odd.fused_shape() == shape and not odd.takes_operator(torch.from_numpy(x).to(gpu_device))
        before = launches()
        got = flat(*run(odd, x, dy)[:3])
        assert launches() == before
        check_against(got, flat(*ref64(state, shape[1], x, dy)),
                      flat(*run(make_net(*shape, state, torch.device("cpu")), x, dy)[:3]), "shape %s" % (shape,))


def test_size_64_runs_per_layer_as_shipped(gpu_device, monkeypatch):
    from taiyaki_amd import layers
    monkeypatch.undo()      # (the module's autouse fixture lifted the limit)
    assert layers.SQUIGGLE_NET_64_MAX_ROWS == 0
    x, dy, state = G.make_inputs((64, 2, 9, 40, 2), 650)
    net = make_net(64, 2, 9, state, gpu_device)
    xt = torch.from_numpy(x).to(gpu_device)
    assert net.fused_shape() == (64, 2, 9) and not net.takes_operator(xt)
    before = launches()
    got = flat(*run(net, x, dy)[:3])
    assert launches() == before
    check_against(got, flat(*ref64(state, 2, x, dy)),
                  flat(*run(make_net(64, 2, 9, state, torch.device("cpu")), x, dy)[:3]), "size 64 as shipped")
    monkeypatch.setattr(layers, "SQUIGGLE_NET_64_MAX_ROWS", 80)
    assert net.takes_operator(xt) and not net.takes_operator(torch.cat([xt, xt[:1]]))


def test_the_trainers_chain_through_the_match_loss(gpu_device, monkeypatch):
    """train_squiggle.py:216-223 on the model: loss = squiggle_match_loss(model(emb), signal, siglen, back_prob), a
    weight per read, .sum() / siglen.sum(), .backward() -- against the same chain on the per-layer path.  The bound
    between the two chains' parameter gradients is the squiggle match's own: 5e-4 of the largest entry
    (tests/test_squiggle_match.py, GRAD_COL_TOL: the reference's float32 match gradient is 1.2e-4 from float64), since
    the two predictions differ in their last bits and the match gradient is what carries that difference."""
    from taiyaki_amd import layers, squiggle_match as sm
    case = C.from_fixture(load_golden("squiggle_small.npz"), "npos37_back03")
    npos, nbatch = case["params"].shape[:2]
    torch.manual_seed(0)
    from taiyaki_amd import models
    net = models.squiggle_predictor().to(gpu_device)
    rng = np.random.RandomState(3)
    emb = torch.from_numpy(np.stack([sm.embed_sequence(rng.randint(0, 4, npos), alphabet=None)
                                     for _ in range(nbatch)], axis=1)).to(gpu_device)
    signal = torch.from_numpy(case["signal"]).to(gpu_device)
    siglen = torch.from_numpy(case["siglen"].astype(np.int64)).to(gpu_device)
    weights = torch.linspace(0.5, 2.0, nbatch, device=gpu_device)

    def chain():
        net.zero_grad()
        pred = net(emb)
        loss = sm.squiggle_match_loss(pred, signal, siglen, case["back_prob"])
        ((loss * weights).sum() / float(siglen.sum())).backward()
        return loss.detach().cpu().numpy(), pred.detach().cpu().numpy(), \
            {k: p.grad.cpu().numpy().copy() for k, p in net.named_parameters()}

    before = launches()
    loss, pred, grads = chain()
    assert launches() == {"forward": before["forward"] + 1, "backward": before["backward"] + 1}
    np.testing.assert_allclose(loss, sm.squiggle_match_cost(pred, case["signal"], case["siglen"], case["back_prob"]),
                               rtol=1e-6)
    monkeypatch.setattr(layers, "USE_HIP_SQUIGGLE_NET", False)
    loss_ref, pred_ref, grads_ref = chain()
    assert launches()["forward"] == before["forward"] + 1
    assert rel(pred, pred_ref.astype(np.float64)) <= 2 * FLOOR
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-5)
    for k in grads:
        err = rel(grads[k], grads_ref[k].astype(np.float64))
        print("chain %-20s difference %.3g" % (k, err))
        assert err <= 5e-4, k


def test_predict_squiggle_is_one_launch_and_every_sequence_alone(gpu_device):
    from taiyaki_amd import models, squiggle_match as sm
    tile = plan(1, 1, 32, 4, 9, gpu_device)["tile"]
    torch.manual_seed(5)
    net = models.squiggle_predictor().to(gpu_device)
    rng = np.random.RandomState(11)
    seqs = ["".join("ACGT"[b] for b in rng.randint(0, 4, n)) for n in (1, 7, 300, tile + 1, 64)]
    before = launches()
    got = sm.predict_squiggle(net, seqs)
    assert launches() == {"forward": before["forward"] + 1, "backward": before["backward"]}
    for s, g in zip(seqs, got):
        assert g.shape == (len(s), 3) and g.dtype == np.float32
        with torch.no_grad():
            alone = net(torch.from_numpy(sm.embed_sequence(s)[:, None]).to(gpu_device))[:, 0].cpu().numpy()
        assert np.array_equal(bits(g), bits(alone)), len(s)


def test_forward_and_backward_replay_from_a_captured_graph(gpu_device):
    size, depth, winlen, P, N = 32, 4, 9, 150, 3
    x, dy, state = G.make_inputs((size, depth, winlen, P, N), 700)
    net = make_net(size, depth, winlen, state, gpu_device)
    eager = flat(*run(net, x, dy)[:3])
    xs = torch.from_numpy(x).to(gpu_device).requires_grad_(True)
    dys = torch.from_numpy(dy).to(gpu_device)
    params = list(net.parameters())
    stream = torch.cuda.Stream(gpu_device)
    stream.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(stream):
        for _ in range(2):      # (warm-up on the side stream, as torch asks before a capture)
            torch.autograd.grad(net(xs), [xs] + params, dys)
    torch.cuda.current_stream(gpu_device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = net(xs)
        outs = torch.autograd.grad(y, [xs] + params, dys)
    for _ in range(2):
        y.zero_()
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(gpu_device)
        got = dict({k: o for (k, _), o in zip(net.named_parameters(), outs[1:])}, y=y, dx=outs[0])
        for k, v in eager.items():
            assert np.array_equal(bits(got[k].detach().cpu().numpy()), bits(v)), k


def test_bad_arguments_raise_and_launch_nothing(gpu_device):
    from taiyaki_amd import _lib, layers
    size, depth, winlen, P, N = 16, 1, 5, 20, 2
    x, dy, state = G.make_inputs((size, depth, winlen, P, N), 800)
    net = make_net(size, depth, winlen, state, gpu_device)
    xt = torch.from_numpy(x).to(gpu_device)
    before = launches()
    with pytest.raises(ValueError, match="lengths"):
        net(xt, lengths=[P + 1, 3])
    assert launches() == before
    # straight at the C ABI: a misaligned `saved`, a host pointer is not the library's to tell, a null parameter
    L = _lib.squiggle_net_lib()
    params = [p.detach() for p in net.parameter_list()]
    y = torch.full((P, N, 3), 5.0, device=gpu_device)
    saved = torch.empty((depth + 1) * P * N * size + 4, device=gpu_device)
    args = (P, N, size, depth, winlen, layers._cu_count(gpu_device))
    bad = _lib.DEFINES["TK_ERR_BAD_ARG"]
    assert L.tk_squiggle_net_forward_dev(_lib.ptr(xt), layers._pointer_array(params), None, *args,
                                         ctypes.c_void_p(saved.data_ptr() + 4), _lib.ptr(y), _lib.stream_ptr()) == bad
    holes = layers._pointer_array(params)
    holes[3] = None
    assert L.tk_squiggle_net_forward_dev(_lib.ptr(xt), holes, None, *args, None, _lib.ptr(y), _lib.stream_ptr()) == bad
    assert L.tk_squiggle_net_forward_dev(None, layers._pointer_array(params), None, *args, None, _lib.ptr(y),
                                         _lib.stream_ptr()) == bad
    torch.cuda.synchronize(gpu_device)
    assert bool((y == 5.0).all())       # nothing ran
    # a CPU tensor never reaches the operator: the model runs it per layer on the CPU's own model, or raises on a mix
    with pytest.raises(RuntimeError):
        net(torch.from_numpy(x))
    assert launches() == before

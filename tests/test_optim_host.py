"""The optimiser step (include/taiyaki_amd_optim.h, csrc/optim.hip, taiyaki_amd/optim.py) as far as the host decides it:
the binding, the tile builder, the refusal of bad arguments before any launch, the one-cycle schedule against torch's, the
rolling quantile, the checkpoint layout and the trainers' switch.  No GPU: no device pointer is dereferenced."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, clipping, optim, train

OK, BAD_ARG, WORKSPACE = 0, 1, 3
D = _lib.OPTIM_DEFINES
TILE = D["TK_OPTIM_TILE"]
SIZES = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 0]


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _tiles(off):
    L = _lib.optim_lib()
    nseg = len(off) - 1
    n = L.tk_optim_tile_count(off.ctypes.data, nseg)
    out = np.zeros((n, D["TK_OPTIM_TILE_WORDS"]), dtype=np.uint32)
    assert L.tk_optim_tiles(off.ctypes.data, nseg, out.ctypes.data, n) == OK
    return out


def test_header_exports_and_binding_agree():
    names = {"tk_optim_tile_count", "tk_optim_tiles", "tk_optim_workspace_bytes", "tk_adamw_step_dev"}
    assert set(_lib.OPTIM_SIGNATURES) == names
    res, args = _lib.OPTIM_SIGNATURES["tk_adamw_step_dev"]
    assert res is ctypes.c_int and len(args) == 17
    assert args[:5] == [ctypes.c_void_p] * 5 and args[5:8] == [ctypes.c_size_t] * 3
    assert args[8:12] == [ctypes.c_void_p] * 4 and args[12] is ctypes.c_size_t
    assert args[13:16] == [ctypes.c_int] * 3 and args[16] is ctypes.c_void_p
    res, args = _lib.OPTIM_SIGNATURES["tk_optim_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_void_p, ctypes.c_size_t]
    L = _lib.optim_lib()            # every symbol resolves
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib.OPTIM_LIBNAME)], check=True,
                        capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if re.search(r" [TW] ", line)}
    assert exported == names, exported
    assert L.tk_optim_tile_count(None, 3) == 0
    # the hyper block: distinct words inside the block, the inputs in front
    words = [D[k] for k in ("TK_OPTIM_LR", "TK_OPTIM_BETA1", "TK_OPTIM_BETA2", "TK_OPTIM_EPS", "TK_OPTIM_WEIGHT_DECAY",
                            "TK_OPTIM_GRAD_SCALE", "TK_OPTIM_MAX_NORM", "TK_OPTIM_STEP", "TK_OPTIM_GRAD_NORM",
                            "TK_OPTIM_STEP_NOW")]
    assert words == list(range(10)) and D["TK_OPTIM_HYPER_WORDS"] >= 16 and TILE % 1024 == 0


@pytest.mark.parametrize("order", ["as listed", "shuffled", "reversed"])
def test_tiles_cover_every_element_once_in_order_inside_one_segment(order):
    sizes = list(SIZES)
    if order == "shuffled":
        np.random.RandomState(3).shuffle(sizes)
    elif order == "reversed":
        sizes = sizes[::-1]
    off = _offsets(sizes)
    tiles = _tiles(off)
    assert len(tiles) == sum(max(1, -(-s // TILE)) for s in sizes)
    at, seen = 0, np.zeros(len(sizes), dtype=np.int64)
    last_seg = -1
    for seg, first, count, local in tiles.tolist():
        assert seg in (last_seg, last_seg + 1), "segments in order, none left out"
        last_seg = seg
        assert first == at and local == first - off[seg], (seg, first, local)
        assert count <= TILE and first + count <= off[seg + 1], "a tile never crosses its segment's end"
        assert count > 0 or sizes[seg] == 0, "only an empty segment has an empty tile"
        assert count == TILE or first + count == off[seg + 1], "only a segment's last tile is short"
        at += count
        seen[seg] += count
    assert last_seg == len(sizes) - 1 and at == off[-1] and np.array_equal(seen, sizes)
    L = _lib.optim_lib()
    assert L.tk_optim_workspace_bytes(off.ctypes.data, len(sizes)) == 16 * len(tiles)


def test_tile_builder_refuses():
    L = _lib.optim_lib()
    good = _offsets([5, 0, 9])
    out = np.zeros((8, 4), dtype=np.uint32)
    n = L.tk_optim_tile_count(good.ctypes.data, 3)
    assert n == 3 and L.tk_optim_tiles(good.ctypes.data, 3, out.ctypes.data, 3) == OK
    assert L.tk_optim_tiles(good.ctypes.data, 3, out.ctypes.data, 2) == BAD_ARG       # capacity
    assert L.tk_optim_tiles(good.ctypes.data, 3, None, 3) == BAD_ARG
    assert L.tk_optim_tiles(None, 3, out.ctypes.data, 8) == BAD_ARG
    for bad in (np.array([0, 7, 6, 9], dtype=np.int64),             # decreasing
                np.array([1, 7, 8, 9], dtype=np.int64),             # does not start at 0
                np.array([0, 7, 8, (1 << 31) + 1], dtype=np.int64)):    # a total above 2^31
        assert L.tk_optim_tile_count(bad.ctypes.data, 3) == 0
        assert L.tk_optim_workspace_bytes(bad.ctypes.data, 3) == 0
        assert L.tk_optim_tiles(bad.ctypes.data, 3, out.ctypes.data, 8) == BAD_ARG
    assert L.tk_optim_tile_count(good.ctypes.data, 0) == 0 and L.tk_optim_workspace_bytes(good.ctypes.data, 0) == 0
    assert L.tk_optim_workspace_bytes(None, 3) == 0
    top = np.array([0, 1 << 31], dtype=np.int64)                    # 2^31 itself is inside the range
    assert L.tk_optim_tile_count(top.ctypes.data, 1) == (1 << 31) // TILE


def test_bad_arguments_are_refused_before_any_launch():
    """Decided on the host: the pointers are never dereferenced (no GPU in this test)."""
    L = _lib.optim_lib()
    names = ("grads", "exp_avg", "exp_avg_sq", "params", "tiles", "hyper", "thresh", "maxs", "ws")
    ptrs = {n: ctypes.c_void_p(4096 * (i + 1)) for i, n in enumerate(names)}
    null = ctypes.c_void_p(0)

    def call(ntiles=5, nseg=3, total=9000, wsb=16 * 5, cus=256, **over):
        p = dict(ptrs, **over)
        return L.tk_adamw_step_dev(p["grads"], p["exp_avg"], p["exp_avg_sq"], p["params"], p["tiles"], ntiles, nseg, total,
                                   p["hyper"], p["thresh"], p["maxs"], p["ws"], wsb, 1, 1, cus, None)

    for name in ("grads", "exp_avg", "exp_avg_sq", "params", "tiles", "hyper", "ws"):
        assert call(**{name: null}) == BAD_ARG, name
    assert call(nseg=0) == BAD_ARG and call(ntiles=0) == BAD_ARG and call(ntiles=2) == BAD_ARG
    assert call(ntiles=7, wsb=16 * 7) == BAD_ARG            # more tiles than nseg + total / TILE
    assert call(total=(1 << 31) + 1) == BAD_ARG and call(total=1 << 40) == BAD_ARG
    assert call(cus=0) == BAD_ARG and call(cus=-1) == BAD_ARG
    assert call(ws=ctypes.c_void_p(4096 + 8)) == BAD_ARG
    assert call(wsb=16 * 5 - 1) == WORKSPACE and call(wsb=0) == WORKSPACE


def _torch_schedule(cycle, total=1000):
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.AdamW([p], lr=4e-3, betas=(0.9, 0.999))
    kw = dict(base_momentum=0.85, max_momentum=0.9) if cycle else {}
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, 4e-3, total_steps=total, pct_start=0.2, div_factor=4e-3 / 1e-4,
                                                final_div_factor=1.0, cycle_momentum=cycle, **kw)
    out = []
    for i in range(total):
        out.append((opt.param_groups[0]["lr"], opt.param_groups[0]["betas"][0]))
        opt.step()
        if i + 1 < total:
            sched.step()
    return out


@pytest.mark.parametrize("cycle", [True, False])
def test_one_cycle_is_torchs_schedule(cycle):
    """lr_max 4e-3, warm-up from 1e-4 over 200 of 1000 iterations, down to 1e-4; momentum 0.85 <-> 0.9.  The reference here
    is torch's own scheduler on a CPU AdamW; two constructions of it agree exactly, so 1e-12 relative is the restatement's
    to meet."""
    want = _torch_schedule(cycle)
    assert want == _torch_schedule(cycle)
    sched = optim.OneCycle(4e-3, 1000, pct_start=0.2, div_factor=4e-3 / 1e-4, final_div_factor=1.0,
                           base_momentum=0.85 if cycle else None, max_momentum=0.9 if cycle else None)
    for i, (lr, b1) in enumerate(want):
        got_lr, got_b1 = sched.at(i)
        assert abs(got_lr - lr) <= 1e-12 * lr, (i, got_lr, lr)
        if cycle:
            assert abs(got_b1 - b1) <= 1e-12 * b1, (i, got_b1, b1)
        else:
            assert got_b1 is None and b1 == 0.9
    assert abs(want[0][0] - 1e-4) < 1e-15 and abs(want[199][0] - 4e-3) < 1e-15 and abs(want[999][0] - 1e-4) < 1e-15
    if cycle:
        assert abs(want[0][1] - 0.9) < 1e-15 and abs(want[199][1] - 0.85) < 1e-15


def test_rolling_quantile_is_np_quantile_over_the_window():
    rs = np.random.RandomState(11)
    xs = np.exp(rs.standard_normal(350))
    for frac, window, min_data in ((0.05, 100, 1), (0.5, 7, 3), (0.25, 1, 1)):
        rq = clipping.RollingQuantile(frac, window=window, min_data=min_data, default_to=-1.0)
        for i, x in enumerate(xs):
            held = xs[max(0, i + 1 - window):i + 1]
            got = rq.update(x)
            if len(held) < min_data:
                assert got == -1.0
            else:
                assert got == np.quantile(held, 1.0 - frac), (frac, window, i)
    first = clipping.RollingQuantile(0.05)
    assert first.update(3.0) == 3.0 and abs(first.update(1.0) - (0.05 * 1.0 + 0.95 * 3.0)) < 1e-12     # maths.py:110-113


class _FakeArena:
    """What FlatAdamW looks at before it touches the device."""

    def __init__(self, params, flat=None):
        self.params = params
        self.flat = flat if flat is not None else torch.zeros(sum(p.numel() for p in params))


def test_flat_adamw_refuses_what_the_kernels_cannot_update(monkeypatch):
    def boom():
        raise AssertionError("the optimiser's library was asked for")

    monkeypatch.setattr(_lib, "optim_lib", boom)
    p = torch.zeros(4, 3, requires_grad=True)
    before = p.clone()
    with pytest.raises(TypeError, match="no CPU fallback"):
        optim.FlatAdamW(_FakeArena([p]))
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(TypeError, match="amsgrad / maximize"):
            optim.FlatAdamW(_FakeArena([p]), **kw)

    class _Cuda:            # stands in for a device tensor: no GPU here
        is_cuda, device = True, "cuda:0"

        def __init__(self, dtype=torch.float32, contiguous=True):
            self.dtype, self._c = dtype, contiguous

        def is_contiguous(self):
            return self._c

        def numel(self):
            return 4

    flat = _Cuda()
    with pytest.raises(TypeError, match="float32"):
        optim.FlatAdamW(_FakeArena([_Cuda(), _Cuda(torch.float16)], flat))
    with pytest.raises(TypeError, match="not contiguous"):
        optim.FlatAdamW(_FakeArena([_Cuda(contiguous=False)], flat))
    with pytest.raises(TypeError, match="float64"):
        optim.FlatAdamW(_FakeArena([_Cuda()], _Cuda(torch.float64)))
    assert torch.equal(p, before)


def test_state_dict_keys_are_torchs():
    """The layout, checked without a device: FlatAdamW's accessors on an object assembled by hand."""
    params = [torch.randn(3, 2), torch.randn(5)]
    ref = torch.optim.AdamW([p.clone().requires_grad_(True) for p in params], lr=2e-3, betas=(0.8, 0.99), eps=1e-6,
                            weight_decay=0.1)
    for p in ref.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    ref.step()
    want = ref.state_dict()
    opt = optim.FlatAdamW.__new__(optim.FlatAdamW)
    opt.params, opt.nseg, opt.seg_off = params, 2, np.array([0, 6, 11], dtype=np.int64)
    opt.hyper = torch.zeros(D["TK_OPTIM_HYPER_WORDS"])
    opt.exp_avg, opt.exp_avg_sq = torch.zeros(11), torch.zeros(11)
    opt.defaults = dict(lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.0)
    opt.load_state_dict(want)
    got = opt.state_dict()
    assert set(got) == set(want) == {"state", "param_groups"}
    assert sorted(got["state"]) == sorted(want["state"]) == [0, 1]
    for i in (0, 1):
        assert set(got["state"][i]) == set(want["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(got["state"][i]["step"]) == 1.0 and got["state"][i]["step"].dtype == torch.float32
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(got["state"][i][k], want["state"][i][k])
    g, w = got["param_groups"][0], want["param_groups"][0]
    assert set(g) == set(w) and g["params"] == w["params"] == [0, 1]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (2e-3, (0.8, 0.99), 1e-6, 0.1)
    assert g["amsgrad"] is False and g["maximize"] is False
    # ... and torch's optimiser takes it back
    ref.load_state_dict(got)
    assert float(ref.state_dict()["state"][1]["step"]) == 1.0
    hyper = opt.hyper.numpy()
    assert hyper[D["TK_OPTIM_STEP"]] == 1.0 and hyper[D["TK_OPTIM_BETA1"]] == np.float32(0.8)
    assert hyper[D["TK_OPTIM_LR"]] == np.float32(2e-3) and hyper[D["TK_OPTIM_WEIGHT_DECAY"]] == np.float32(0.1)
    # param_groups is read-only: torch's idiom of writing group["lr"] must not pass silently
    with pytest.raises(TypeError):
        opt.param_groups[0]["lr"] = 1.0
    assert opt.param_groups[0]["lr"] == 2e-3 and len(opt.param_groups[0]["params"]) == 2
    # a step captured without a norm cannot follow a cap set later; with one (or before any capture) it can
    opt.with_norm, opt._captured_with_norm = False, False
    with pytest.raises(RuntimeError, match="captured without a norm"):
        opt.set_max_norm(5.0)
    assert not opt.with_norm and hyper[D["TK_OPTIM_MAX_NORM"]] == 0.0
    opt._captured_with_norm = None
    opt.set_max_norm(5.0)
    assert opt.with_norm and opt.hyper.numpy()[D["TK_OPTIM_MAX_NORM"]] == 5.0
    with pytest.raises(ValueError):
        opt.load_state_dict(dict(want, param_groups=[dict(w, params=[0])]))
    with pytest.raises(TypeError):
        opt.load_state_dict(dict(want, param_groups=[dict(w, amsgrad=True)]))


def test_on_the_cpu_the_trainer_is_as_before():
    from taiyaki_amd import models, parallel
    assert train.USE_HIP_OPTIM in (True, False)
    net = models.mLstm_flipflop(size=16, stride=5)
    for flag in (None, True, False):
        tr = train.Trainer(net, parallel.FlatGradArena(net), hip_optim=flag)
        assert tr.hip_optim is False and isinstance(tr.opt, torch.optim.AdamW) and tr.norm_cap is None
    with pytest.raises(ValueError, match="HIP optimiser"):
        train.Trainer(net, parallel.FlatGradArena(net), grad_norm_cap_fraction=0.05)
    with pytest.raises(RuntimeError, match="beta1 of its capture"):
        train._set_momentum(tr.opt, 0.85)
    arena = parallel.FlatGradArena(net)
    arena.flat.fill_(2.0)
    assert arena.finish(scale=0.5, defer=True) == 0.5 and float(arena.flat[0]) == 2.0
    assert arena.finish(scale=0.5) == 0.5 and float(arena.flat[0]) == 1.0

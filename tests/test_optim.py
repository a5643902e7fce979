"""The optimiser step on the GPU (include/taiyaki_amd_optim.h, csrc/optim.hip, taiyaki_amd/optim.py) against a float64
restatement of its eight steps.

The allowance is measured, not fixed (the rule tests/test_rnn_instantiations.py keeps for MIOpen): per tensor, the kernels'
largest error against float64 may be twice that of torch's float32 optimiser on the same inputs (`torch.optim.AdamW(
foreach=False)` on the CPU for one step; `AdamW(capturable=True)` + `DeviceClipper` on the GPU for runs of steps) plus one
float32 ulp of the tensor's largest entry.  Every comparison prints both errors (`optim-err ...`, pytest -s).

Measured on an MI355X (profiles/r47_optim.txt): see that file for the figures of the run this was written with."""
import copy
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, clipping, models, optim, parallel, train

pytestmark = pytest.mark.gpu

D = _lib.OPTIM_DEFINES
TILE = D["TK_OPTIM_TILE"]
# tests/test_optim_host.py's sizes in an order that puts ten of the seventeen segments at an odd offset and three of at least
# eight elements (4097, 63, 65) at a multiple of four: both access widths, whole and ragged tiles, a one-element and an
# empty segment
SIZES = [4097, 7, 63, 4096, 64, 255, 4095, 3, 65, 8, 257, 0, 256, 5, 2, 4, 1]
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
NSEG, TOTAL = len(SIZES), int(OFF[-1])
F32 = np.float32
HYPER = dict(lr=F32(4e-3), b1=F32(0.9), b2=F32(0.999), eps=F32(1e-6), wd=F32(0.01), scale=F32(0.5), step=F32(3.0))
INF = float("inf")


def test_the_layout_has_what_it_says():
    assert sorted(SIZES) == sorted([1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 0])
    assert int((OFF[:-1] % 2 == 1).sum()) >= 10
    assert {s for s, o in zip(SIZES, OFF) if o % 4 == 0 and s >= 8} >= {4097, 63, 65}


def _inputs(seed=0):
    rs = np.random.RandomState(seed)
    return dict(p=rs.standard_normal(TOTAL).astype(F32), g=rs.standard_normal(TOTAL).astype(F32),
                m=(0.1 * rs.standard_normal(TOTAL)).astype(F32), v=((0.1 * rs.standard_normal(TOTAL)) ** 2).astype(F32))


def _thresholds():
    th = np.full(NSEG, 0.4, dtype=F32)
    th[1::3] = INF              # no threshold yet
    th[5] = np.nan              # a diverged window: no clamp
    th[7] = -1.0                # negative: no clamp
    th[4] = 0.0                 # clamps everything to zero
    return th


def _segments(x):
    return [x[OFF[s]:OFF[s + 1]] for s in range(NSEG)]


def ref64(inp, h, thresh, max_norm, zero_grads):
    """The eight steps in float64 numpy.  `max_norm` None: no norm."""
    g = inp["g"].astype(np.float64) * float(h["scale"])
    maxs = np.zeros(NSEG)
    for s, seg in enumerate(_segments(g)):
        if seg.size:
            maxs[s] = np.nan if np.isnan(seg).any() else np.abs(seg).max()
        if thresh is not None and np.isfinite(thresh[s]) and thresh[s] >= 0:
            seg[:] = np.fmin(np.fmax(seg, -float(thresh[s])), float(thresh[s]))
    norm = np.sqrt((g * g).sum())
    if max_norm is not None and np.isfinite(max_norm):
        coef = float(max_norm) / (norm + 1e-6)
        g = g * (1.0 if coef > 1.0 else coef)
    lr, b1, b2, eps, wd = (float(h[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    t = float(h["step"]) + 1.0
    p = inp["p"].astype(np.float64) * (1.0 - lr * wd)
    m = inp["m"].astype(np.float64)
    m = m + (g - m) * (1.0 - b1)
    v = b2 * inp["v"].astype(np.float64) + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return dict(p=p, m=m, v=v, g=np.zeros_like(g) if zero_grads else g, maxs=maxs, norm=norm, step=t)


def torch32(inp, h, thresh, max_norm, zero_grads):
    """The same step as float32 library calls on the CPU: mul_, max |g|, clamp_, clip_grad_norm_, AdamW(foreach=False)."""
    g = torch.from_numpy(inp["g"].copy()) * float(h["scale"])
    maxs = np.zeros(NSEG, dtype=F32)
    for s, seg in enumerate(_segments(g)):
        if seg.numel():
            maxs[s] = float(seg.abs().max())
        if thresh is not None and np.isfinite(thresh[s]) and thresh[s] >= 0:
            seg.clamp_(min=-float(thresh[s]), max=float(thresh[s]))
    params = [torch.from_numpy(x.copy()).requires_grad_(True) for x in _segments(inp["p"])]
    for p, seg in zip(params, _segments(g)):
        p.grad = seg
    norm = np.nan
    if max_norm is not None and np.isfinite(max_norm):
        norm = float(torch.nn.utils.clip_grad_norm_(params, float(max_norm), foreach=False))
    elif max_norm is not None:      # +inf: no cap (clip_grad_norm_ would still multiply by its factor, NaN for a NaN norm)
        norm = float(torch.nn.utils.get_total_norm([p.grad for p in params], foreach=False))
    opt = torch.optim.AdamW(params, lr=float(h["lr"]), betas=(float(h["b1"]), float(h["b2"])), eps=float(h["eps"]),
                            weight_decay=float(h["wd"]), foreach=False)
    for p, m, v in zip(params, _segments(inp["m"]), _segments(inp["v"])):
        opt.state[p] = dict(step=torch.tensor(float(h["step"])), exp_avg=torch.from_numpy(m.copy()),
                            exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    cat = lambda xs: np.concatenate([x.detach().numpy().reshape(-1) for x in xs])     # noqa: E731
    return dict(p=cat(params), m=cat([opt.state[p]["exp_avg"] for p in params]),
                v=cat([opt.state[p]["exp_avg_sq"] for p in params]),
                g=np.zeros(TOTAL, dtype=F32) if zero_grads else g.numpy(), maxs=maxs, norm=norm,
                step=float(opt.state[params[0]]["step"]))


class Device:
    """The layout on the GPU: separately allocated parameters, flat g, m, v, the tables -- and one checked launch."""

    def __init__(self, dev):
        self.dev = dev
        self.L = _lib.optim_lib()
        self.ntiles = self.L.tk_optim_tile_count(OFF.ctypes.data, NSEG)
        tiles = np.zeros((self.ntiles, 4), dtype=np.uint32)
        assert self.L.tk_optim_tiles(OFF.ctypes.data, NSEG, tiles.ctypes.data, self.ntiles) == 0
        self.tiles = torch.from_numpy(tiles.view(np.int32)).to(dev)
        self.wsb = self.L.tk_optim_workspace_bytes(OFF.ctypes.data, NSEG)
        assert self.wsb == 16 * self.ntiles

    def run(self, inp, h, thresh, want_maxs, max_norm, zero_grads, cus=256, junk=0.0):
        dev = self.dev
        params = [torch.from_numpy(x.copy()).to(dev) for x in _segments(inp["p"])]
        ptrs = torch.tensor([p.data_ptr() for p in params], dtype=torch.int64, device=dev)
        g, m, v = (torch.from_numpy(inp[k].copy()).to(dev) for k in "gmv")
        hyper = np.full(D["TK_OPTIM_HYPER_WORDS"], junk, dtype=F32)
        for word, key in (("LR", "lr"), ("BETA1", "b1"), ("BETA2", "b2"), ("EPS", "eps"), ("WEIGHT_DECAY", "wd"),
                          ("GRAD_SCALE", "scale"), ("STEP", "step")):
            hyper[D["TK_OPTIM_" + word]] = h[key]
        hyper[D["TK_OPTIM_MAX_NORM"]] = INF if max_norm is None else max_norm
        hyper = torch.from_numpy(hyper).to(dev)
        th = torch.from_numpy(thresh).to(dev) if thresh is not None else None
        maxs = torch.full((NSEG,), junk - 7.0, dtype=torch.float32, device=dev) if want_maxs else None
        ws = torch.full((self.wsb // 4,), junk, dtype=torch.float32, device=dev)        # whatever the workspace held
        rc = self.L.tk_adamw_step_dev(_lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(ptrs), _lib.ptr(self.tiles),
                                      self.ntiles, NSEG, TOTAL, _lib.ptr(hyper), _lib.ptr(th), _lib.ptr(maxs), _lib.ptr(ws),
                                      self.wsb, int(max_norm is not None), int(zero_grads), cus, _lib.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
        hy = hyper.cpu().numpy()
        return dict(p=np.concatenate([p.cpu().numpy() for p in params]), m=m.cpu().numpy(), v=v.cpu().numpy(),
                    g=g.cpu().numpy(), maxs=maxs.cpu().numpy() if want_maxs else None,
                    norm=float(hy[D["TK_OPTIM_GRAD_NORM"]]), step=float(hy[D["TK_OPTIM_STEP"]]))


@pytest.fixture(scope="module")
def device(gpu_device):
    return Device(gpu_device)


def within(name, ours, lib, ref):
    """The measured rule; prints both errors first."""
    ours, lib, ref = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (ours, lib, ref))
    if ref.size == 0:
        return
    e_ours, e_lib = float(np.abs(ours - ref).max()), float(np.abs(lib - ref).max())
    allow = 2.0 * e_lib + float(np.spacing(F32(np.abs(ref).max())))
    print("optim-err %-40s ours %.3e  library %.3e  allowed %.3e" % (name, e_ours, e_lib, allow))
    assert np.isfinite(ours).all() and e_ours <= allow, (name, e_ours, e_lib, allow)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def same_bits(a, b):
    keys = [k for k in ("p", "m", "v", "g", "maxs") if a[k] is not None]
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys) and \
        np.array_equal(bits([a["norm"], a["step"]]), bits([b["norm"], b["step"]]))


CASES = list(itertools.product((False, True), (False, True), (None, INF, 30.0), (0, 1)))


@pytest.mark.parametrize("with_thresh,with_maxs,max_norm,zero_grads", CASES)
def test_one_step_against_float64(device, with_thresh, with_maxs, max_norm, zero_grads):
    inp, thresh = _inputs(), _thresholds() if with_thresh else None
    got = device.run(inp, HYPER, thresh, with_maxs, max_norm, zero_grads)
    want, lib = ref64(inp, HYPER, thresh, max_norm, zero_grads), torch32(inp, HYPER, thresh, max_norm, zero_grads)
    tag = "1step th%d mx%d cap%s z%d " % (with_thresh, with_maxs, max_norm, zero_grads)
    for k in ("p", "m", "v", "g"):
        within(tag + k, got[k], lib[k], want[k])
    if zero_grads:
        assert not got["g"].any()
    if with_maxs:
        within(tag + "maxs", got["maxs"], lib["maxs"], want["maxs"])
        assert got["maxs"][SIZES.index(0)] == 0.0
    if max_norm is not None:
        within(tag + "grad_norm", got["norm"], lib["norm"], want["norm"])
        if max_norm == 30.0:
            assert want["norm"] > 30.0, "the cap is active in this case"
    assert got["step"] == want["step"] == lib["step"] == 4.0


def test_a_cap_above_the_norm_changes_no_bit(device):
    inp, thresh = _inputs(1), _thresholds()
    free = device.run(inp, HYPER, thresh, True, INF, 0)
    assert free["norm"] < 1000.0
    assert same_bits(free, device.run(inp, HYPER, thresh, True, 1000.0, 0))
    none = device.run(inp, HYPER, thresh, True, None, 0)         # no norm at all: the same update
    assert all(np.array_equal(bits(free[k]), bits(none[k])) for k in ("p", "m", "v", "g", "maxs"))
    capped = device.run(inp, HYPER, thresh, True, 0.5 * free["norm"], 0)
    assert capped["norm"] == free["norm"] and not np.array_equal(bits(capped["g"]), bits(free["g"]))


def test_same_arguments_same_bits_at_every_grid(device):
    inp, thresh = _inputs(2), _thresholds()
    first = device.run(inp, HYPER, thresh, True, 30.0, 0)
    assert same_bits(first, device.run(inp, HYPER, thresh, True, 30.0, 0, junk=3.5e7))
    for cus in (1, 64):
        assert same_bits(first, device.run(inp, HYPER, thresh, True, 30.0, 0, cus=cus, junk=float(cus))), cus


def test_clip_is_the_clip_entry_points_bit_for_bit(device):
    """lr = 0, weight_decay = 0, zero_grads = 0: grads and maxs are tk_grad_maxabs_clip_dev's on a copy, the parameters do
    not change -- with a +inf threshold, a NaN in a clamped segment (that entry point clamps it to -thresh) and a
    one-element segment."""
    dev = device.dev
    inp, thresh = _inputs(3), _thresholds()
    one = SIZES.index(1)
    thresh[one] = 0.01
    inp["g"][OFF[one]] = 5.0
    nan_seg = SIZES.index(4095)
    assert np.isfinite(thresh[nan_seg]) and thresh[nan_seg] > 0 and thresh[SIZES.index(7)] == INF
    inp["g"][OFF[nan_seg] + 1234] = np.nan
    h = dict(HYPER, lr=F32(0.0), wd=F32(0.0), scale=F32(1.0))
    got = device.run(inp, h, thresh, True, None, 0)
    g = torch.from_numpy(inp["g"].copy()).to(dev)
    maxs = torch.zeros(NSEG, dtype=torch.float32, device=dev)
    seg_off, th = torch.from_numpy(OFF).to(dev), torch.from_numpy(thresh).to(dev)       # (named: alive until the launch ran)
    rc = _lib.lib().tk_grad_maxabs_clip_dev(_lib.ptr(g), _lib.ptr(seg_off), NSEG, max(SIZES), _lib.ptr(th), _lib.ptr(maxs),
                                            _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(got["g"]), bits(g.cpu().numpy()))
    assert np.array_equal(bits(got["maxs"]), bits(maxs.cpu().numpy()))
    assert np.isnan(got["maxs"][nan_seg]) and got["g"][OFF[nan_seg] + 1234] == -thresh[nan_seg]
    assert got["maxs"][one] == 5.0 and got["g"][OFF[one]] == F32(0.01)
    assert np.array_equal(bits(got["p"]), bits(inp["p"]))


def test_a_nan_spreads_as_in_torch(device):
    """One NaN gradient in a segment without a threshold: that element of p, m and v, its segment's maximum and the norm
    are NaN and nothing else is; with a finite cap the factor is NaN and so is everything (clip_grad_norm_ likewise)."""
    inp, thresh = _inputs(4), _thresholds()
    seg = SIZES.index(257)
    assert thresh[seg] == INF
    at = OFF[seg] + 17
    inp["g"][at] = np.nan
    for max_norm in (INF, 30.0):
        got, lib = device.run(inp, HYPER, thresh, True, max_norm, 0), torch32(inp, HYPER, thresh, max_norm, 0)
        for k in ("p", "m", "v", "g"):
            assert np.array_equal(np.isnan(got[k]), np.isnan(lib[k])), (k, max_norm)
            assert np.isnan(got[k][at]) and int(np.isnan(got[k]).sum()) == (1 if max_norm == INF else TOTAL)
        assert np.isnan(got["norm"]) and np.isnan(lib["norm"])
        assert np.array_equal(np.isnan(got["maxs"]), np.arange(NSEG) == seg)


# -- runs of steps on a model's arena --------------------------------------------------------------------------------

SCHEDULE = optim.OneCycle(4e-3, 40, pct_start=0.25, div_factor=40.0, final_div_factor=1.0, base_momentum=0.85,
                          max_momentum=0.9)
EPS, WD, B2, SCALE = 1e-6, 0.01, 0.999, 0.5


def _grads(total, k):
    return torch.randn(total, generator=torch.Generator().manual_seed(100 + k)) * 0.05


def _seg_thresholds(nseg, k, from_step):
    th = np.full(nseg, INF, dtype=F32)
    if from_step is not None and k >= from_step:
        th[::2] = 0.04
    return th


def drive(make_net, kinds, dev, thresh_from=None):
    """len(kinds) steps on one arena, step k by `kinds[k]` ("hip": FlatAdamW with the clipper folded in; "torch":
    mul_, DeviceClipper's launch pair, AdamW(capturable=True)); where the kind changes the state moves through
    state_dict / load_state_dict.  lr and beta1 from OneCycle every step.  Returns the parameters and the last maxima."""
    torch.manual_seed(5)
    net = make_net().to(dev)
    arena = parallel.FlatGradArena(net)
    clipper = clipping.DeviceClipper(arena, 0, 1000)
    opts = dict(hip=optim.FlatAdamW(arena, lr=1.0, betas=(0.9, B2), eps=EPS, weight_decay=WD, clipper=clipper),
                torch=torch.optim.AdamW(arena.params, lr=1.0, betas=(0.9, B2), eps=EPS, weight_decay=WD, capturable=True))
    total = arena.flat.numel()
    for k, kind in enumerate(kinds):
        lr, b1 = (float(F32(x)) for x in SCHEDULE.at(k))
        if k and kinds[k - 1] != kind:
            opts[kind].load_state_dict(opts[kinds[k - 1]].state_dict())
        arena.flat.copy_(_grads(total, k))
        clipper.thresh.copy_(torch.from_numpy(_seg_thresholds(clipper.nseg, k, thresh_from)))
        if kind == "hip":
            opts["hip"].set_lr(lr)
            opts["hip"].set_momentum(b1)
            opts["hip"].step(grad_scale=SCALE, zero_grads=True)
        else:
            arena.flat.mul_(SCALE)
            clipper.launch_kernels()
            for group in opts["torch"].param_groups:
                group["lr"], group["betas"] = lr, (b1, B2)
            opts["torch"].step()
    torch.cuda.synchronize()
    if kinds[-1] == "hip":
        assert float(opts["hip"].step_count) == len(kinds) and not bool(arena.flat.any())
    return (np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in arena.params]), clipper.maxs.cpu().numpy())


def drive64(make_net, steps, thresh_from=None):
    torch.manual_seed(5)
    net = make_net()
    sizes = [p.numel() for p in net.parameters() if p.requires_grad]
    off = np.concatenate([[0], np.cumsum(sizes)])
    p = np.concatenate([q.detach().numpy().reshape(-1) for q in net.parameters() if q.requires_grad]).astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for k in range(steps):
        lr, b1 = (float(F32(x)) for x in SCHEDULE.at(k))
        b2, eps, wd = float(F32(B2)), float(F32(EPS)), float(F32(WD))
        g = _grads(p.size, k).numpy().astype(np.float64) * SCALE
        maxs = np.array([np.abs(g[off[s]:off[s + 1]]).max() for s in range(len(sizes))])
        for s, th in enumerate(_seg_thresholds(len(sizes), k, thresh_from)):
            if np.isfinite(th):
                g[off[s]:off[s + 1]] = np.clip(g[off[s]:off[s + 1]], -float(th), float(th))
        t = k + 1.0
        p *= 1.0 - lr * wd
        m += (g - m) * (1.0 - b1)
        v = b2 * v + (1.0 - b2) * g * g
        p -= (lr / (1.0 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return p, maxs


ARENAS = {"mLstm_flipflop16": lambda: models.mLstm_flipflop(size=16),
          "mGru_cat_mod_flipflop32": lambda: models.mGru_cat_mod_flipflop(size=32)}


@pytest.mark.parametrize("arena", sorted(ARENAS))
def test_25_steps_on_a_models_arena(gpu_device, arena):
    make = ARENAS[arena]
    got, got_maxs = drive(make, ["hip"] * 25, gpu_device, thresh_from=5)
    lib, lib_maxs = drive(make, ["torch"] * 25, gpu_device, thresh_from=5)
    want, want_maxs = drive64(make, 25, thresh_from=5)
    within("25 steps %s params" % arena, got, lib, want)
    within("25 steps %s maxs" % arena, got_maxs, lib_maxs, want_maxs)


@pytest.mark.parametrize("order", [("hip", "torch"), ("torch", "hip")])
def test_state_dict_round_trip(gpu_device, order):
    """5 steps by one optimiser, its state loaded into the other, 5 more: the parameters stay within the rule of the ten
    steps taken by torch's alone."""
    make = ARENAS["mLstm_flipflop16"]
    got, _ = drive(make, [order[0]] * 5 + [order[1]] * 5, gpu_device)
    lib, _ = drive(make, ["torch"] * 10, gpu_device)
    want, _ = drive64(make, 10)
    within("state_dict %s -> %s params" % order, got, lib, want)


class _Arena:
    def __init__(self, dev):
        self.params = [torch.zeros(n, device=dev) for n in SIZES]
        self.flat = torch.zeros(TOTAL, device=dev)


class _Clipper:
    def __init__(self, arena, thresh):
        self.arena = arena
        self.thresh = torch.from_numpy(thresh).to(arena.flat.device)
        self.maxs = torch.zeros(NSEG, device=arena.flat.device)


def test_captured_step_reads_lr_and_beta1_at_replay(gpu_device):
    """`step()` captured once, replayed three times with `set_lr` / `set_momentum` (and new gradients) in between: bit for
    bit the same three eager calls; the step word advances by one per replay."""
    dev = gpu_device
    settings = [(4e-3, 0.9), (1e-3, 0.85), (2.5e-3, 0.5)]

    def setup():
        inp = _inputs(6)
        arena = _Arena(dev)
        for p, x in zip(arena.params, _segments(inp["p"])):
            p.copy_(torch.from_numpy(x))
        opt = optim.FlatAdamW(arena, lr=1.0, betas=(0.7, 0.999), eps=1e-6, weight_decay=0.01,
                              clipper=_Clipper(arena, _thresholds()), max_norm=30.0)
        opt.exp_avg.copy_(torch.from_numpy(inp["m"]))
        opt.exp_avg_sq.copy_(torch.from_numpy(inp["v"]))
        opt.set_grad_scale(0.5)
        return arena, opt

    def state(arena, opt):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in arena.params + [opt.exp_avg, opt.exp_avg_sq, arena.flat, opt.clipper.maxs,
                                                                opt.hyper[:D["TK_OPTIM_STEP_NOW"]]]]

    arena, opt = setup()
    eager = []
    for k, (lr, b1) in enumerate(settings):
        arena.flat.copy_(_grads(TOTAL, k) * 20)
        opt.set_lr(lr)
        opt.set_momentum(b1)
        opt.step(grad_scale=0.5, zero_grads=False)
        eager.append(state(arena, opt))
    arena, opt = setup()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, **train._CAPTURE):
        opt.step(grad_scale=0.5, zero_grads=False)          # (capture records, it does not run)
    torch.cuda.synchronize()
    assert float(opt.step_count) == 0.0
    for k, (lr, b1) in enumerate(settings):
        arena.flat.copy_(_grads(TOTAL, k) * 20)
        opt.set_lr(lr)
        opt.set_momentum(b1)
        graph.replay()
        got = state(arena, opt)
        assert float(opt.step_count) == k + 1.0
        assert float(opt.grad_norm) > 30.0, "the cap is active"
        for a, b in zip(got, eager[k]):
            assert np.array_equal(bits(a), bits(b)), k


# -- the trainers ------------------------------------------------------------------------------------------------------

def _batches(dev, n, nbatch=4, chunk_len=300, stride=5):
    from taiyaki_amd import synth
    out = []
    for i in range(n):
        seqlens = synth.realistic_seqlens(chunk_len // stride, nbatch, 40 + i, chunk_len, 9.0)
        seqs, _ = synth.sequences(seqlens, 40 + i)
        out.append(dict(indata=torch.from_numpy(synth.signal_chunks(chunk_len, nbatch, 40 + i)).to(dev),
                        seqs=torch.from_numpy(seqs).long(), seqlens=torch.from_numpy(seqlens).long()))
    return out


def test_trainer_with_the_hip_optimiser_against_without(gpu_device):
    """mGru_flipflop(size=32), T 60, N 4, five steps of two sub-batches, adaptive clipping on (window 2: the clamp is active
    from the third step).

    There is no float64 network to measure against, so the library's error is measured as the distance between two library
    trainers that differ only in float32 roundings of the optimiser: `hip_optim=False` as it is (torch.optim.AdamW,
    capturable: its bias corrections are float32 tensor arithmetic) and the same trainer with AdamW(capturable=False,
    foreach=False) (the same formula with the scalars computed in float64 on the host).  The rule is then the file's: the
    trainer on the HIP optimiser may be twice that distance plus one ulp of the largest weight away from the first.  The
    loss to first order: |dL| <= ||g||_1 x (the parameters' allowance), with the mean gradient the first trainer leaves in
    its arena, times 2 for the clamp and the second order, plus one ulp of the loss.  The three are printed every step."""
    dev = gpu_device
    torch.manual_seed(11)
    net_a = models.mGru_flipflop(size=32, stride=5).to(dev)
    net_b, net_c = copy.deepcopy(net_a), copy.deepcopy(net_a)
    subs = _batches(dev, 10)
    kw = dict(clip_num_mads=0, clip_window=2)
    tr_a = train.Trainer(net_a, parallel.FlatGradArena(net_a), hip_optim=False, **kw)
    tr_b = train.Trainer(net_b, parallel.FlatGradArena(net_b), hip_optim=True, **kw)
    tr_c = train.Trainer(net_c, parallel.FlatGradArena(net_c), hip_optim=False, **kw)
    group = tr_a.opt.param_groups[0]
    tr_c.opt = torch.optim.AdamW(tr_c.arena.params, lr=group["lr"], betas=group["betas"], eps=group["eps"],
                                 weight_decay=group["weight_decay"], capturable=False, foreach=False)
    assert isinstance(tr_b.opt, optim.FlatAdamW) and isinstance(tr_a.opt, torch.optim.AdamW)
    start = [p.detach().clone() for p in net_b.parameters()]
    apart = lambda x, y: max(float((p - q).abs().max()) for p, q in zip(x.parameters(), y.parameters()))     # noqa: E731
    lr, steps, allow_p = 4e-3, 5, 0.0
    for k in range(steps):
        batch = subs[2 * k:2 * k + 2]
        la, lb, lc = (float(t.step(batch)) for t in (tr_a, tr_b, tr_c))
        allow_l = 2.0 * float(tr_a.arena.flat.abs().sum()) * allow_p + float(np.spacing(F32(abs(la))))
        biggest = max(float(p.abs().max()) for p in net_a.parameters())
        d_ours, d_lib = apart(net_a, net_b), apart(net_a, net_c)
        allow_p = 2.0 * d_lib + float(np.spacing(F32(biggest)))
        print("optim-trainer step %d loss %.7f / hip %.7f / library %.7f (allowed %.3e)  |dp| hip %.3e library %.3e "
              "(allowed %.3e)" % (k, la, lb, lc, allow_l, d_ours, d_lib, allow_p))
        assert np.isfinite(la) and np.isfinite(lb)
        assert abs(la - lb) <= allow_l, (k, la, lb, allow_l)
        assert d_ours <= allow_p, (k, d_ours, d_lib, allow_p)
        assert not bool(tr_b.arena.flat.any()), "the update left the arena zeroed"
    assert tr_a.clipper.active and tr_b.clipper.active
    assert np.allclose(tr_a.clipper.last_maxs, tr_b.clipper.last_maxs, rtol=1e-3, atol=1e-9)
    assert float(tr_b.opt.step_count) == steps
    moved = max(float((p - q).abs().max()) for p, q in zip(net_b.parameters(), start))
    assert moved > lr, moved
    # the flag that skips arena.zero() holds only between an update that ran to its end and the next step
    assert tr_b._arena_zeroed
    tr_b.arena.flat.fill_(3.0)                  # a caller that wrote the arena ...
    tr_b._arena_zeroed = False                  # ... says so (Trainer.step clears the flag itself when it starts)
    la, lb, lc = (float(t.step(subs[:2])) for t in (tr_a, tr_b, tr_c))
    assert abs(la - lb) <= 2.0 * float(tr_a.arena.flat.abs().sum()) * allow_p + float(np.spacing(F32(abs(la))))
    d_ours, d_lib = apart(net_a, net_b), apart(net_a, net_c)
    print("optim-trainer step 5 (arena written by the caller) |dp| hip %.3e library %.3e" % (d_ours, d_lib))
    assert d_ours <= 2.0 * d_lib + float(np.spacing(F32(biggest)))


def test_norm_cap_of_the_ab_initio_trainer(gpu_device):
    """`grad_norm_cap_fraction`: every step's norm reaches the rolling quantile one step later; its value is the next step's
    cap (bin/train_abinitio.py:219-222)."""
    dev = gpu_device
    torch.manual_seed(12)
    net = models.mGru_flipflop(size=32, stride=5).to(dev)
    tr = train.Trainer(net, parallel.FlatGradArena(net), hip_optim=True, grad_norm_cap_fraction=0.5)
    norms = []
    for k, batch in enumerate(_batches(dev, 4)):
        tr.step(batch)
        assert tr.norm_cap.last_norm == (norms[-1] if norms else None)
        if norms:
            assert tr.norm_cap.cap == np.quantile(norms, 0.5)
            assert float(tr.opt.hyper[D["TK_OPTIM_MAX_NORM"]]) == F32(tr.norm_cap.cap)
        norms.append(float(tr.opt.grad_norm))
        assert np.isfinite(norms[-1]) and norms[-1] > 0


def test_hybrid_trainer_set_momentum_changes_the_next_replay():
    """Out of process (a failed hipGraph capture aborts inside the HIP runtime): tests/helpers/optim_hybrid.py."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "optim_hybrid.py")
    res = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "optim-hybrid-ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout.strip().splitlines()[-1])

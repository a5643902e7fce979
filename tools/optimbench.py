#!/usr/bin/env python
"""Times the tail of a train step alone on the GPU, on the gradient arenas of real models:

  chain    what train.Trainer runs with USE_HIP_OPTIM off: arena.zero(), arena.finish's mul_, DeviceClipper's launch pair,
           torch.optim.AdamW(capturable=True) (foreach)
  fused    the same chain with torch.optim.AdamW(fused=True, capturable=True), if this torch runs it
  flat     optim.FlatAdamW.step (scale, maxima, clamp, AdamW and the zero fill in its launch pair)

each eager and replayed from a hipGraph, the sides in turns inside one process (--turns turns a side, per turn the median of
--calls calls timed with device events after warm-up).  One JSON line per turn and one summary line per arena and mode.

The update launch moves seven float32 arrays of the arena (g, m, v, p read; g, m, v, p written, g's write being the fill):
its bytes over this library's own streaming copy rate (tk_devcopy_f32_dev on buffers that move the same number of bytes,
measured in the same run) are the time it cannot beat; `update_floor_fraction` is that time over the measured time of
FlatAdamW.step without clipper and norm (a one-thread launch and the update launch).

    python tools/optimbench.py [--turns 3] [--calls 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, clipping, models, optim, parallel, train  # noqa: E402

ARENAS = [("mLstm_flipflop", 96), ("mLstm_flipflop", 256), ("mLstm_flipflop", 384), ("mGru_flipflop", 96)]
SCALE = 0.5


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return 1e3 * float(np.median(times))


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, **train._CAPTURE):
        fn()
    torch.cuda.synchronize()
    return graph.replay


class Side:
    """One arena of its own per side: a copy of the model, gradients of a plausible size."""

    def __init__(self, name, size, kind, dev):
        torch.manual_seed(3)
        self.net = getattr(models, name)(size=size).to(dev)
        self.arena = parallel.FlatGradArena(self.net)
        self.clipper = clipping.DeviceClipper(self.arena, 0, 1000)
        self.clipper.thresh.fill_(0.05)
        self.grads = 0.05 * torch.randn_like(self.arena.flat)
        if kind == "flat":
            self.opt = optim.FlatAdamW(self.arena, lr=4e-3, eps=1e-6, clipper=self.clipper)
            self.call = lambda: self.opt.step(grad_scale=SCALE, zero_grads=True)
        else:
            self.opt = torch.optim.AdamW(self.arena.params, lr=4e-3, eps=1e-6, capturable=True, fused=(kind == "fused"),
                                         foreach=None if kind == "fused" else True)
            self.call = self.chain
        self.arena.flat.copy_(self.grads)

    def chain(self):
        self.arena.zero()
        self.arena.flat.mul_(SCALE)
        self.clipper.launch_kernels()
        self.opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimbench needs a GPU")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    for name, size in ARENAS:
        sides = {}
        for kind in ("chain", "fused", "flat"):
            try:
                sides[kind] = Side(name, size, kind, dev)
                sides[kind].call()
                torch.cuda.synchronize()
            except Exception as e:      # fused + capturable is not in every torch build for ROCm
                if kind != "fused":
                    raise
                sides.pop(kind, None)
                print(json.dumps(dict(arena=name, size=size, side=kind, skipped=str(e)[:120])), flush=True)
        n = sides["flat"].arena.flat.numel()
        tag = dict(arena=name, size=size, elements=n, tensors=len(sides["flat"].arena.params))
        for mode in ("eager", "graph"):
            calls = {k: (graphed(s.call) if mode == "graph" else s.call) for k, s in sides.items()}
            res = {k: [] for k in calls}
            for turn in range(a.turns):
                for k, fn in calls.items():
                    us = timed(fn, a.calls, a.warmup)
                    res[k].append(us)
                    print(json.dumps(dict(tag, mode=mode, turn=turn, side=k, us=round(us, 1))), flush=True)
            summary = dict(tag, mode=mode)
            for k, v in res.items():
                summary[k + "_us"] = round(float(np.median(v)), 1)
                summary[k + "_range_us"] = round(max(v) - min(v), 1)
            for k in res:
                if k != "flat":
                    summary["every_flat_turn_below_every_%s_turn" % k] = max(res["flat"]) < min(res[k])
            print(json.dumps(summary), flush=True)
        # the update launch against the streaming copy at the same number of bytes: 28 n moved = a copy of 3.5 n floats
        bare = optim.FlatAdamW(sides["flat"].arena, lr=4e-3, eps=1e-6)
        step = graphed(lambda: bare.step(grad_scale=SCALE, zero_grads=True))
        ncopy = (7 * n // 2 + 3) // 4 * 4
        src, dst = torch.randn(ncopy, device=dev), torch.empty(ncopy, device=dev)

        def copy():
            _lib.check(L.tk_devcopy_f32_dev(_lib.ptr(dst), _lib.ptr(src), ncopy, _lib.stream_ptr()), "tk_devcopy_f32_dev")

        copy_replay = graphed(copy)
        step_us, copy_us = [], []
        for turn in range(a.turns):
            step_us.append(timed(step, a.calls, a.warmup))
            copy_us.append(timed(copy_replay, a.calls, a.warmup))
        s_us, c_us = float(np.median(step_us)), float(np.median(copy_us))
        print(json.dumps(dict(tag, update_bytes=28 * n, update_step_us=round(s_us, 1), copy_same_bytes_us=round(c_us, 1),
                              copy_GBs=round(8.0 * ncopy / c_us / 1e3, 1), update_GBs=round(28.0 * n / s_us / 1e3, 1),
                              update_floor_fraction=round(c_us / s_us, 3))), flush=True)


if __name__ == "__main__":
    main()

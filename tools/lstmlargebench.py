#!/usr/bin/env python
"""Times one LSTM layer at hidden size 512 on the library of its own (csrc/lstm_kernels.hip built -DTK_LSTM_LARGE).

For every (T, N) of --shapes: tk_lstm_large_forward_dev (saving, and with NULL for the activations) and
tk_lstm_large_backward_dev at 4 and at 8 batch columns per group (the lab build's tk_lab_lstm_large_cols; a batch wider
than a forced count admits runs as slabs inside the call, so at N 128 on 256 CUs this is one launch at 8 columns against
two slabs at 4), each timed with device events after warm-up, --turns turns of the column counts one after the other;
then layers.Lstm(512, 512) on one input, forward (grad mode) and backward, the HIP recurrence and nn.LSTM
(layers.USE_HIP_LSTM_LARGE = False: MIOpen, what the size ran before) in turns in the same process.  Both sides of the
layer include the input GEMM and the weight gradients.  One JSON line per shape, microseconds per timestep (medians over
--steps).

    python tools/lstmlargebench.py [--shapes 800x64,800x128] [--steps 10] [--warmup 2] [--turns 3] [--reverse] [--cols 4,8]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, layers  # noqa: E402

H = 512


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def kernel_turns(T, N, reverse, cols, turns, steps, warmup, dev):
    """{"fwd" / "infer" / "bwd": {C: [us per step, one per turn]}, "launches": {C: slabs}} through the lab build's forced
    column counts"""
    g = torch.Generator(device="cpu").manual_seed(11)
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1).div_(H ** 0.5).to(dev)
    gx = torch.randn(T, N, 4 * H, generator=g).to(dev)
    dy = torch.randn(T, N, H, generator=g).div_((T * N) ** 0.5).to(dev)
    y, cell = torch.empty(T, N, H, device=dev), torch.empty(T, N, H, device=dev)
    gates, dg = torch.empty(T, N, 4 * H, device=dev), torch.empty(T, N, 4 * H, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    cus = layers._cu_count(dev)
    L = _lib.use_lab(True) and _lib.lstm_large_lib()
    p, stream = _lib.ptr, _lib.stream_ptr()
    out = {k: {c: [] for c in cols} for k in ("fwd", "infer", "bwd")}
    out["launches"] = {}
    try:
        for _ in range(turns):
            for C in cols:
                L.tk_lab_lstm_large_cols(C)
                wsb = L.tk_lstm_large_workspace_bytes(N, H, cus)
                if not wsb:
                    raise SystemExit("no launch at %d columns per group on %d CUs" % (C, cus))
                out["launches"][C] = -(-N // L.tk_lstm_large_slab(N, H, cus))
                ws = _lib.workspace(wsb, dev, "lstmlargebench")

                def fwd(save=True):
                    _lib.check(L.tk_lstm_large_forward_dev(p(gx), p(w_hh), None, T, N, H, int(reverse), cus, p(y),
                                                           p(gates if save else None), p(cell if save else None), p(ws),
                                                           wsb, p(status), stream), "tk_lstm_large_forward_dev")

                def bwd():
                    _lib.check(L.tk_lstm_large_backward_dev(p(w_hh), p(gates), p(cell), p(dy), None, T, N, H,
                                                            int(reverse), cus, p(dg), p(ws), wsb, p(status), stream),
                               "tk_lstm_large_backward_dev")

                for k, fn in (("fwd", fwd), ("infer", lambda: fwd(False)), ("bwd", bwd)):
                    out[k][C].append(round(1e3 * timed(fn, steps, warmup) / T, 3))
                if int(status.item()):
                    raise SystemExit("status word %d" % int(status.item()))
    finally:
        L.tk_lab_lstm_large_cols(0)
        _lib.use_lab(False)
    return out


def layer_turns(T, N, reverse, turns, steps, warmup, dev):
    """{"hip_fwd", "hip_bwd", "nn_lstm_fwd", "nn_lstm_bwd": [us per step, one per turn]}"""
    torch.manual_seed(12)
    lstm = layers.Lstm(H, H).to(dev)
    layer = layers.Reverse(lstm) if reverse else lstm
    x = torch.randn(T, N, H, device=dev).requires_grad_(True)
    dy = torch.randn(T, N, H, device=dev).div_((T * N) ** 0.5)
    if not layers.hip_lstm_large_workspace_bytes(lstm.rnn, x):
        raise SystemExit("the size-512 recurrence does not take this layer")

    def one(use_hip):
        layers.USE_HIP_LSTM_LARGE = use_hip
        f, b = [], []
        for i in range(warmup + steps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            y = layer(x)
            e[1].record()
            y.backward(dy)
            e[2].record()
            e[2].synchronize()
            if i >= warmup:
                f.append(e[0].elapsed_time(e[1]))
                b.append(e[1].elapsed_time(e[2]))
        return round(1e3 * float(np.median(f)) / T, 3), round(1e3 * float(np.median(b)) / T, 3)

    keys = ("hip_fwd", "hip_bwd", "nn_lstm_fwd", "nn_lstm_bwd")
    out = {k: [] for k in keys}
    old = layers.USE_HIP_LSTM_LARGE
    try:
        for _ in range(turns):
            for k, v in zip(keys, one(True) + one(False)):
                out[k].append(v)
    finally:
        layers.USE_HIP_LSTM_LARGE = old
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="800x64,800x128", help="T x N, comma separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--cols", default="4,8", help="forced batch columns per group, comma separated")
    ap.add_argument("--reverse", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstmlargebench needs a GPU (the recurrence has no CPU fallback)")
    dev = torch.device("cuda:0")
    cols = [int(c) for c in a.cols.split(",")]
    for shape in a.shapes.split(","):
        T, N = (int(v) for v in shape.split("x"))
        cus = layers._cu_count(dev)
        geo = (ctypes.c_size_t * 8)()
        L = _lib.use_lab(True) and _lib.lstm_large_lib()
        try:
            rule = list(geo)[2:6] if L.tk_lab_lstm_large_geometry(N, H, cus, geo) else None
        finally:
            _lib.use_lab(False)
        out = {"T": T, "N": N, "H": H, "reverse": a.reverse, "cus": cus, "rule_U_C_groups_grid": rule,
               "kernel_us_per_step_by_cols": kernel_turns(T, N, a.reverse, cols, a.turns, a.steps, a.warmup, dev),
               "layer_us_per_step": layer_turns(T, N, a.reverse, a.turns, a.steps, a.warmup, dev),
               "device": torch.cuda.get_device_name(dev)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

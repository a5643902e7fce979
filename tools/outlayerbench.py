#!/usr/bin/env python
"""Times the output layer alone on the GPU: the kernels of csrc/out_layer.hip against the library path
(layers.USE_HIP_OUT_LAYER = False: nn.Linear and the element-wise operators behind it), the switch on and off in turns
inside one process, --turns turns a side, per turn the median of --calls calls timed with device events after warm-up.
One JSON line per turn and, per measurement, one line that says whether EVERY turn of the kernels was below EVERY turn
of the library path, with the difference of the medians against the larger of the two sides' max - min ranges.

  rows = T N = 800 x 128 (--rows: other numbers of rows, 128 columns each, to see where the grad-mode rule
      layers.OUT_LAYER_GRAD_MIN_ROWS and OUT_LAYER_PLAIN_GRAD_MIN_ROWS has to draw its line; the rule is lifted while this
      runs),
  I = 96, 256 and 384, the plain layer (nbase 4) and the cat-mod layer (1, 1, 0, 0),
  forward alone (no_grad) and forward + backward (dx, dW and db).

    python tools/outlayerbench.py [--turns 3] [--calls 20] [--warmup 5] [--rows 102400 ...]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import layers  # noqa: E402


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


def compare(tag, fn, a):
    res = {True: [], False: []}
    for turn in range(a.turns):
        for hip in (True, False):
            layers.USE_HIP_OUT_LAYER = hip
            us = timed(fn, a.calls, a.warmup)
            res[hip].append(us)
            print(json.dumps(dict(tag, turn=turn, path="kernels" if hip else "library", us=round(us, 1))), flush=True)
    layers.USE_HIP_OUT_LAYER = True
    op, ref = res[True], res[False]
    spread = max(max(op) - min(op), max(ref) - min(ref))
    diff = float(np.median(ref) - np.median(op))
    print(json.dumps(dict(tag, kernels_us=round(float(np.median(op)), 1), library_us=round(float(np.median(ref)), 1),
                          difference_us=round(diff, 1), larger_range_us=round(spread, 1),
                          difference_over_range=round(diff / spread, 1) if spread > 0 else None,
                          every_kernel_turn_below_every_library_turn=max(op) < min(ref))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[800 * 128])
    ap.add_argument("--sizes", type=int, nargs="+", default=[96, 256, 384])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("outlayerbench needs a GPU")
    dev = torch.device("cuda:0")
    torch.backends.cuda.preferred_blas_library("cublas")        # rocBLAS, as bench.py runs the GEMM path
    rule = {"plain": layers.OUT_LAYER_PLAIN_GRAD_MIN_ROWS, "cat-mod": layers.OUT_LAYER_GRAD_MIN_ROWS}
    layers.OUT_LAYER_GRAD_MIN_ROWS = layers.OUT_LAYER_PLAIN_GRAD_MIN_ROWS = 0      # (measure what the rule excludes too)
    for rows in a.rows:
        N = 128 if rows % 128 == 0 else 1
        T = rows // N
        for I in a.sizes:
            for kind in ("plain", "cat-mod"):
                torch.manual_seed(1)
                layer = (layers.GlobalNormFlipFlop(I, 4) if kind == "plain"
                         else layers.GlobalNormFlipFlopCatMod(I, (1, 1, 0, 0))).to(dev)
                nout = layer.size if kind == "plain" else layer.nout
                x = (2 * torch.rand(T, N, I, device=dev) - 1).requires_grad_(True)
                dy = torch.randn(T, N, nout, device=dev)
                assert layers.hip_out_layer_takes(layer, x)
                tag = dict(rows=rows, I=I, layer=kind, rule_admits_grad=rule[kind] is not None and rows >= rule[kind])

                def fwd():
                    with torch.no_grad():
                        layer(x)

                def fwd_bwd():
                    layer.zero_grad(set_to_none=True)
                    x.grad = None
                    layer(x).backward(dy)

                calls = dict(layers.out_layer_calls)
                compare(dict(tag, what="fwd"), fwd, a)
                compare(dict(tag, what="fwd+bwd"), fwd_bwd, a)
                assert layers.out_layer_calls["forward"] > calls["forward"]
                assert layers.out_layer_calls["backward"] > calls["backward"]
    layers.OUT_LAYER_PLAIN_GRAD_MIN_ROWS, layers.OUT_LAYER_GRAD_MIN_ROWS = rule["plain"], rule["cat-mod"]
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "grad_min_rows": rule}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times the two narrow Convolution layers (csrc/conv_kernels.hip) on the GPU: conv 1 (1 -> 4) and conv 2 (4 -> 16),
winlen 5, swish, forward and backward, at (T, N) = (4000, 128) and (8000, 64), each timed with device events after
warm-up.  The HIP operator and the unfold + GEMM path (layers.USE_HIP_CONV = False) run in one process; one JSON
line each (median and min over --steps, and the achieved GB/s against the compulsory bytes: forward reads x and
writes y, backward reads dy and x and writes dx where the layer has an input gradient -- conv 1 has none).  Then conv 3
(16 -> 256, window 19, stride 5; csrc/conv_strided.hip) against its unfold + GEMM path, in alternating turns (`conv3`).

    python tools/convbench.py [--steps 30] [--warmup 5] [--shapes 4000x128 8000x64] [--turns 5] [--calls 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import layers  # noqa: E402


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
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["4000x128", "8000x64"])
    ap.add_argument("--turns", type=int, default=5, help="conv 3: alternating turns of the kernels and the GEMM path")
    ap.add_argument("--calls", type=int, default=20, help="conv 3: calls per turn")
    ap.add_argument("--cout", type=int, nargs="*", default=[256], help="conv 3: output channels (the models' size)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convbench needs a GPU")
    dev = torch.device("cuda:0")
    torch.backends.cuda.preferred_blas_library("cublas")        # rocBLAS, as bench.py runs the GEMM path
    for shape in a.shapes:
        T, N = (int(v) for v in shape.split("x"))
        for name, cin, cout, want_dx in (("conv1", 1, 4, False), ("conv2", 4, 16, True)):
            torch.manual_seed(1)
            conv = layers.Convolution(cin, cout, 5, stride=1, fun=layers.swish).to(dev)
            x = torch.randn(T, N, cin, device=dev).requires_grad_(want_dx)
            dy = torch.randn(T, N, cout, device=dev)
            fwd_bytes = 4 * T * N * (cin + cout)
            bwd_bytes = 4 * T * N * (cout + cin + (cin if want_dx else 0))
            for hip in (True, False):
                layers.USE_HIP_CONV = hip
                y = conv(x)

                def fwd():
                    with torch.no_grad():
                        conv(x)

                def bwd():
                    y.backward(dy, retain_graph=True)

                f_med, f_min = timed(fwd, a.steps, a.warmup)
                b_med, b_min = timed(bwd, a.steps, a.warmup)
                print(json.dumps({"layer": name, "T": T, "N": N, "path": "hip" if hip else "gemm",
                                  "fwd_us": round(1e3 * f_med, 1), "fwd_min_us": round(1e3 * f_min, 1),
                                  "bwd_us": round(1e3 * b_med, 1), "bwd_min_us": round(1e3 * b_min, 1),
                                  "fwd_MB": round(fwd_bytes / 1e6, 2), "bwd_MB": round(bwd_bytes / 1e6, 2),
                                  "fwd_GBps": round(fwd_bytes / f_med / 1e6, 1),
                                  "bwd_GBps": round(bwd_bytes / b_med / 1e6, 1),
                                  "device": torch.cuda.get_device_name(dev)}))
                conv.zero_grad(set_to_none=True)
                x.grad = None
            layers.USE_HIP_CONV = True
        for cout in a.cout:
            conv3(T, N, cout, a, dev)


def conv3(T, N, cout, a, dev):
    """The third layer (16 -> cout, window 19, stride 5; csrc/conv_strided.hip): the kernels and the unfold + GEMM path
    (layers.USE_HIP_CONV_STRIDED = False) in alternating turns, the median of --calls calls per turn; the forward in
    grad mode, as a training step runs it.  The last line says whether the kernels were below the GEMM path in every
    turn."""
    torch.manual_seed(1)
    conv = layers.Convolution(16, cout, 19, stride=5, fun=layers.swish).to(dev)
    x = torch.randn(T, N, 16, device=dev).requires_grad_(True)
    dy = torch.randn((T + 4) // 5, N, cout, device=dev)
    gflop = 2 * dy.shape[0] * N * cout * 304 / 1e9
    if not conv._hip_strided(x):
        print(json.dumps({"layer": "conv3", "T": T, "N": N, "cout": cout, "kernels": "not admitted at this size"}))
        return
    res = {True: [], False: []}
    for turn in range(a.turns):
        for hip in (True, False):
            layers.USE_HIP_CONV_STRIDED = hip
            y = conv(x)
            f_med, f_min = timed(lambda: conv(x), a.calls, a.warmup)
            b_med, b_min = timed(lambda: y.backward(dy, retain_graph=True), a.calls, a.warmup)
            res[hip].append((f_med, b_med))
            print(json.dumps({"layer": "conv3", "T": T, "N": N, "cout": cout, "turn": turn, "path": "hip" if hip else "gemm",
                              "fwd_us": round(1e3 * f_med, 1), "fwd_min_us": round(1e3 * f_min, 1),
                              "bwd_us": round(1e3 * b_med, 1), "bwd_min_us": round(1e3 * b_min, 1),
                              "gflop_per_gemm": round(gflop, 2)}))
            del y
            conv.zero_grad(set_to_none=True)
            x.grad = None
    layers.USE_HIP_CONV_STRIDED = True
    print(json.dumps({"layer": "conv3", "T": T, "N": N, "cout": cout, "hip_below_gemm_every_turn": {
        "fwd": max(f for f, _ in res[True]) < min(f for f, _ in res[False]),
        "bwd": max(b for _, b in res[True]) < min(b for _, b in res[False])}}))


if __name__ == "__main__":
    main()

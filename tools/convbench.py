#!/usr/bin/env python
"""Times the two narrow Convolution layers (csrc/conv_kernels.hip) on the GPU: conv 1 (1 -> 4) and conv 2 (4 -> 16),
winlen 5, swish, forward and backward, at (T, N) = (4000, 128) and (8000, 64), each timed with device events after
warm-up.  The HIP operator and the unfold + GEMM path (layers.USE_HIP_CONV = False) run in one process; one JSON
line each (median and min over --steps, and the achieved GB/s against the compulsory bytes: forward reads x and
writes y, backward reads dy and x and writes dx where the layer has an input gradient -- conv 1 has none).  Then conv 3
(16 -> 256, window 19, stride 5; csrc/conv_strided.hip) against its unfold + GEMM path, in alternating turns (`conv3`).
--signal: only the mGru models' first layer (1 -> Cout on the raw signal, window 19, tanh; csrc/conv_signal.hip) against
its unfold + GEMM path, in alternating turns, at every TxN:stride:cout[:fwd] of --signal-shapes (`signal`).
--window: only conv 3 at the fast and the RNA models' shapes (16 -> Cout, window 19 or 31, stride 5, 10 or 12;
csrc/conv_strided.hip built -DTK_CONV_WINDOW) against its unfold + GEMM path, in alternating turns, at every
TxN:cout:winlen:stride of --window-shapes (`window`).

    python tools/convbench.py [--steps 30] [--warmup 5] [--shapes 4000x128 8000x64] [--turns 5] [--calls 20]
    python tools/convbench.py --signal [--signal-shapes 2000x64:2:96 60000x8:4:96:fwd] [--turns 5] [--calls 20]
    python tools/convbench.py --window [--window-shapes 4000x128:96:19:5 20000x128:256:31:10] [--turns 5] [--calls 20]
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
    ap.add_argument("--signal", action="store_true", help="time the signal convolution (1 -> Cout, tanh) only")
    ap.add_argument("--signal-shapes", nargs="*", default=["2000x64:2:96", "4000x128:5:256", "4000x128:5:384",
                                                            "60000x8:4:96:fwd"],
                    help="signal: TxN:stride:cout, `:fwd` for the forward alone (whole reads)")
    ap.add_argument("--window", action="store_true",
                    help="time conv 3 at the fast and the RNA models' shapes (libtaiyaki_amd_conv_window.so) only")
    ap.add_argument("--window-shapes", nargs="*",
                    default=["4000x128:96:19:5", "2000x256:96:19:5", "20000x128:256:31:10", "10000x256:256:31:10",
                             "20000x128:96:31:12", "10000x256:96:31:12"],
                    help="window: TxN:cout:winlen:stride (the trainer's shapes: DNA fast, RNA, RNA fast)")
    ap.add_argument("--host-warmup", type=int, default=1000, help="signal: eager calls per path before the first turn")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convbench needs a GPU")
    dev = torch.device("cuda:0")
    torch.backends.cuda.preferred_blas_library("cublas")        # rocBLAS, as bench.py runs the GEMM path
    if a.window:
        for spec in a.window_shapes:
            shape, cout, winlen, stride = spec.split(":")
            T, N = (int(v) for v in shape.split("x"))
            window(T, N, int(cout), int(winlen), int(stride), a, dev)
        return
    if a.signal:
        for spec in a.signal_shapes:
            shape, stride, cout, *rest = spec.split(":")
            T, N = (int(v) for v in shape.split("x"))
            signal(T, N, int(stride), int(cout), rest == ["fwd"], a, dev)
        return
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


def window(T, N, cout, winlen, stride, a, dev):
    """The third layer at the fast and the RNA models' shapes (16 -> cout, window 19 or 31, stride 5, 10 or 12;
    libtaiyaki_amd_conv_window.so): the kernels and the unfold + GEMM path (layers.USE_HIP_CONV_WINDOW = False) in
    alternating turns, as `conv3` runs them, the forward in grad mode with the configuration in
    layers.CONV_WINDOW_GRAD_SHAPES whatever that table holds.  The last line says in how many turns the kernels' forward
    + backward was not behind the GEMM path's: the majority puts a configuration into the table."""
    torch.manual_seed(1)
    conv = layers.Convolution(16, cout, winlen, stride=stride, fun=layers.swish).to(dev)
    x = torch.randn(T, N, 16, device=dev).requires_grad_(True)
    dy = torch.randn(-(-T // stride), N, cout, device=dev)
    tag = {"layer": "window", "T": T, "N": N, "cout": cout, "winlen": winlen, "stride": stride}
    table = layers.CONV_WINDOW_GRAD_SHAPES
    layers.CONV_WINDOW_GRAD_SHAPES = table | {(cout, winlen, stride)}
    try:
        if conv._hip_strided(x) or not conv._hip_window(x):
            print(json.dumps(dict(tag, kernels="not this library's shape")))
            return
        res = {True: [], False: []}
        for turn in range(a.turns):
            for hip in (True, False):
                layers.USE_HIP_CONV_WINDOW = hip
                calls = dict(layers.conv_window_calls)
                y = conv(x)
                f_med, f_min = timed(lambda: conv(x), a.calls, a.warmup)
                b_med, b_min = timed(lambda: y.backward(dy, retain_graph=True), a.calls, a.warmup)
                assert (layers.conv_window_calls != calls) == hip
                res[hip].append((f_med, b_med))
                print(json.dumps(dict(tag, turn=turn, path="hip" if hip else "gemm", fwd_us=round(1e3 * f_med, 1),
                                      fwd_min_us=round(1e3 * f_min, 1), bwd_us=round(1e3 * b_med, 1),
                                      bwd_min_us=round(1e3 * b_min, 1), fwd_bwd_us=round(1e3 * (f_med + b_med), 1))))
                del y
                conv.zero_grad(set_to_none=True)
                x.grad = None
        not_behind = sum(fh + bh <= fg + bg for (fh, bh), (fg, bg) in zip(res[True], res[False]))
        print(json.dumps(dict(tag, turns=a.turns, hip_fwd_bwd_not_behind_gemm_turns=not_behind,
                              hip_fwd_bwd_us=round(1e3 * float(np.median([f + b for f, b in res[True]])), 1),
                              gemm_fwd_bwd_us=round(1e3 * float(np.median([f + b for f, b in res[False]])), 1),
                              grad_mode=bool(2 * not_behind > a.turns))))
    finally:
        layers.USE_HIP_CONV_WINDOW = True
        layers.CONV_WINDOW_GRAD_SHAPES = table


def signal(T, N, stride, cout, fwd_only, a, dev):
    """The mGru models' first layer (1 -> cout, window 19, tanh; csrc/conv_signal.hip): the kernels and the unfold + GEMM
    path (layers.USE_HIP_CONV_SIGNAL = False) in alternating turns, the median of --calls calls per turn: the forward
    under no_grad, as a basecaller runs it, the grad-mode forward + backward of a training step called eagerly (the
    larger of the host's and the device's time), and the same step (whole reads: the forward) replayed from a hipGraph
    (the device's time alone).  The last line says whether the kernels were below the GEMM path in every turn."""
    torch.manual_seed(1)
    conv = layers.Convolution(1, cout, 19, stride=stride).to(dev)
    x = torch.randn(T, N, 1, device=dev)
    tout = -(-T // stride)
    dy = torch.randn(tout, N, cout, device=dev)
    tag = {"layer": "signal", "T": T, "N": N, "stride": stride, "cout": cout}
    if not conv._hip_signal(x):
        print(json.dumps(dict(tag, kernels="not admitted at this size")))
        return

    def fwd():
        with torch.no_grad():
            conv(x)

    def both():
        conv(x).backward(dy)

    def step():
        return torch.autograd.grad(conv(x), [conv.conv.weight, conv.conv.bias], dy)

    def captured(fn):       # one hipGraph of the call, as a captured train step holds it: replays cost the host nothing
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = fn()
        return g, keep

    graphs = {}
    for hip in (True, False):
        layers.USE_HIP_CONV_SIGNAL = hip
        graphs[hip] = captured(fwd if fwd_only else step)
        # the eager calls are bound by the host at these sizes, and the host (the autograd thread, the allocator's
        # pools, its clocks) takes a few hundred calls to settle: both paths get them before the first turn
        for _ in range(a.host_warmup):
            fwd() if fwd_only else both()
        torch.cuda.synchronize()
    res = {True: [], False: []}
    for turn in range(a.turns):
        for hip in (True, False):
            layers.USE_HIP_CONV_SIGNAL = hip
            f_med, f_min = timed(fwd, a.calls, a.warmup)
            fb_med, fb_min = (f_med, f_min) if fwd_only else timed(both, a.calls, a.warmup)
            g_med, g_min = timed(graphs[hip][0].replay, a.calls, a.warmup)
            res[hip].append((f_med, fb_med, g_med))
            line = dict(tag, turn=turn, path="hip" if hip else "gemm", fwd_us=round(1e3 * f_med, 1),
                        fwd_min_us=round(1e3 * f_min, 1), y_MB=round(4 * tout * N * cout / 1e6, 1))
            if not fwd_only:
                line.update(fwd_bwd_us=round(1e3 * fb_med, 1), fwd_bwd_min_us=round(1e3 * fb_min, 1))
            line.update({"graph_%s_us" % ("fwd" if fwd_only else "fwd_bwd"): round(1e3 * g_med, 1),
                         "graph_min_us": round(1e3 * g_min, 1)})
            print(json.dumps(line))
            conv.zero_grad(set_to_none=True)
    layers.USE_HIP_CONV_SIGNAL = True
    below = {"fwd": max(r[0] for r in res[True]) < min(r[0] for r in res[False])}
    if not fwd_only:
        below["fwd_bwd"] = max(r[1] for r in res[True]) < min(r[1] for r in res[False])
    below["graph"] = max(r[2] for r in res[True]) < min(r[2] for r in res[False])
    print(json.dumps(dict(tag, hip_below_gemm_every_turn=below)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times one layer's LSTM recurrence (csrc/lstm_kernels.hip) on the GPU: tk_lstm_forward_dev and
tk_lstm_backward_dev at (T, N, H), each timed with device events after warm-up; prints one JSON line per
units setting (microseconds per timestep and direction, median and min over --steps).  The flagship layer
(config 2) is the default shape.  The weight-gradient leg follows: `wgrad_ms` is tk_lstm_weight_grad_dev
(csrc/lstm_wgrad.hip) at (T, N, H, I = H), `wgrad_gemm_ms` the two GEMMs and the sum over dG that it replaces.
The projection legs (csrc/rnn_proj.hip, include/taiyaki_amd_rnn_proj.h) come last: `proj_ms` is tk_rnn_input_proj_dev
(x W_ih^T + b) and `proj_gemm_ms` the torch.addmm it replaces, `dx_ms` tk_rnn_input_grad_dev (dG W_ih) and `dx_gemm_ms`
the `@` it replaces, each pair timed in --proj-turns alternating turns (the median of --steps calls per turn and the
list of turns are both printed).

    python tools/lstmbench.py [--T 800] [--N 128] [--H 256] [--steps 20] [--warmup 3] [--units 0 16 32 64] [--varlen]
                              [--fallback PAIRS]

--varlen also times, in turns of five, tk_lstm_forward_varlen_dev with every length = T beside the forward, and the
training pair with per-column lengths (include/taiyaki_amd_rnn_varlen_train.h), forward and backward, at lengths = NULL
and at a half-full pattern (lengths[n] spread evenly over 0..T) beside tk_lstm_forward_dev / tk_lstm_backward_dev.

--units (lab build) forces the hidden units per workgroup; 0 is the release rule.  Without --units the
release library is timed.  H = 192 and 384 run at 48 units whatever is forced: a setting other than 0 is reported as
skipped there, with the units of the plan.

--fallback PAIRS times layers.Lstm(H, H) on one input, forward (grad mode) and backward, PAIRS times in turns: the HIP
recurrence, then nn.LSTM (layers.USE_HIP_LSTM = False: MIOpen, what a size the kernels refuse runs).  Both sides include
the input GEMM and the weight gradients; one JSON line, microseconds per timestep, in front of the others.
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


def proj_turns(T, N, H, gates, turns, steps, warmup, dev):
    """The two projection GEMMs of one recurrent layer (I = H, `gates` H gate columns) as the kernel of
    include/taiyaki_amd_rnn_proj.h and as the rocBLAS call it replaces, in alternating turns: {leg: [median ms per
    turn]}, the largest difference between the two relative to the largest entry, and the GFLOP of one call."""
    g = torch.Generator(device="cpu").manual_seed(13)
    rows, G = T * N, gates * H
    x = torch.randn(rows, H, generator=g).to(dev)
    dgt = torch.randn(rows, G, generator=g).to(dev)
    w = (torch.rand(G, H, generator=g) * 2 - 1).div_(H ** 0.5).to(dev)
    b = torch.randn(G, generator=g).to(dev)
    cus = layers._cu_count(dev)
    P = _lib.rnn_proj_lib()
    # (the workspace depends on the widths alone; below the rows the rule admits the legs are timed all the same)
    big = max(rows, 1 << 16)
    wsb = max(P.tk_rnn_proj_workspace_bytes(big, H, G, cus), P.tk_rnn_proj_workspace_bytes(big, G, H, cus))
    if min(P.tk_rnn_proj_workspace_bytes(big, H, G, cus), P.tk_rnn_proj_workspace_bytes(big, G, H, cus)) == 0:
        raise SystemExit("(H, gates) = (%d, %d) has no projection plan" % (H, gates))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    gx, dx = torch.empty(rows, G, device=dev), torch.empty(rows, H, device=dev)
    stream = _lib.stream_ptr()
    legs = {
        "proj_ms": lambda: _lib.check(P.tk_rnn_input_proj_dev(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), rows, H, G, cus,
                                                              _lib.ptr(gx), _lib.ptr(ws), wsb, stream), "proj"),
        "proj_gemm_ms": lambda: torch.addmm(b, x, w.t()),
        "dx_ms": lambda: _lib.check(P.tk_rnn_input_grad_dev(_lib.ptr(dgt), _lib.ptr(w), rows, H, G, cus, _lib.ptr(dx),
                                                            _lib.ptr(ws), wsb, stream), "dx"),
        "dx_gemm_ms": lambda: dgt @ w,
    }
    out = {k: [] for k in legs}
    for _ in range(turns):
        for k, fn in legs.items():
            out[k].append(round(timed(fn, steps, warmup)[0], 4))
    ref_gx, ref_dx = torch.addmm(b, x, w.t()), dgt @ w
    diff = max(((gx - ref_gx).abs().max() / ref_gx.abs().max()).item(),
               ((dx - ref_dx).abs().max() / ref_dx.abs().max()).item())
    admitted = [P.tk_rnn_proj_workspace_bytes(rows, H, G, cus) > 0, P.tk_rnn_proj_workspace_bytes(rows, G, H, cus) > 0]
    return out, diff, 2.0 * rows * H * G * 1e-9, admitted


def proj_report(T, N, H, gates, turns, steps, warmup, dev):
    """proj_turns as the keys of a result line: each leg's median over the turns, the turns, TFLOP/s of the medians."""
    legs, diff, gflop, admitted = proj_turns(T, N, H, gates, turns, steps, warmup, dev)
    rep = {k: float(np.median(v)) for k, v in legs.items()}
    rep.update({k.replace("_ms", "_turns_ms"): v for k, v in legs.items()})
    rep.update({k.replace("_ms", "_tflops"): round(gflop / np.median(v), 1) for k, v in legs.items()})
    rep["proj_vs_gemm_maxrel"] = diff
    rep["proj_admitted"], rep["dx_admitted"] = admitted
    return rep


def layer_turns(T, N, H, pairs, steps, warmup, dev):
    """[(hip fwd, hip bwd, nn.LSTM fwd, nn.LSTM bwd)] * pairs, median microseconds per timestep."""
    torch.manual_seed(12)
    layer = layers.Lstm(H, H).to(dev)
    x = torch.randn(T, N, H, device=dev).requires_grad_(True)
    dy = torch.randn(T, N, H, device=dev).div_((T * N) ** 0.5)
    if layers.hip_lstm_workspace_bytes(layer.rnn, x) == 0:
        raise SystemExit("(N, H) = (%d, %d) is not admitted on %d CUs" % (N, H, layers._cu_count(dev)))

    def one(use_hip):
        layers.USE_HIP_LSTM = use_hip
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
        return 1e3 * float(np.median(f)) / T, 1e3 * float(np.median(b)) / T

    try:
        return [one(True) + one(False) for _ in range(pairs)]
    finally:
        layers.USE_HIP_LSTM = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=800)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reverse", action="store_true")
    ap.add_argument("--varlen", action="store_true",
                    help="also time tk_lstm_forward_varlen_dev (release rule) with every length = T, in turns with the forward")
    ap.add_argument("--proj-turns", type=int, default=5, help="alternating turns of the projection legs")
    ap.add_argument("--units", type=int, nargs="*", default=None, help="(lab) units per workgroup; 0 = release rule")
    ap.add_argument("--fallback", type=int, default=0, metavar="PAIRS",
                    help="also time layers.Lstm(H, H) forward and backward, HIP and nn.LSTM in turns, PAIRS times")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstmbench needs a GPU (the LSTM recurrence has no CPU fallback)")
    dev = torch.device("cuda:0")
    T, N, H = a.T, a.N, a.H
    g = torch.Generator(device="cpu").manual_seed(11)
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1).div_(H ** 0.5).to(dev)
    gx = torch.randn(T, N, 4 * H, generator=g).to(dev)
    dy = torch.randn(T, N, H, generator=g).div_((T * N) ** 0.5).to(dev)
    y = torch.empty(T, N, H, device=dev)
    gates = torch.empty(T, N, 4 * H, device=dev)
    cell = torch.empty(T, N, H, device=dev)
    dg = torch.empty(T, N, 4 * H, device=dev)
    x_in = torch.randn(T, N, H, generator=g).to(dev)
    cus = layers._cu_count(dev)
    _lib.set_strict(False)
    if a.fallback:
        turns = layer_turns(T, N, H, a.fallback, a.steps, a.warmup, dev)
        keys = ("hip_fwd", "hip_bwd", "nn_lstm_fwd", "nn_lstm_bwd")
        print(json.dumps({"T": T, "N": N, "H": H, "layer_turns_us_per_step": {k: [round(t[i], 3) for t in turns]
                                                                              for i, k in enumerate(keys)}}))
    for units in (a.units if a.units is not None else [None]):
        L = _lib.use_lab(units is not None)
        if units is not None:
            L.tk_lab_lstm_units(units)
        wsb = L.tk_lstm_workspace_bytes(N, H, cus)
        if wsb == 0:
            raise SystemExit("(N, H) = (%d, %d) is not admitted on %d CUs" % (N, H, cus))
        if units:
            plan = (ctypes.c_size_t * 8)()
            L.tk_lab_lstm_geometry(N, H, cus, plan)
            if plan[2] not in (16, 32, 64):  # H = 192, 384: the forced units do not apply
                L.tk_lab_lstm_units(0)
                print(json.dumps({"T": T, "N": N, "H": H, "units": units, "skipped": "the plan runs %d units" % plan[2]}))
                continue
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
        status = _lib.status_word(dev)
        stream = _lib.stream_ptr()

        def fwd():
            _lib.check(L.tk_lstm_forward_dev(_lib.ptr(gx), _lib.ptr(w_hh), T, N, H, int(a.reverse), cus, _lib.ptr(y),
                                             _lib.ptr(gates), _lib.ptr(cell), _lib.ptr(ws), wsb, _lib.ptr(status),
                                             stream), "tk_lstm_forward_dev")

        def bwd():
            _lib.check(L.tk_lstm_backward_dev(_lib.ptr(w_hh), _lib.ptr(gates), _lib.ptr(cell), _lib.ptr(dy), T, N, H,
                                              int(a.reverse), cus, _lib.ptr(dg), _lib.ptr(ws), wsb, _lib.ptr(status),
                                              stream), "tk_lstm_backward_dev")

        varlen = {}
        if a.varlen and units is None:
            # include/taiyaki_amd_rnn_varlen.h: five turns each, the forward above and the launch with lengths
            V = _lib.varlen_lib()
            vwsb = V.tk_rnn_varlen_workspace_bytes(_lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"], N, H, cus)
            vws = torch.empty(vwsb // 4, dtype=torch.float32, device=dev)
            lens = torch.full((N,), T, dtype=torch.int32, device=dev)

            def vfwd():
                _lib.check(V.tk_lstm_forward_varlen_dev(_lib.ptr(gx), _lib.ptr(w_hh), _lib.ptr(lens), T, N, H,
                                                        int(a.reverse), cus, _lib.ptr(y), _lib.ptr(vws), vwsb,
                                                        _lib.ptr(status), stream), "tk_lstm_forward_varlen_dev")
            turns = [(timed(fwd, a.steps, a.warmup)[0], timed(vfwd, a.steps, a.warmup)[0]) for _ in range(5)]
            varlen = {"fwd_turns_us_per_step": [round(1e3 * f / T, 3) for f, _ in turns],
                      "varlen_turns_us_per_step": [round(1e3 * v / T, 3) for _, v in turns]}
            # the training pair with lengths: NULL, and half full (its backward on what its own forward saved)
            VT = _lib.varlen_train_lib()
            twsb = VT.tk_rnn_varlen_train_workspace_bytes(_lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"], N, H, cus)
            tws = torch.empty(twsb // 4, dtype=torch.float32, device=dev)
            half = ((torch.arange(N) * T) // max(N - 1, 1)).to(dtype=torch.int32, device=dev)
            y2, gates2, cell2 = torch.empty_like(y), torch.empty_like(gates), torch.empty_like(cell)

            def tfwd(ln, yy, gg, cc):
                _lib.check(VT.tk_lstm_forward_varlen_save_dev(_lib.ptr(gx), _lib.ptr(w_hh), _lib.ptr(ln), T, N, H,
                                                              int(a.reverse), cus, _lib.ptr(yy), _lib.ptr(gg),
                                                              _lib.ptr(cc), _lib.ptr(tws), twsb, _lib.ptr(status),
                                                              stream), "tk_lstm_forward_varlen_save_dev")

            def tbwd(ln, gg, cc):
                _lib.check(VT.tk_lstm_backward_varlen_dev(_lib.ptr(w_hh), _lib.ptr(gg), _lib.ptr(cc), _lib.ptr(dy),
                                                          _lib.ptr(ln), T, N, H, int(a.reverse), cus, _lib.ptr(dg),
                                                          _lib.ptr(tws), twsb, _lib.ptr(status), stream),
                           "tk_lstm_backward_varlen_dev")
            fwd()
            tfwd(half, y2, gates2, cell2)
            legs = {"fwd": fwd, "bwd": bwd, "train_null_fwd": lambda: tfwd(None, y, gates, cell),
                    "train_null_bwd": lambda: tbwd(None, gates, cell),
                    "train_half_fwd": lambda: tfwd(half, y2, gates2, cell2),
                    "train_half_bwd": lambda: tbwd(half, gates2, cell2)}
            tt = [{k: timed(fn, a.steps, a.warmup)[0] for k, fn in legs.items()} for _ in range(5)]
            varlen["train_half_mean_length"] = float(half.float().mean().item())
            varlen["train_turns_us_per_step"] = {k: [round(1e3 * t[k] / T, 3) for t in tt] for k in legs}
        f_med, f_min = timed(fwd, a.steps, a.warmup)
        b_med, b_min = timed(bwd, a.steps, a.warmup)

        # the parameter gradients from that dG, this y and an input of the layer's size
        W = _lib.wgrad_lib()
        wgb = W.tk_lstm_weight_grad_workspace_bytes(T, N, H, H, cus)
        if wgb == 0:
            raise SystemExit("(T, N, H, I) = (%d, %d, %d, %d) has no weight-gradient plan on %d CUs" % (T, N, H, H, cus))
        wws = torch.empty(wgb // 4, dtype=torch.float32, device=dev)
        dw_ih, dw_hh, db = torch.empty(4 * H, H, device=dev), torch.empty(4 * H, H, device=dev), torch.empty(4 * H, device=dev)

        def wgrad():
            _lib.check(W.tk_lstm_weight_grad_dev(_lib.ptr(dg), _lib.ptr(x_in), _lib.ptr(y), T, N, H, H, int(a.reverse),
                                                 cus, _lib.ptr(dw_ih), _lib.ptr(dw_hh), _lib.ptr(db), _lib.ptr(wws), wgb,
                                                 stream), "tk_lstm_weight_grad_dev")

        def wgrad_gemm():
            dg2 = dg.view(T * N, 4 * H)
            dgs, hp = (dg[:-1], y[1:]) if a.reverse else (dg[1:], y[:-1])
            return dg2.t() @ x_in.view(T * N, H), dgs.reshape(-1, 4 * H).t() @ hp.reshape(-1, H), dg2.sum(0)

        w_med, w_min = timed(wgrad, a.steps, a.warmup)
        g_med, g_min = timed(wgrad_gemm, a.steps, a.warmup)
        ref = wgrad_gemm()
        wgrad_diff = max(((p - q).abs().max() / q.abs().max()).item() for p, q in zip((dw_ih, dw_hh, db), ref))
        gflop = 2.0 * T * N * 4 * H * (2 * H + 1) * 1e-9
        proj = proj_report(T, N, H, 4, a.proj_turns, a.steps, a.warmup, dev)
        _lib.finish(status)
        _lib.raise_if_nonfinite()
        if units is not None:
            L.tk_lab_lstm_units(0)
        print(json.dumps({"T": T, "N": N, "H": H, "reverse": a.reverse, "units": units, "cus": cus, **varlen,
                          "fwd_ms": round(f_med, 3), "bwd_ms": round(b_med, 3),
                          "fwd_us_per_step": round(1e3 * f_med / T, 3), "fwd_min_us_per_step": round(1e3 * f_min / T, 3),
                          "bwd_us_per_step": round(1e3 * b_med / T, 3), "bwd_min_us_per_step": round(1e3 * b_min / T, 3),
                          "wgrad_ms": round(w_med, 4), "wgrad_min_ms": round(w_min, 4), "wgrad_gemm_ms": round(g_med, 4),
                          "wgrad_gemm_min_ms": round(g_min, 4), "wgrad_tflops": round(gflop / w_med, 1),
                          "wgrad_gemm_tflops": round(gflop / g_med, 1), "wgrad_vs_gemm_maxrel": wgrad_diff, **proj,
                          "device": torch.cuda.get_device_name(dev)}))
    _lib.use_lab(False)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times one layer's GRU recurrence (csrc/gru_kernels.hip) on the GPU: tk_gru_forward_dev and tk_gru_backward_dev
at (T, N, H), each timed with device events after warm-up; prints one JSON line (microseconds per timestep and
direction, median and min over --steps).  bench.py --config 1's layer is the default shape; the other shape on
record is --T 800 --N 128 --H 256.  The weight-gradient leg follows: `wgrad_ms` is tk_gru_weight_grad_dev
(csrc/gru_wgrad.hip) at (T, N, H, I = H) on that dG, dq and y, `wgrad_gemm_ms` the lines of
layers._gru_grads_from_dgates that it replaces (the batched GEMMs, the sums and the two cats), `--wgrad-turns` times
in turns; `wgrad_vs_gemm_maxrel` is the largest difference between the two relative to a result's largest entry.
The projection legs of tools/lstmbench.py (`proj_ms` / `proj_gemm_ms`, `dx_ms` / `dx_gemm_ms`: csrc/rnn_proj.hip against
the rocBLAS calls it replaces, five alternating turns) come last, at the GRU's three gates.

    python tools/grubench.py [--T 1000] [--N 64] [--H 96] [--steps 20] [--warmup 3] [--reverse] [--infer] [--varlen] [--cols C]
                             [--fallback PAIRS] [--wgrad-turns 3]

--cols (lab build) forces the batch columns per workgroup at H <= 128; without it the release library is timed.

--fallback PAIRS times layers.GruMod(H, H) on one input, forward (grad mode) and backward, PAIRS times in turns: the HIP
recurrence, then nn.GRU (layers.USE_HIP_GRU = False: MIOpen, what a size the kernels refuse runs).  Both sides include
the input GEMM and the weight gradients; one JSON line, microseconds per timestep, in front of the other.

--infer also times the forward with NULL for gates and q (what a torch.no_grad() call launches).

--varlen also times tk_gru_forward_varlen_dev (include/taiyaki_amd_rnn_varlen.h, the release rule) with every length
equal to T, in turns with the forward above, five turns each: the mask's cost per step against the same run's forward
and the spread of that forward between its turns.  It then times the training pair with per-column lengths
(include/taiyaki_amd_rnn_varlen_train.h) the same way, forward and backward, at lengths = NULL and at a half-full
pattern (lengths[n] spread evenly over 0..T), in turns with tk_gru_forward_dev / tk_gru_backward_dev.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, layers  # noqa: E402
from lstmbench import proj_report  # noqa: E402  (tools/ is the script's directory)


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


def layer_turns(T, N, H, pairs, steps, warmup, dev):
    """[(hip fwd, hip bwd, nn.GRU fwd, nn.GRU bwd)] * pairs, median microseconds per timestep."""
    torch.manual_seed(12)
    layer = layers.GruMod(H, H).to(dev)
    x = torch.randn(T, N, H, device=dev).requires_grad_(True)
    dy = torch.randn(T, N, H, device=dev).div_((T * N) ** 0.5)
    if layers.hip_gru_workspace_bytes(layer.rnn, x) == 0:
        raise SystemExit("(N, H) = (%d, %d) is not admitted on %d CUs" % (N, H, layers._cu_count(dev)))

    def one(use_hip):
        layers.USE_HIP_GRU = use_hip
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
        layers.USE_HIP_GRU = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--H", type=int, default=96)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reverse", action="store_true")
    ap.add_argument("--infer", action="store_true", help="also time the forward that saves nothing (gates = q = NULL)")
    ap.add_argument("--varlen", action="store_true", help="also time the forward with per-column lengths, all = T")
    ap.add_argument("--cols", type=int, default=None, help="(lab build) batch columns per workgroup at H <= 128")
    ap.add_argument("--wgrad-turns", type=int, default=3, help="turns of the weight-gradient leg, kernel then GEMMs")
    ap.add_argument("--fallback", type=int, default=0, metavar="PAIRS",
                    help="also time layers.GruMod(H, H) forward and backward, HIP and nn.GRU in turns, PAIRS times")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grubench needs a GPU (the GRU recurrence has no CPU fallback)")
    dev = torch.device("cuda:0")
    T, N, H = a.T, a.N, a.H
    g = torch.Generator(device="cpu").manual_seed(11)
    w_hh = (torch.rand(3 * H, H, generator=g) * 2 - 1).div_(H ** 0.5).to(dev)
    b_hh = torch.zeros(3 * H, device=dev)
    gx = torch.randn(T, N, 3 * H, generator=g).to(dev)
    dy = torch.randn(T, N, H, generator=g).div_((T * N) ** 0.5).to(dev)
    y = torch.empty(T, N, H, device=dev)
    gates = torch.empty(T, N, 3 * H, device=dev)
    q = torch.empty(T, N, H, device=dev)
    dg = torch.empty(T, N, 3 * H, device=dev)
    dq = torch.empty(T, N, H, device=dev)
    cus = layers._cu_count(dev)
    _lib.set_strict(False)
    if a.fallback:
        turns = layer_turns(T, N, H, a.fallback, a.steps, a.warmup, dev)
        keys = ("hip_fwd", "hip_bwd", "nn_gru_fwd", "nn_gru_bwd")
        print(json.dumps({"T": T, "N": N, "H": H, "layer_turns_us_per_step": {k: [round(t[i], 3) for t in turns]
                                                                              for i, k in enumerate(keys)}}))
    L = _lib.use_lab(a.cols is not None)
    if a.cols is not None:
        L.tk_lab_gru_cols(a.cols)
    wsb = L.tk_gru_workspace_bytes(N, H, cus)
    if wsb == 0:
        raise SystemExit("(N, H) = (%d, %d) is not admitted on %d CUs" % (N, H, cus))
    ws = torch.empty(max(wsb // 4, 4), dtype=torch.float32, device=dev)
    status = _lib.status_word(dev)
    stream = _lib.stream_ptr()

    def fwd(save=True):
        _lib.check(L.tk_gru_forward_dev(_lib.ptr(gx), _lib.ptr(w_hh), _lib.ptr(b_hh), T, N, H, int(a.reverse), cus,
                                        _lib.ptr(y), _lib.ptr(gates if save else None), _lib.ptr(q if save else None),
                                        _lib.ptr(ws), wsb, _lib.ptr(status), stream), "tk_gru_forward_dev")

    def bwd():
        _lib.check(L.tk_gru_backward_dev(_lib.ptr(w_hh), _lib.ptr(y), _lib.ptr(gates), _lib.ptr(q), _lib.ptr(dy), T, N,
                                         H, int(a.reverse), cus, _lib.ptr(dg), _lib.ptr(dq), _lib.ptr(ws), wsb,
                                         _lib.ptr(status), stream), "tk_gru_backward_dev")

    out = {"T": T, "N": N, "H": H, "reverse": a.reverse, "cols": a.cols, "cus": cus}
    if a.infer:
        i_med, i_min = timed(lambda: fwd(False), a.steps, a.warmup)
        out.update(infer_ms=round(i_med, 3), infer_us_per_step=round(1e3 * i_med / T, 3),
                   infer_min_us_per_step=round(1e3 * i_min / T, 3))
    if a.varlen:
        V = _lib.varlen_lib()
        vwsb = V.tk_rnn_varlen_workspace_bytes(_lib.VARLEN_DEFINES["TK_RNN_KIND_GRU"], N, H, cus)
        vws = torch.empty(max(vwsb // 4, 4), dtype=torch.float32, device=dev)
        lens = torch.full((N,), T, dtype=torch.int32, device=dev)

        def vfwd():
            _lib.check(V.tk_gru_forward_varlen_dev(_lib.ptr(gx), _lib.ptr(w_hh), _lib.ptr(b_hh), _lib.ptr(lens), T, N, H,
                                                   int(a.reverse), cus, _lib.ptr(y), _lib.ptr(vws), vwsb,
                                                   _lib.ptr(status), stream), "tk_gru_forward_varlen_dev")
        turns = [(timed(fwd, a.steps, a.warmup)[0], timed(vfwd, a.steps, a.warmup)[0]) for _ in range(5)]
        out.update(fwd_turns_us_per_step=[round(1e3 * f / T, 3) for f, _ in turns],
                   varlen_turns_us_per_step=[round(1e3 * v / T, 3) for _, v in turns])
        # the training pair with lengths: NULL, and half full (its backward on what its own forward saved)
        VT = _lib.varlen_train_lib()
        twsb = VT.tk_rnn_varlen_train_workspace_bytes(_lib.VARLEN_DEFINES["TK_RNN_KIND_GRU"], N, H, cus)
        tws = torch.empty(max(twsb // 4, 4), dtype=torch.float32, device=dev)
        half = ((torch.arange(N) * T) // max(N - 1, 1)).to(dtype=torch.int32, device=dev)
        y2, gates2, q2 = torch.empty_like(y), torch.empty_like(gates), torch.empty_like(q)

        def tfwd(lens, yy, gg, qq):
            _lib.check(VT.tk_gru_forward_varlen_save_dev(_lib.ptr(gx), _lib.ptr(w_hh), _lib.ptr(b_hh), _lib.ptr(lens), T,
                                                         N, H, int(a.reverse), cus, _lib.ptr(yy), _lib.ptr(gg),
                                                         _lib.ptr(qq), _lib.ptr(tws), twsb, _lib.ptr(status), stream),
                       "tk_gru_forward_varlen_save_dev")

        def tbwd(lens, yy, gg, qq):
            _lib.check(VT.tk_gru_backward_varlen_dev(_lib.ptr(w_hh), _lib.ptr(yy), _lib.ptr(gg), _lib.ptr(qq),
                                                     _lib.ptr(dy), _lib.ptr(lens), T, N, H, int(a.reverse), cus,
                                                     _lib.ptr(dg), _lib.ptr(dq), _lib.ptr(tws), twsb, _lib.ptr(status),
                                                     stream), "tk_gru_backward_varlen_dev")
        fwd()
        tfwd(half, y2, gates2, q2)
        legs = {"fwd": fwd, "bwd": bwd, "train_null_fwd": lambda: tfwd(None, y, gates, q),
                "train_null_bwd": lambda: tbwd(None, y, gates, q), "train_half_fwd": lambda: tfwd(half, y2, gates2, q2),
                "train_half_bwd": lambda: tbwd(half, y2, gates2, q2)}
        tt = [{k: timed(fn, a.steps, a.warmup)[0] for k, fn in legs.items()} for _ in range(5)]
        out.update(train_half_mean_length=float(half.float().mean().item()),
                   train_turns_us_per_step={k: [round(1e3 * t[k] / T, 3) for t in tt] for k in legs})
    f_med, f_min = timed(fwd, a.steps, a.warmup)
    b_med, b_min = timed(bwd, a.steps, a.warmup)

    # the parameter gradients from that dG, dq and y and an input of the layer's size
    W = _lib.gru_wgrad_lib()
    wgb = W.tk_gru_weight_grad_workspace_bytes(T, N, H, H, cus)
    if wgb == 0:
        raise SystemExit("(T, N, H, I) = (%d, %d, %d, %d) has no weight-gradient plan on %d CUs" % (T, N, H, H, cus))
    x_in = torch.randn(T, N, H, generator=g).to(dev)
    wws = torch.empty(wgb // 4, dtype=torch.float32, device=dev)
    res = [torch.empty(3 * H, H, device=dev), torch.empty(3 * H, H, device=dev), torch.empty(3 * H, device=dev),
           torch.empty(3 * H, device=dev)]

    def wgrad():
        _lib.check(W.tk_gru_weight_grad_dev(_lib.ptr(dg), _lib.ptr(dq), _lib.ptr(x_in), _lib.ptr(y), T, N, H, H,
                                            int(a.reverse), cus, *[_lib.ptr(t) for t in res], _lib.ptr(wws), wgb,
                                            stream), "tk_gru_weight_grad_dev")

    def wgrad_gemm():
        dw_ih = layers._time_sum_tn(dg, x_in)
        sl, hp = (slice(0, T - 1), y[1:]) if a.reverse else (slice(1, T), y[:-1])
        dw_hh = torch.cat([layers._time_sum_tn(dg[sl][:, :, :2 * H], hp), layers._time_sum_tn(dq[sl], hp)])
        db_ih = dg.view(T * N, 3 * H).sum(0)
        return dw_ih, dw_hh, db_ih, torch.cat([db_ih[:2 * H], dq.view(T * N, H).sum(0)])

    turns = [timed(wgrad, a.steps, a.warmup) + timed(wgrad_gemm, a.steps, a.warmup) for _ in range(a.wgrad_turns)]
    ref = wgrad_gemm()
    wgrad_diff = max(((p - r).abs().max() / r.abs().max()).item() for p, r in zip(res, ref))
    out.update(wgrad_ms=[round(t[0], 4) for t in turns], wgrad_min_ms=[round(t[1], 4) for t in turns],
               wgrad_gemm_ms=[round(t[2], 4) for t in turns], wgrad_gemm_min_ms=[round(t[3], 4) for t in turns],
               wgrad_vs_gemm_maxrel=wgrad_diff)
    out.update(proj_report(T, N, H, 3, 5, a.steps, a.warmup, dev))
    _lib.finish(status)
    _lib.raise_if_nonfinite()
    out.update(fwd_ms=round(f_med, 3), bwd_ms=round(b_med, 3), fwd_us_per_step=round(1e3 * f_med / T, 3),
               fwd_min_us_per_step=round(1e3 * f_min / T, 3), bwd_us_per_step=round(1e3 * b_med / T, 3),
               bwd_min_us_per_step=round(1e3 * b_min / T, 3), device=torch.cuda.get_device_name(dev))
    if a.cols is not None:
        L.tk_lab_gru_cols(0)
        _lib.use_lab(False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

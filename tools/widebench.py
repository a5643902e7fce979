#!/usr/bin/env python
"""Times a recurrence on a batch wider than one launch admits (include/taiyaki_amd_rnn_wide.h) beside the admitted
launches it is made of: the wide forward and backward at (T, N, H), and the training pair with per-column lengths
(include/taiyaki_amd_rnn_varlen_train.h, lengths = NULL) at (T, S, H), S the slab width that tk_rnn_wide_slab returns
for the batch, and at the last slab's width.  In --turns alternating turns, each the median of --steps calls timed with
device events; prints one JSON line, microseconds per timestep.  `wide_over_slabs` is the wide call's time over the sum
of its slabs' launches run alone, (slabs - 1) x the full slab's + the last slab's: 1 where cutting costs nothing.

    python tools/widebench.py [--cell lstm|gru] [--T 800] [--N 341] [--H 384] [--reverse] [--turns 3] [--steps 10]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", choices=("lstm", "gru"), default="lstm")
    ap.add_argument("--T", type=int, default=800)
    ap.add_argument("--N", type=int, default=341)
    ap.add_argument("--H", type=int, default=384)
    ap.add_argument("--reverse", action="store_true")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("widebench needs a GPU (the recurrences have no CPU fallback)")
    dev = torch.device("cuda:0")
    T, N, H, lstm = a.T, a.N, a.H, a.cell == "lstm"
    ng = 4 if lstm else 3
    kind = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM" if lstm else "TK_RNN_KIND_GRU"]
    cus = layers._cu_count(dev)
    W, V = _lib.rnn_wide_lib(), _lib.varlen_train_lib()
    S = W.tk_rnn_wide_slab(kind, N, H, cus)
    if not 0 < S < N:
        raise SystemExit("(N, H) = (%d, %d) is one launch on %d CUs, or is not covered (slab %d)" % (N, H, cus, S))
    g = torch.Generator(device="cpu").manual_seed(11)
    w_hh = (torch.rand(ng * H, H, generator=g) * 2 - 1).div_(H ** 0.5).to(dev)
    b_hh = (0.1 * torch.randn(ng * H, generator=g)).to(dev)
    _lib.set_strict(False)
    status, stream, P = _lib.status_word(dev), _lib.stream_ptr(), _lib.ptr

    def legs(lib, fwd_name, bwd_name, n, wsb):
        gx = torch.randn(T, n, ng * H, generator=g).to(dev)
        dy = torch.randn(T, n, H, generator=g).div_((T * n) ** 0.5).to(dev)
        y, gates, c = (torch.empty(T, n, w * H, device=dev) for w in (1, ng, 1))
        dg, dq = torch.empty_like(gates), torch.empty_like(c)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        dims = (T, n, H, int(a.reverse), cus)
        end = (P(ws), wsb, P(status), stream)
        f_in = (P(gx), P(w_hh)) + (() if lstm else (P(b_hh),)) + (None,)
        b_in = (P(w_hh),) + (() if lstm else (P(y),)) + (P(gates), P(c), P(dy), None)
        b_out = (P(dg),) + (() if lstm else (P(dq),))
        return (lambda: _lib.check(getattr(lib, fwd_name)(*f_in, *dims, P(y), P(gates), P(c), *end), fwd_name),
                lambda: _lib.check(getattr(lib, bwd_name)(*b_in, *dims, *b_out, *end), bwd_name))

    wide = legs(W, "tk_%s_forward_wide_dev" % a.cell, "tk_%s_backward_wide_dev" % a.cell, N,
                W.tk_rnn_wide_workspace_bytes(kind, N, H, cus))
    slab = legs(V, "tk_%s_forward_varlen_save_dev" % a.cell, "tk_%s_backward_varlen_dev" % a.cell, S,
                V.tk_rnn_varlen_train_workspace_bytes(kind, S, H, cus))
    k = -(-N // S)
    rest = N - (k - 1) * S
    last = legs(V, "tk_%s_forward_varlen_save_dev" % a.cell, "tk_%s_backward_varlen_dev" % a.cell, rest,
                V.tk_rnn_varlen_train_workspace_bytes(kind, rest, H, cus))
    names = ("slab_fwd", "slab_bwd", "last_fwd", "last_bwd", "wide_fwd", "wide_bwd")
    turns = [[timed(fn, a.steps, a.warmup)[0] for fn in slab + last + wide] for _ in range(a.turns)]
    _lib.raise_if_nonfinite()
    med = {n: float(np.median([t[i] for t in turns])) for i, n in enumerate(names)}
    print(json.dumps({"cell": a.cell, "T": T, "N": N, "H": H, "reverse": a.reverse, "cus": cus, "slab": S, "slabs": k,
                      "last_slab": rest,
                      "turns_us_per_step": {n: [round(1e3 * t[i] / T, 3) for t in turns] for i, n in enumerate(names)},
                      "wide_over_slabs": {d: round(med["wide_" + d] / ((k - 1) * med["slab_" + d] + med["last_" + d]), 3) for d in ("fwd", "bwd")},
                      "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()

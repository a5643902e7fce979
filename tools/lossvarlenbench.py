#!/usr/bin/env python
"""The fused flip-flop loss with a time length per column, timed against the fixed-length operator (run it under
rocprofv3 --kernel-trace --stats for the per-kernel split).

    python tools/lossvarlenbench.py [--reps 40] [--only a|b|c|d] [--out profiles/r38_loss_varlen.txt]
Shape: T 800 x N 128, configs[1]'s lengths (synth.realistic_seqlens at chunk_len 4000, 9 samples per base), plain CRF.
  (a) the existing fused call (ctc.flipflop_mean_loss without lengths)
  (b) the call with lengths = [T] * N: kernel A's VL instantiations, and the one-wave-per-column posterior with lengths in
      kernel B's place
  (c) lengths spread evenly over T/4 .. T, labels of 0.5 T_n bases
  (d) the only route to (c) without the feature: N calls of the existing operator, one per column, on scores[:T_n, n:n+1]
The variants are timed in turns of five calls each, so that clock and thermal drift fall on all of them alike; (d) in turns
of one (a turn of it is N calls).  With each variant: the reads retried and redone in the log domain by one call.

    python tools/lossvarlenbench.py --long
Kernel A alone (the CRF's gradient call) where its launch has four cells per lane and no row maker -- reads beyond 3840
bases, 16 chunk waves: T 5000 x N 32, reads of 3850 .. 3900 bases, 12-step blocks -- without lengths and with lengths =
[T] * N: the instantiations whose VL form spills more than its fixed-length twin."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, ctc, synth  # noqa: E402


def long_reads(args, dev):
    T, N = 5000, 32
    inp = synth.crf_case(T, N, 2, seqlens=np.linspace(3850, 3900, N).astype(np.int32))
    x = torch.from_numpy(inp["scores"]).to(dev)
    seqs, seqlens = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    full = torch.full((N,), T, dtype=torch.int32, device=dev)
    variants = [("a", "kernel A, existing call", lambda: ctc._run(x, seqs, seqlens, 1.0, 1.0, 1.0, 40, True)),
                ("b", "kernel A, lengths = [T] * N", lambda: ctc._run(x, seqs, seqlens, 1.0, 1.0, 1.0, 40, True, lengths=full))]
    counts, outs = {}, {}
    for key, _, fn in variants:
        outs[key] = fn()
        counts[key] = (ctc.last_retry_count(), ctc.last_gate_count())
    same = bool(torch.equal(outs["a"][0], outs["b"][0]) and torch.equal(outs["a"][1], outs["b"][1]))
    _lib.set_strict(False)
    times = {"a": [], "b": []}
    for _ in range(max(1, args.reps // 5)):
        for key, _, fn in variants:
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                times[key].append((a, b))
    torch.cuda.synchronize()
    _lib.raise_if_nonfinite()
    lines = ["kernel A (CRF cost and gradient), plain, T %d x N %d, reads of %d .. %d bases: four cells per lane, 16 chunk waves, no row maker"
             % (T, N, int(inp["seqlens"].min()), int(inp["seqlens"].max()))]
    med = {}
    for key, label, _ in variants:
        us = np.array([a.elapsed_time(b) for a, b in times[key]]) * 1e3
        med[key] = float(np.median(us))
        lines.append("(%s) %-30s calls %3d  median %9.1f us  min %9.1f  max %9.1f   retried %d, redone %d per call" % (
            key, label, len(us), np.median(us), us.min(), us.max(), counts[key][0], counts[key][1]))
    lines.append("(b) / (a) = %.3f; cost and gradient of (b) bit for bit those of (a): %s" % (med["b"] / med["a"], same))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40, help="timed calls per variant, taken in turns of five")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="a | b | c | d: that variant alone (for a per-kernel trace of it)")
    ap.add_argument("--long", action="store_true", help="kernel A at four cells per lane without a row maker, with and without lengths")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.long:
        return long_reads(args, dev)
    T, N = 800, 128
    inp = synth.crf_case(T, N, 1, seqlens=synth.realistic_seqlens(T, N, 17000, 4000, 9.0))
    x = torch.from_numpy(inp["scores"]).to(dev)
    seqs, seqlens = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    # (c): T_n evenly over T/4 .. T, labels of 0.5 T_n
    lens_c = np.linspace(T // 4, T, N).astype(np.int64)
    sl_c = (lens_c // 2).astype(np.int32)
    seqs_c_np, _ = synth.sequences(sl_c, 1)
    seqs_c, seqlens_c = torch.from_numpy(seqs_c_np), torch.from_numpy(sl_c)
    off = np.concatenate([[0], np.cumsum(sl_c)])
    cols = [(x[:int(lens_c[n]), n:n + 1].contiguous(), seqs_c[off[n]:off[n + 1]], seqlens_c[n:n + 1]) for n in range(N)]
    full = torch.full((N,), T, dtype=torch.int32, device=dev)
    lens_c_dev = torch.from_numpy(lens_c.astype(np.int32)).to(dev)

    def per_column():
        for xc, sc, lc in cols:
            ctc._run_fused(xc, sc, lc, 1.0, True, grad_scale=1.0 / N)
    variants = [
        ("a", "existing fused call", 5, lambda: ctc._run_fused(x, seqs, seqlens, 1.0, True, grad_scale=1.0 / N)),
        ("b", "lengths = [T] * N", 5, lambda: ctc._run_fused(x, seqs, seqlens, 1.0, True, grad_scale=1.0 / N, lengths=full)),
        ("c", "T_n over T/4 .. T, labels 0.5 T_n", 5,
         lambda: ctc._run_fused(x, seqs_c, seqlens_c, 1.0, True, grad_scale=1.0 / N, lengths=lens_c_dev)),
        ("d", "N per-column existing calls for (c)", 1, per_column),
    ]
    if args.only:
        variants = [v for v in variants if v[0] == args.only]
    counts = {}
    for key, _, _, fn in variants:          # strict mode: the counts of one call (of (d): summed over its N calls)
        if key == "d":
            r = g = 0
            for xc, sc, lc in cols:
                ctc._run_fused(xc, sc, lc, 1.0, True, grad_scale=1.0 / N)
                r, g = r + ctc.last_retry_count(), g + ctc.last_gate_count()
            counts[key] = (r, g)
        else:
            fn()
            counts[key] = (ctc.last_retry_count(), ctc.last_gate_count())
    _lib.set_strict(False)
    for _, _, _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key, _, _, _ in variants}
    done = 0
    while done < args.reps:
        for key, _, turn, fn in variants:
            for _ in range(turn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                times[key].append((a, b))
        done += 5
    torch.cuda.synchronize()
    _lib.raise_if_nonfinite()
    lines = ["fused flip-flop loss, plain CRF, T %d x N %d, %s; eager calls timed with events on the stream, in turns of five"
             % (T, N, torch.cuda.get_device_name(0)),
             "(a), (b): configs[1]'s lengths (%d .. %d bases); (c), (d): T_n %d .. %d, labels 0.5 T_n" % (
                 int(inp["seqlens"].min()), int(inp["seqlens"].max()), int(lens_c.min()), int(lens_c.max()))]
    stat = {}
    for key, label, _, _ in variants:
        us = np.array([a.elapsed_time(b) for a, b in times[key]]) * 1e3
        stat[key] = float(np.median(us))
        lines.append("(%s) %-38s calls %3d  median %9.1f us  mean %9.1f  min %9.1f  max %9.1f   retried %d, redone %d per call" % (
            key, label, len(us), np.median(us), us.mean(), us.min(), us.max(), counts[key][0], counts[key][1]))
    if not args.only:
        lines.append("(b) / (a) = %.3f    (d) / (c) = %.1f" % (stat["b"] / stat["a"], stat["d"] / stat["c"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

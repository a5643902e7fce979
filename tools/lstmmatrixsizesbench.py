#!/usr/bin/env python
"""Times one `layers.Lstm` at hidden size --size (384 or 192) under no_grad on the matrix cores
(csrc/lstm_matrix_sizes.hip: groups of size / 32 workgroups, slabs inside the entry) against what runs the same call
with the switch off: the saving forward of the main library, beyond 128 columns at 384 and 512 at 192 as slabs
(csrc/lstm_kernels.hip).

For every (T, N) of --shapes, with full lengths (none given) and with lengths spread evenly over T/4 ... T, and for
every built number of column sets per group (--sets: 1 at 384, 1 or 2 at 192; the lab build reads TK_LAB_LSTM_MATRIX_SIZES_M per call): the layer
with the switch on (threshold 1, lab build) and off (release build) in turns in one process, each timed with device
events after warm-up (median over --steps), --turns turns.  Both sides include the layer's input projection.  One JSON
line per case: microseconds per call and turn, whether the new kernel was ahead in EVERY turn, and the largest
difference of the two outputs.  Then one JSON line per number of sets with the threshold the table sets: the smallest
measured N from which the new kernel is ahead in every turn, there and at every larger N measured, at every T and with
both kinds of lengths (null: there is none).

--basecall: one whole `Basecaller.call` on a seeded mLstm_flipflop of size --size on the reads of tools/basecallbench.py at
max_concurrent_chunks 2048 and 4096, with layers.USE_HIP_LSTM_MATRIX_SIZES off and on in turns (release build, the
threshold as shipped unless --min-columns): samples per second, reads with equal calls, largest score difference of the
network pass on the first batch.

    python tools/lstmmatrixsizesbench.py [--size 384] [--shapes 800x256,...] [--sets 1] [--steps 5] [--warmup 2] [--turns 3]
    python tools/lstmmatrixsizesbench.py --basecall [--size 384] [--reads 384] [--min-columns 257]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, layers  # noqa: E402

SHAPES = ",".join("%dx%d" % (800, N) for N in (256, 512, 1024, 2048, 4096, 8192))


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


def side(on, sets, H):
    """The process on the new row (lab build, `sets` column sets per group, every width) or where the parent runs."""
    _lib.use_lab(on)
    os.environ["TK_LAB_LSTM_MATRIX_SIZES_M"] = str(sets)
    layers.USE_HIP_LSTM_MATRIX_SIZES = on
    layers.LSTM_MATRIX_SIZES_MIN_COLUMNS = {H: 1}


def layer_turns(H, T, N, spread, sets, turns, steps, warmup, dev):
    torch.manual_seed(11)
    lstm = layers.Lstm(H, H).to(dev)
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(T, N, H, generator=g, device=dev)
    lens = None
    if spread:
        lens = torch.linspace(T // 4, T, N, device=dev).round().to(torch.int32)[torch.randperm(N, generator=g, device=dev)]
        lens = lens.contiguous()
    out, ys = {"group": [], "parent": []}, {}

    def run(k):
        with torch.no_grad():
            ys[k] = lstm(x, lengths=lens)

    for _ in range(turns):
        for k in out:
            side(k == "group", sets, H)
            before = layers.lstm_matrix_sizes_calls["inference"]
            out[k].append(round(1e3 * timed(lambda: run(k), steps, warmup), 1))
            assert (layers.lstm_matrix_sizes_calls["inference"] > before) == (k == "group")
    return {"H": H, "T": T, "N": N, "sets": sets, "lengths": "spread" if spread else "full", "us_per_call": out,
            "us_per_step_median": {k: round(float(np.median(v)) / T, 3) for k, v in out.items()},
            "group_ahead_every_turn": all(a < b for a, b in zip(out["group"], out["parent"])),
            "max_abs_diff": (ys["group"] - ys["parent"]).abs().max().item()}


def basecall_turns(H, turns, reads, min_columns, dev):
    from taiyaki_amd import basecall, models, synth
    rs = np.random.RandomState(9)
    sigs = [(90 + 12 * rs.standard_normal(int(n))).astype(np.float32) for n in rs.randint(20000, 100001, size=reads)]
    torch.manual_seed(17)
    net = synth.excite_network(models.mLstm_flipflop(size=H)).to(dev).eval()
    if min_columns:
        layers.LSTM_MATRIX_SIZES_MIN_COLUMNS = dict(layers.LSTM_MATRIX_SIZES_MIN_COLUMNS, **{H: min_columns})
    nsamples = sum(len(s) for s in sigs)
    shipped = layers.USE_HIP_LSTM_MATRIX_SIZES
    rows = []
    try:
        for concurrent in (2048, 4096):
            caller = basecall.Basecaller(net, fastq=True, max_concurrent_chunks=concurrent)
            out, calls, seqs, scores = {"off": [], "on": []}, {}, {}, {}
            x = torch.randn(1000, concurrent, 1, generator=torch.Generator().manual_seed(3)).to(dev)
            for turn in range(turns + 1):           # (the first turn is the warm-up at the timed shapes)
                for k in out:
                    layers.USE_HIP_LSTM_MATRIX_SIZES = k == "on"
                    before = layers.lstm_matrix_sizes_calls["inference"]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = caller.call(sigs)         # (ends in its download)
                    dt = time.perf_counter() - t0
                    calls[k] = layers.lstm_matrix_sizes_calls["inference"] - before
                    seqs[k] = [r[0] for r in res]
                    if turn:
                        out[k].append(round(nsamples / dt))
                    else:
                        with torch.no_grad():
                            scores[k] = net(x)
            same = sum(a == b for a, b in zip(seqs["off"], seqs["on"]))
            rows.append({"basecall": "mLstm_flipflop %d, %d reads, %d samples, max_concurrent_chunks %d"
                                     % (H, len(sigs), nsamples, concurrent),
                         "min_columns": layers.LSTM_MATRIX_SIZES_MIN_COLUMNS[H], "samples_per_s": out,
                         "group_launches_per_call": calls, "reads_with_equal_calls": "%d / %d" % (same, len(sigs)),
                         "bases": sum(len(s) for s in seqs["on"]),
                         "max_score_diff": (scores["on"] - scores["off"]).abs().max().item(),
                         "max_score": scores["off"].abs().max().item()})
    finally:
        layers.USE_HIP_LSTM_MATRIX_SIZES = shipped
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=384, choices=(192, 384))
    ap.add_argument("--shapes", default=SHAPES, help="T x N, comma separated")
    ap.add_argument("--sets", default="", help="column sets per group, comma separated (default: every built one)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--basecall", action="store_true")
    ap.add_argument("--reads", type=int, default=384)
    ap.add_argument("--min-columns", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstmmatrixsizesbench needs a GPU (the recurrence has no CPU fallback)")
    dev = torch.device("cuda:0")
    if a.basecall:
        for row in basecall_turns(a.size, a.turns, a.reads, a.min_columns, dev):
            print(json.dumps(row), flush=True)
        return
    for sets in (int(v) for v in (a.sets or ("1" if a.size == 384 else "1,2")).split(",")):
        ahead = {}
        for shape in a.shapes.split(","):
            T, N = (int(v) for v in shape.split("x"))
            for spread in (False, True):
                row = layer_turns(a.size, T, N, spread, sets, a.turns, a.steps, a.warmup, dev)
                ahead[N] = ahead.get(N, True) and row["group_ahead_every_turn"]
                print(json.dumps(row), flush=True)
        widths = sorted(ahead)
        from_n = [n for i, n in enumerate(widths) if all(ahead[m] for m in widths[i:])]
        print(json.dumps({"device": torch.cuda.get_device_name(dev), "cus": layers._cu_count(dev), "H": a.size, "sets": sets,
                          "ahead_at_every_T_and_lengths": ahead, "threshold": from_n[0] if from_n else None}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times the squiggle trainer's batches at bin/train_squiggle.py's defaults: 100 chunks of 300 bases, from 200 synthetic
reads of about 1500 bases (fixed seeds).  Two producers of the same batch, measured in turns in one process:

  device   `MappedSignalStore.sample_sequence_chunks`: locate + select + gather on the resident store
  host     the reference's loop, stood in for by the numpy restatement per chunk (tests/chunks_seqlen_support.py),
           np.concatenate and three uploads, on the candidates the device batch was drawn with

(a) one device batch, (b) one host batch, (c) a whole `SquiggleTrainer.step` fed by each.  (a) is timed twice: with
device events around the call (what the GPU spends) and by the host clock around the call and a synchronise (what a
loop that waited for the batch would see); (b) and (c) by the host clock, ending in a synchronise.  The gather launch
alone is timed with device events over `--inner` back-to-back launches, against the store's 6 B per sample
(int16 in, float32 out) plus the sequence arrays' bytes.  Medians over --steps after --warmup; one JSON line last.

    python tools/squigglechunkbench.py [--steps 30] [--warmup 5] [--chunks 100] [--bases 300] [--reads 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from taiyaki_amd import _lib, mapped_signal as ms, models, synth, train  # noqa: E402
from tests import chunks_seqlen_support as support  # noqa: E402


def host_batch(reads, regions, fpd, cand_read, cand_start, nwant, bases, dev):
    """The reference's per-chunk loop, concatenation and upload (bin/train_squiggle.py:188-209)."""
    chunks, _, _ = support.sample_chunks(reads, nwant, bases, fpd, zip(cand_read, cand_start))
    seq_embed, signal, siglens, _ = support.assemble_batch(chunks)
    return (torch.from_numpy(seq_embed).to(dev), torch.from_numpy(signal).to(dev), torch.from_numpy(siglens).to(dev))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn, inner=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=100)
    ap.add_argument("--bases", type=int, default=300)
    ap.add_argument("--reads", type=int, default=200)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("squigglechunkbench needs a GPU (the chunk kernels have no CPU fallback)")
    dev = torch.device("cuda:0")
    _lib.set_strict(False)          # as a training loop runs: status words are read once, at the end
    reads = synth.mapped_reads(a.reads, 181, mean_reflen=1500, long_dwell_prob=0.002)
    store = ms.MappedSignalStore(reads, dev)
    regions = store.mapped_ref
    torch.manual_seed(1)
    N, B = a.chunks, a.bases
    fp = store.sample_filter_parameters(1000, B, 3.0, 10.0, 0.5, 1, 1.1, chunk_len_means_sequence_len=True)
    fpd = dict(fp._asdict())
    net = models.squiggle_predictor(32, 4, 9).to(dev)
    trainer = train.SquiggleTrainer(net)

    # the candidates of one device batch, read back: both producers assemble these
    b = store.sample_sequence_chunks(N, B, fp)
    cand_read = b.cand_read.cpu().numpy()
    lo = regions[cand_read, 0]
    spare = regions[cand_read, 1] - lo - B
    cand_start = np.where(spare > 0, b.refstart.cpu().numpy() - lo, 0)
    cands = (cand_read, cand_start)
    n, total = b.naccepted, int(b.sigoff[-1])
    got, want = b.trimmed(), host_batch(reads, regions, fpd, cand_read, cand_start, N, B, dev)
    assert all(torch.equal(g, w.to(g.dtype)) for g, w in zip(got, want)), "the two producers disagree"

    device_batch = lambda: store.sample_sequence_chunks(N, B, fp, candidates=cands)                        # noqa: E731
    device_drawn = lambda: store.sample_sequence_chunks(N, B, fp)                                           # noqa: E731
    host_chain = lambda: host_batch(reads, regions, fpd, cand_read, cand_start, N, B, dev)                  # noqa: E731
    runs = {
        "a_device_batch_events_ms": lambda: events(device_batch)[0],
        "a_device_batch_wall_ms": lambda: wall(device_batch)[0],
        "a_device_batch_drawn_on_device_wall_ms": lambda: wall(device_drawn)[0],
        "b_host_chain_wall_ms": lambda: wall(host_chain)[0],
        "c_step_device_fed_wall_ms": lambda: wall(lambda: trainer.step(device_batch()))[0],
        "c_step_host_fed_wall_ms": lambda: wall(lambda: trainer.step(host_chain()))[0],
        "step_alone_wall_ms": lambda: wall(lambda: trainer.step(got))[0],
    }
    times = {k: [] for k in runs}
    for i in range(a.warmup + a.steps):         # in turns: every pass runs every leg once
        for k, fn in runs.items():
            t = fn()
            if i >= a.warmup:
                times[k].append(t)

    # the gather launch alone, on the located and selected candidates of that batch
    cr = torch.from_numpy(cand_read.astype(np.int32)).to(dev)
    cs = torch.from_numpy(cand_start.astype(np.int32)).to(dev)
    loc = store._locate_sequence(cr, cs, None, B, fp)
    sel, sigoff, counts = store._select(loc, N, "siglen")
    cap = N * ms.sequence_chunk_sample_bound(B, fp)
    gather = lambda: store._gather_sequence(cr, loc, sel, sigoff, counts, N, B, cap, False, True)          # noqa: E731
    gtimes = []
    for i in range(a.warmup + a.steps):
        t = events(gather, a.inner)[0]
        if i >= a.warmup:
            gtimes.append(t)
    gather_ms = float(np.median(gtimes))
    moved = 6 * total + 4 * (cap - total) + n * B * 2 + N * B * 16 + N * 4      # samples in and out, zero fill, bases in, seqs and seq_embed out, siglens

    _lib.raise_if_nonfinite()
    out = {"chunks": N, "bases": B, "reads": a.reads, "accepted": n, "samples": total, "signal_capacity": cap,
           "steps": a.steps, "device": torch.cuda.get_device_name(dev)}
    for k, v in times.items():
        out[k] = round(float(np.median(v)), 3)
        out[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 3)
    out["gather_launch_events_us"] = round(gather_ms * 1e3, 2)
    out["gather_bytes"] = int(moved)
    out["gather_GB_per_s"] = round(moved / (gather_ms * 1e-3) / 1e9, 1)
    out["gather_GB_per_s_store_bytes_only"] = round(6 * total / (gather_ms * 1e-3) / 1e9, 1)
    print("squiggle chunk batches: %d chunks x %d bases from %d reads; %d accepted, %d samples (capacity %d)"
          % (N, B, a.reads, n, total, cap))
    for k in times:
        print("  %-42s median %9.3f   min %9.3f" % (k, out[k], out[k.replace("_ms", "_min_ms")]))
    print("  gather launch alone (events, %d back to back): %.2f us; %d bytes -> %.1f GB/s (%.1f GB/s counting the "
          "store's 6 B per sample only)" % (a.inner, gather_ms * 1e3, moved, out["gather_GB_per_s"],
                                            out["gather_GB_per_s_store_bytes_only"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

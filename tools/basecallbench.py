#!/usr/bin/env python
"""Times the basecaller's tail two ways on the same inputs, and a whole `Basecaller.call`.

The tail, at --chunks 128 x --blocks 1000, stride 5, overlap 100 blocks (the reference's default
max_concurrent_chunks and chunk_size), on Viterbi paths and error probabilities of `synth.confident_scores`:
  device   tk_basecall_call_dev (stitch, collapse, quality characters) plus its ONE download of seq, qual, seqlen
  host     the chain this repository had before: `.cpu()` of path and error probabilities, `stitch_chunks`,
           `path_to_str`, `path_errprobs_to_qstring`, per read
Both produce every read's sequence and quality string; they are compared before anything is timed.  Each side is
warmed up, then timed --steps times with a host clock around work that ends in a synchronising copy, the two sides
alternating; median and min are printed.

The whole call: reads/s and samples/s of `Basecaller.call` (fastq, posterior) on a seeded mGru_flipflop and
mLstm_flipflop for --reads reads of 20 000 - 100 000 samples.  Prints one JSON line.

--beam WIDTH adds a row per model: a whole `Basecaller.call` with beam=(WIDTH, guided) -- every read's stitched scores
through ONE launch of the beam search -- at 1, 8 and 64 of those reads, beside the same reads through the per-read
chain the operators allowed before (chunk_read, the network, `stitch_chunks` of the scores, one `decodeutil.beamsearch`
launch and its downloads per read, `path_to_str`).  Both split the network's invocations per read (pack=False), so
their calls are equal (compared first; a mismatch ends the run).  The two sides alternate --beam-steps times after one
warm-up each.  Median, min and max per side: the spread is that of the alternated runs themselves.

--mods times, instead of all the above, modified-base calling on a seeded size-256 mLstm_cat_mod_flipflop (excited so
that it calls bases) at 1, 8 and 64 of those reads, three sides alternating --mods-steps times after one warm-up each,
each ending in its downloads:
  call_mods  `Basecaller(mod_output=True).call_mods`: calls and modified-base scores, one download
  call       `Basecaller.call` on the same model: the calls alone
  chain      what the operators allowed before: per read chunk_read, the network, posterior, the Viterbi, a download
             of paths and categorical columns, then `stitch_chunks`, `path_to_str` and the numpy
             extract_mod_weights on the host
All at pack=False, so the three sides give equal calls and call_mods and chain equal scores (compared first, bit for
bit; a mismatch ends the run).  Prints one JSON line.

--short times, instead of all the above, batches of 1, 8 and 64 reads of 300 - 4 900 samples (every one shorter than
a chunk) on the two seeded models, excited so that they call bases: whole calls ending in their downloads, with
batch_short=False (a network pass and three or four decode launches per read) against batch_short=True (the reads as
padded columns of one tensor), alternating --short-steps times after one warm-up each.  Checked first: both sides
report every read's sample count and well-formed records (the sequences may differ where the network's GEMMs round
differently at another column count; how many are equal is reported).  Prints one JSON line.

    python tools/basecallbench.py [--chunks 128] [--blocks 1000] [--reads-per-batch 8] [--steps 20] [--warmup 3]
                                  [--beam 5] [--beam-steps 5] [--mods] [--mods-steps 5] [--short] [--short-steps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, basecall, basecall_helpers, clipping, decode, decodeutil, flipflopfings, models, qscores, synth  # noqa: E402

STRIDE, OVERLAP_BLOCKS = 5, 100


def stats(times):
    return dict(median_us=round(1e6 * float(np.median(times)), 1), min_us=round(1e6 * float(np.min(times)), 1))


def chain_call(sigs, net, stride, width, guided, dev, chunk_blocks=1000, overlap_blocks=100, concurrent=128):
    """bin/basecall.py:151-221 with a beam, read by read, on the operators this package had before the batched path."""
    out = []
    for x in sigs:
        med, mad = clipping.med_mad(x)
        if not mad > 0:                                                         # (Basecaller's answer for such a read)
            out.append(("", None, len(x)))
            continue
        chunks, starts, ends = basecall_helpers.chunk_read(((x - med) / mad).astype("f4"), chunk_blocks * stride,
                                                           overlap_blocks * stride)
        with torch.no_grad():
            chunks = torch.tensor(chunks, device=dev)
            trans = torch.cat([net(c.contiguous())[:, :, :40] for c in torch.split(chunks, concurrent, 1)], 1)
            trans = (decode.flipflop_make_trans(trans) + 1e-8).log()
            stitched = basecall_helpers.stitch_chunks(trans, starts, ends, stride).contiguous()
            best, _ = decodeutil.beamsearch(stitched, 0.0, width, guided)       # one launch, three downloads
        out.append((flipflopfings.path_to_str(best, include_first_source=False), None, len(x)))
    return out


def beam_rows(net, sigs, width, steps, dev):
    """{reads: timings} of the batched beam call and of the per-read chain on sigs[:reads], alternating."""
    caller = basecall.Basecaller(net, beam=(width, True), pack=False)
    rows = {}
    for nread in (1, 8, 64):
        batch = sigs[:nread]
        sides = dict(batched=lambda: caller.call(batch),
                     chain=lambda: chain_call(batch, net, caller.stride, width, True, dev))
        first = {k: fn() for k, fn in sides.items()}                           # (the warm-up at the timed shapes)
        same = sum(a == b for a, b in zip(first["batched"], first["chain"]))
        if same != len(batch):
            raise SystemExit("basecallbench --beam: %d of %d reads have the same call on both sides; nothing timed"
                             % (same, len(batch)))
        times = {k: [] for k in sides}
        for _ in range(steps):
            for k, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                                                            # ends in a download
                times[k].append(time.perf_counter() - t0)
        blocks = [len(x) // caller.stride for x in batch]
        row = dict(reads=len(batch), blocks_longest=max(blocks), blocks_total=sum(blocks),
                   bases=sum(len(r[0]) for r in first["batched"]),
                   reads_with_equal_calls=same)
        for k, t in times.items():
            row[k] = dict(median_ms=round(1e3 * float(np.median(t)), 2), min_ms=round(1e3 * float(np.min(t)), 2),
                          max_ms=round(1e3 * float(np.max(t)), 2), reads_per_s=round(len(batch) / float(np.median(t)), 2))
        row["chain_over_batched"] = round(float(np.median(times["chain"]) / np.median(times["batched"])), 2)
        rows[str(nread)] = row
    return rows


def host_extract_mod_weights(mod_weights, path, can_nmods):
    """flipflopfings.py:100-143 in numpy, without its NaN row 0: what a user ran on the host, per read."""
    move = np.flatnonzero(path[1:] != path[:-1]) + 1
    base = path[move] % len(can_nmods)
    out = np.full((len(move), int(sum(can_nmods))), np.nan, dtype=np.float32)
    col = off = 0
    for b, n in enumerate(can_nmods):
        for m in range(n):
            out[base == b, col] = mod_weights[move[base == b] - 1, off + 1 + m]
            col += 1
        off += 1 + n
    return out


def chain_mods(sigs, net, stride, can_nmods, dev, chunk_blocks=1000, overlap_blocks=100, concurrent=128):
    """bin/basecall.py:151-242 read by read on the operators this package had before call_mods, plus the host's
    extract_mod_weights on the downloaded paths and categorical columns."""
    calls, mods = [], []
    for x in sigs:
        med, mad = clipping.med_mad(x)
        chunks, starts, ends = basecall_helpers.chunk_read(((x - med) / mad).astype("f4"), chunk_blocks * stride,
                                                           overlap_blocks * stride)
        with torch.no_grad():
            chunks = torch.tensor(chunks, device=dev)
            out = torch.cat([net(c.contiguous()) for c in torch.split(chunks, concurrent, 1)], 1)
            trans = (decode.flipflop_make_trans(out[:, :, :40].contiguous()) + 1e-8).log()
            path = decode.flipflop_viterbi_path(trans)
            err = qscores.errprobs_from_trans(trans, path)
            p, e, w = path.cpu(), err.cpu(), out[:, :, 40:].cpu()              # the downloads (synchronise)
        sp = basecall_helpers.stitch_chunks(p, starts, ends, stride).numpy()
        se = basecall_helpers.stitch_chunks(e, starts, ends, stride)
        sw = basecall_helpers.stitch_chunks(w, starts, ends, stride).numpy()
        calls.append((flipflopfings.path_to_str(sp, include_first_source=False),
                      qscores.path_errprobs_to_qstring(se, sp, 1.0, 0.0), len(x)))
        mods.append(host_extract_mod_weights(sw, sp, can_nmods))
    return calls, mods


def same_bits(a, b):
    nan = np.isnan(b)
    return (a.shape == b.shape and np.array_equal(np.isnan(a), nan) and
            np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def mods_rows(size, steps, dev):
    can_nmods = (1, 1, 0, 0)
    rs = np.random.RandomState(9)
    sigs = [(90 + 12 * rs.standard_normal(int(n))).astype(np.float32) for n in rs.randint(20000, 100001, size=64)]
    torch.manual_seed(17)
    net = synth.excite_network(models.mLstm_cat_mod_flipflop(size=size, can_nmods=can_nmods)).to(dev).eval()
    caller = basecall.Basecaller(net, fastq=True, pack=False, mod_output=True)
    plain = basecall.Basecaller(net, fastq=True, pack=False)
    rows = {}
    for nread in (1, 8, 64):
        batch = sigs[:nread]
        sides = dict(call_mods=lambda: caller.call_mods(batch), call=lambda: (plain.call(batch), None),
                     chain=lambda: chain_mods(batch, net, caller.stride, can_nmods, dev))
        first = {k: fn() for k, fn in sides.items()}                           # (the warm-up at the timed shapes)
        seqs = {k: [r[0] for r in v[0]] for k, v in first.items()}
        if not seqs["call_mods"] == seqs["call"] == seqs["chain"]:
            raise SystemExit("basecallbench --mods: the three sides disagree on a call; nothing timed")
        if not all(same_bits(a, b) for a, b in zip(first["call_mods"][1], first["chain"][1])):
            raise SystemExit("basecallbench --mods: call_mods and the host chain disagree on a score; nothing timed")
        times = {k: [] for k in sides}
        for _ in range(steps):
            for k, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                                                            # ends in its downloads
                times[k].append(time.perf_counter() - t0)
        bases = sum(len(s) for s in seqs["call"])
        row = dict(reads=nread, samples=int(sum(map(len, batch))), bases=bases,
                   mods_bytes_in_download=4 * bases * int(sum(can_nmods)))
        for k, t in times.items():
            row[k] = dict(median_ms=round(1e3 * float(np.median(t)), 2), min_ms=round(1e3 * float(np.min(t)), 2),
                          max_ms=round(1e3 * float(np.max(t)), 2), reads_per_s=round(nread / float(np.median(t)), 2))
        row["call_mods_minus_call_ms"] = round(1e3 * float(np.median(times["call_mods"]) - np.median(times["call"])), 2)
        row["chain_over_call_mods"] = round(float(np.median(times["chain"]) / np.median(times["call_mods"])), 2)
        rows[str(nread)] = row
    return dict(model="mLstm_cat_mod_flipflop", size=size, stride=caller.stride, can_nmods=list(can_nmods), steps=steps,
                pack=False, rows=rows)


def short_rows(size, steps, dev):
    rs = np.random.RandomState(19)
    sigs = [(90 + 12 * rs.standard_normal(int(n))).astype(np.float32) for n in rs.randint(300, 4901, size=64)]
    out = {}
    for name, make in (("mGru_flipflop", models.mGru_flipflop), ("mLstm_flipflop", models.mLstm_flipflop)):
        torch.manual_seed(17)
        net = synth.excite_network(make(size=size)).to(dev).eval()
        callers = {k: basecall.Basecaller(net, fastq=True, batch_short=v) for k, v in (("alone", False), ("batched", True))}
        rows = {}
        for nread in (1, 8, 64):
            batch = sigs[:nread]
            sides = {k: (lambda c=c: c.call(batch)) for k, c in callers.items()}
            first = {k: fn() for k, fn in sides.items()}                       # (the warm-up at the timed shapes)
            for k, res in first.items():
                if [r[2] for r in res] != [len(x) for x in batch] or not all(
                        len(q) == len(s) and set(s) <= set("ACGT") for s, q, _ in res):
                    raise SystemExit("basecallbench --short: %s gives a malformed record; nothing timed" % k)
            same = sum(a[0] == b[0] for a, b in zip(first["alone"], first["batched"]))
            times = {k: [] for k in sides}
            for _ in range(steps):
                for k, fn in sides.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()                                                        # ends in its download
                    times[k].append(time.perf_counter() - t0)
            row = dict(reads=nread, samples=int(sum(map(len, batch))), samples_longest=int(max(map(len, batch))),
                       bases=sum(len(r[0]) for r in first["batched"]), reads_with_equal_sequences=same)
            for k, t in times.items():
                row[k] = dict(median_ms=round(1e3 * float(np.median(t)), 2), min_ms=round(1e3 * float(np.min(t)), 2),
                              max_ms=round(1e3 * float(np.max(t)), 2), reads_per_s=round(nread / float(np.median(t)), 2))
            row["alone_over_batched"] = round(float(np.median(times["alone"]) / np.median(times["batched"])), 2)
            rows[str(nread)] = row
        out[name] = dict(size=size, stride=callers["alone"].stride, steps=steps, rows=rows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=1000)
    ap.add_argument("--reads-per-batch", type=int, default=8, help="reads the tail's chunks are split into")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=32, help="reads of the whole-call measurement")
    ap.add_argument("--size", type=int, default=256, help="layer size of the two models")
    ap.add_argument("--beam", type=int, default=0, metavar="WIDTH",
                    help="also time a whole call with beam=(WIDTH, guided) at 1, 8, 64 reads beside the per-read chain")
    ap.add_argument("--beam-steps", type=int, default=5)
    ap.add_argument("--mods", action="store_true",
                    help="time call_mods, call and the host chain on a cat-mod model at 1, 8, 64 reads (nothing else)")
    ap.add_argument("--mods-steps", type=int, default=5)
    ap.add_argument("--short", action="store_true",
                    help="time batch_short False against True at 1, 8, 64 reads shorter than a chunk (nothing else)")
    ap.add_argument("--short-steps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("basecallbench needs a GPU (the basecaller has no CPU fallback)")
    dev = torch.device("cuda:0")
    if a.mods:
        print(json.dumps(dict(mods=mods_rows(a.size, a.mods_steps, dev))))
        return
    if a.short:
        print(json.dumps(dict(short=short_rows(a.size, a.short_steps, dev))))
        return
    L = _lib.basecall_lib()
    T, N = a.blocks, a.chunks
    chunk, overlap = T * STRIDE, OVERLAP_BLOCKS * STRIDE

    # ---- the tail's inputs: the chunks of `reads-per-batch` reads, paths and error probabilities from the decode kernels
    per = np.full(a.reads_per_batch, N // a.reads_per_batch)
    per[:N % a.reads_per_batch] += 1
    lens = [chunk + (int(k) - 1) * (chunk - overlap) - 137 * (int(k) > 1) for k in per]
    geo = [basecall_helpers.chunk_bounds(n, chunk, overlap) for n in lens]
    assert [len(g[0]) for g in geo] == list(per)
    rco = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    starts_h, ends_h = (np.concatenate([g[i] for g in geo]).astype(np.int64) for i in (0, 1))
    seqlens = (T * (0.35 + 0.2 * np.random.RandomState(5).uniform(size=N))).astype(np.int32)
    scores = torch.from_numpy(synth.confident_scores(synth.crf_case(T, N, 5, seqlens=seqlens), 6, on=2.0, off=-1.0)["scores"]).to(dev)
    trans = decode.flipflop_make_trans(scores)
    path = decode.flipflop_viterbi_path(scores)
    err = qscores.errprobs_from_trans(trans, path)
    rows = [basecall.stitched_rows(int(k), n, chunk, overlap, STRIDE, T + 1) for k, n in zip(per, lens)]
    out_off_h = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    cap, nread = int(out_off_h[-1]), len(lens)
    starts, ends, rco_d, out_off = (torch.from_numpy(x).to(dev) for x in (starts_h, ends_h, rco, out_off_h))
    o_seq = basecall._align(4 * nread)
    buf = torch.zeros(o_seq + 2 * basecall._align(cap), dtype=torch.uint8, device=dev)
    seqlen, seq, qual = buf[:4 * nread].view(torch.int32), buf[o_seq:o_seq + cap], buf[o_seq + basecall._align(cap):]

    def device_tail():
        _lib.check(L.tk_basecall_call_dev(
            _lib.ptr(path), _lib.ptr(err), T, N, _lib.ptr(starts), _lib.ptr(ends), _lib.ptr(rco_d), None, nread, STRIDE, 4,
            b"ACGT", 1.0, 0.0, _lib.ptr(out_off), _lib.ptr(seq), _lib.ptr(qual), _lib.ptr(seqlen), None, _lib.stream_ptr()),
            "tk_basecall_call_dev")
        got = buf.cpu().numpy()                                 # the one download (synchronises)
        n = got[:4 * nread].view(np.int32)
        q0 = o_seq + basecall._align(cap)
        return [(got[o_seq + out_off_h[r]:o_seq + out_off_h[r] + n[r]].tobytes().decode(),
                 got[q0 + out_off_h[r]:q0 + out_off_h[r] + n[r]].tobytes().decode()) for r in range(nread)]

    def host_tail():
        p, e = path.cpu(), err.cpu()                            # (synchronises)
        out = []
        for r in range(nread):
            c0, c1 = int(rco[r]), int(rco[r + 1])
            sp = basecall_helpers.stitch_chunks(p[:, c0:c1], starts_h[c0:c1], ends_h[c0:c1], STRIDE).numpy()
            se = basecall_helpers.stitch_chunks(e[:, c0:c1], starts_h[c0:c1], ends_h[c0:c1], STRIDE)
            out.append((flipflopfings.path_to_str(sp, include_first_source=False),
                        qscores.path_errprobs_to_qstring(se, sp, 1.0, 0.0)))
        return out

    dres, hres = device_tail(), host_tail()
    assert [d[0] for d in dres] == [h[0] for h in hres], "device and host tails disagree on a sequence"
    qdiff = sum(x != y for d, h in zip(dres, hres) for x, y in zip(d[1], h[1]))
    for _ in range(a.warmup):
        device_tail()
        host_tail()
    times = {"device": [], "host": []}
    for _ in range(a.steps):                                    # alternating, same process, same inputs
        for name, fn in (("device", device_tail), ("host", host_tail)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    rec = dict(tail=dict(chunks=N, blocks=T, stride=STRIDE, overlap_blocks=OVERLAP_BLOCKS, reads=nread,
                         bases=sum(len(d[0]) for d in dres), quality_characters_differing=qdiff,
                         device_with_download=stats(times["device"]), host_chain=stats(times["host"]),
                         host_over_device=round(float(np.median(times["host"]) / np.median(times["device"])), 2)))

    # ---- the whole call
    rs = np.random.RandomState(9)
    sigs = [(90 + 12 * rs.standard_normal(int(n))).astype(np.float32)
            for n in rs.randint(20000, 100001, size=max(a.reads, 64 if a.beam else 0))]
    beam_sigs, sigs = sigs, sigs[:a.reads]
    for name, make in (("mGru_flipflop", models.mGru_flipflop), ("mLstm_flipflop", models.mLstm_flipflop)):
        torch.manual_seed(17)
        net = make(size=a.size).to(dev).eval()
        caller = basecall.Basecaller(net, fastq=True)
        caller.call(sigs[:2])
        caller.call(sigs)                                       # warm-up at the timed shapes
        torch.cuda.synchronize()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = caller.call(sigs)                             # ends in its download
            wall.append(time.perf_counter() - t0)
        t = float(np.median(wall))
        rec[name] = dict(size=a.size, stride=caller.stride, reads=len(sigs), samples=int(sum(map(len, sigs))),
                         bases=sum(len(r[0]) for r in res), seconds=round(t, 4), reads_per_s=round(len(sigs) / t, 1),
                         samples_per_s=round(sum(map(len, sigs)) / t))
        if a.beam:
            rec[name]["beam"] = dict(width=a.beam, guided=True, steps=a.beam_steps,
                                     rows=beam_rows(net, beam_sigs, a.beam, a.beam_steps, dev))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

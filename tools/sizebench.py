#!/usr/bin/env python
"""Times one eager train step of mLstm_flipflop or mGru_flipflop at a hidden size (default 384, the reference trainer's
own default) with the recurrent layers on the HIP recurrence and on nn.LSTM / nn.GRU (layers.USE_HIP_LSTM / USE_HIP_GRU =
False: what a size the kernels refuse runs), in turns on one model and one batch; prints one JSON line, milliseconds per
step (median over --steps per turn).  Both models are built with the trainer's stride, 5: chunk_len 4000 is T = 800.
--switch NAME flips that switch of `layers` instead (USE_HIP_GRU_WGRAD, USE_HIP_LSTM_WGRAD: the fused weight-gradient
kernel against the GEMMs, the recurrence on the HIP kernels in both turns); the lists are then `on_ms_per_step` and
`off_ms_per_step`.  --switch USE_HIP_RNN_WIDE at a batch wider than one launch of the recurrence admits (say --size 384
--chunks 341): the slabs of include/taiyaki_amd_rnn_wide.h against nn.LSTM / nn.GRU.

    python tools/sizebench.py [--model mLstm_flipflop] [--size 384] [--chunk-len 4000] [--chunks 128] [--pairs 3]
                              [--steps 5] [--warmup 2] [--switch NAME]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, layers, models, parallel, synth, train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("mLstm_flipflop", "mGru_flipflop"), default="mLstm_flipflop")
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--chunk-len", type=int, default=4000)
    ap.add_argument("--chunks", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--switch", default=None, help="the switch of `layers` to flip (default: the recurrence's)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sizebench needs a GPU")
    dev = torch.device("cuda:0")
    stride = 5
    torch.manual_seed(0)
    gru = a.model == "mGru_flipflop"
    switch, fallback = ("USE_HIP_GRU", "nn_gru") if gru else ("USE_HIP_LSTM", "nn_lstm")
    if a.switch:
        if not isinstance(getattr(layers, a.switch, None), bool):
            raise SystemExit("layers has no switch %s" % a.switch)
        switch, fallback = a.switch, "off"
    net = getattr(models, a.model)(size=a.size, stride=stride).to(dev)
    probe = torch.zeros(a.chunk_len // stride, a.chunks, a.size, device=dev)
    rnns = [m for m in net.modules() if isinstance(m, layers.GruMod if gru else layers.Lstm)]
    query = layers.hip_gru_workspace_bytes if gru else layers.hip_lstm_workspace_bytes
    # (a batch wider than one launch admits runs as slabs of columns: layers.USE_HIP_RNN_WIDE, the switch to flip for it)
    if not (len(rnns) == 5 and all(query(m.rnn, probe) > 0 or layers.hip_rnn_wide_workspace_bytes(m.rnn, probe) > 0
                                   for m in rnns)):
        raise SystemExit("size %d x %d chunks is not admitted on %d CUs" % (a.size, a.chunks, layers._cu_count(dev)))
    sl = synth.realistic_seqlens(a.chunk_len // stride, a.chunks, 8, a.chunk_len, 9.0)
    sq, _ = synth.sequences(sl, 8)
    batch = dict(indata=torch.from_numpy(synth.signal_chunks(a.chunk_len, a.chunks, 8)).to(dev),
                 seqs=torch.from_numpy(sq), seqlens=torch.from_numpy(sl))
    trainer = train.Trainer(net, parallel.FlatGradArena(net), clip_num_mads=0)
    _lib.set_strict(False)

    def turn(use_hip):
        setattr(layers, switch, use_hip)
        times = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = trainer.step(batch)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        return float(np.median(times)), float(loss.detach())

    try:
        turns = [turn(True) + turn(False) for _ in range(a.pairs)]
    finally:
        setattr(layers, switch, True)
    _lib.raise_if_nonfinite()
    print(json.dumps({"model": a.model, "size": a.size, "chunk_len": a.chunk_len, "chunks": a.chunks,
                      "cus": layers._cu_count(dev), ("on" if a.switch else "hip") + "_ms_per_step": [round(t[0], 2) for t in turns],
                      fallback + "_ms_per_step": [round(t[2], 2) for t in turns],
                      "last_loss": [round(turns[-1][1], 4), round(turns[-1][3], 4)],
                      "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()

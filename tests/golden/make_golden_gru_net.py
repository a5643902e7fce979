#!/usr/bin/env python
"""Generate tests/golden/gru_net*.npz: the reference's one shipped network, NUMBERS only (this container only).

    python tests/golden/make_golden_gru_net.py

models/mGru_flipflop_remapping_model_r9_DNA.checkpoint is a convolution (1 -> 96, winlen 19, stride 4, tanh), five
GRU layers of size 96 (the first, third and fifth run backwards in time) and the flip-flop layer (96 -> 40).  This
script unpickles it (make_golden_realnet.load_network), cuts chunks of 2000 samples from the reference's mapped
reads with the reference's own chunk selection (make_golden_realnet.cut_chunks, seed 1: the first 16 of
realnet.npz's 32 "real" chunks, asserted against that file's scores) and stores
    param/<key>   every parameter, under the state_dict key of models.mGru_flipflop(size=96, stride=4);
    signal        (2000, 16) the standardised chunks;
    scores/...    (500, 16, 40) the genuine network's fp32 CPU output on them, in two halves of 8 columns.
The arrays are spread over four files (`parts` in main(); tests/helpers/gru_net.py puts them together again): new
files committed to this repository are kept below 1 MiB each, and together these are 2.3 MB.

Measured when the fixture was made: this repository's model, loaded from the arrays, on the CPU in fp32 against
`scores`: max-abs difference 0.0 (bit for bit; both sides are torch CPU nn.GRU on the same weights; scores span
+-5).  tests/test_gru_hip.py asserts 4x that with a floor of 5e-6, so 5e-6.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden  # noqa: E402
from tests.golden.make_golden_realnet import CHUNK_LEN, READ_FILES, cut_chunks, load_network  # noqa: E402

NCHUNK = 16
REVERSED = (1, 3, 5)      # positions of the Reverse(GruMod) layers in models.mGru_flipflop


def only(module, kind):
    found = [m for m in module.modules() if isinstance(m, kind)]
    assert len(found) == 1, (module, kind, found)
    return found[0]


def parameters_by_key(net):
    """The checkpoint's tensors under the keys of models.mGru_flipflop's state_dict."""
    import torch
    layers = list(net.sublayers)
    assert len(layers) == 7, [type(m).__name__ for m in layers]
    out = {}
    conv = only(layers[0], torch.nn.Conv1d)
    assert conv.weight.shape == (96, 1, 19) and conv.stride == (4,), (conv.weight.shape, conv.stride)
    out["0.conv.weight"], out["0.conv.bias"] = conv.weight, conv.bias
    for k in range(1, 6):
        assert (type(layers[k]).__name__ == "Reverse") == (k in REVERSED), (k, type(layers[k]).__name__)
        gru = only(layers[k], torch.nn.GRU)
        assert gru.weight_hh_l0.shape == (288, 96) and gru.num_layers == 1 and not gru.bidirectional
        prefix = "%d.layer.rnn." % k if k in REVERSED else "%d.rnn." % k
        for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            out[prefix + name] = getattr(gru, name)
    lin = only(layers[6], torch.nn.Linear)
    assert lin.weight.shape == (40, 96)
    out["6.linear.weight"], out["6.linear.bias"] = lin.weight, lin.bias
    return {k: v.detach().numpy().astype(np.float32) for k, v in out.items()}


def main():
    make_golden.build_reference()
    import torch
    from taiyaki import signal_mapping
    from taiyaki_amd import hdf5_lite
    torch.set_num_threads(8)
    net = load_network()
    params = parameters_by_key(net)
    print(sum(v.size for v in params.values()), "parameter floats")

    reads = []
    for path in READ_FILES:
        reads += hdf5_lite.read_mapped_signal_file(path)[1]
    sms = [signal_mapping.SignalMapping(
        r["Ref_to_signal"], r["Reference"], signalstart=0,
        **{k: r[k] for k in ("shift_frompA", "scale_frompA", "range", "offset", "digitisation",
                             "read_id", "Dacs")}) for r in reads]
    # the same draw as realnet.npz's "real" case (32 chunks at seed 1); its first 16
    chunks = cut_chunks(sms, CHUNK_LEN, 32, 1)
    full = np.vstack([np.array(c.current) for c in chunks]).T.astype(np.float32)
    with torch.no_grad():       # (as make_golden_realnet ran it: the whole batch of 32)
        scores = net(torch.from_numpy(full).unsqueeze(2)).numpy().astype(np.float32)[:, :NCHUNK]
    signal = np.ascontiguousarray(full[:, :NCHUNK])
    assert signal.shape == (CHUNK_LEN, NCHUNK) and scores.shape == (CHUNK_LEN // 4, NCHUNK, 40)
    real = np.load(os.path.join(HERE, "realnet.npz"))["real/scores"]
    assert np.array_equal(scores, real[:, :NCHUNK]), np.abs(scores - real[:, :NCHUNK]).max()
    print("scores equal realnet.npz real/scores[:, :16] bit for bit")

    # this repository's model on the same arrays, CPU fp32: the figure the test's bound is derived from
    from tests.helpers import gru_net
    arrays = {"param/" + k: v for k, v in params.items()}
    mine = gru_net.build_model(arrays)
    with torch.no_grad():
        got = mine(torch.from_numpy(signal).unsqueeze(2)).numpy()
    print("repository model (CPU fp32) against the network's scores: max-abs", np.abs(got - scores).max())

    gru = lambda ks: {"param/" + k: v for k, v in params.items() if int(k.split(".")[0]) in ks}  # noqa: E731
    parts = {
        "gru_net.npz": dict(gru((0, 1, 2, 3, 6)), signal=signal),
        "gru_net_rnn.npz": gru((4, 5)),
        "gru_net_scores0.npz": {"scores/cols_0_8": scores[:, :8]},
        "gru_net_scores1.npz": {"scores/cols_8_16": scores[:, 8:]},
    }
    assert sorted(parts) == sorted(gru_net.FILES)
    for name, arrs in parts.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrs)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20), name


if __name__ == "__main__":
    main()

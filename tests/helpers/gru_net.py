"""The reference's shipped mGru flip-flop network as this repository's model, from tests/golden/gru_net*.npz
(tests/golden/make_golden_gru_net.py: every parameter of the checkpoint, the standardised chunks it was run on and
its own fp32 CPU scores on them)."""
import os

import numpy as np
import torch

from taiyaki_amd import models

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
# (the generator says why there are four files)
FILES = ["gru_net.npz", "gru_net_rnn.npz", "gru_net_scores0.npz", "gru_net_scores1.npz"]
SIZE, STRIDE, WINLEN = 96, 4, 19


def load_arrays():
    """{name: array}: `param/<state_dict key>` of models.mGru_flipflop(size=96, stride=4), `signal` (2000, 16) and
    `scores` (500, 16, 40)."""
    out = {}
    for name in FILES:
        with np.load(os.path.join(GOLDEN, name)) as z:
            out.update({k: z[k] for k in z.files})
    out["scores"] = np.concatenate([out.pop("scores/cols_0_8"), out.pop("scores/cols_8_16")], axis=1)
    return out


def build_model(arrays, dtype=torch.float32):
    net = models.mGru_flipflop(size=SIZE, stride=STRIDE, winlen=WINLEN)
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in arrays.items() if k.startswith("param/")}
    assert sorted(state) == sorted(net.state_dict()), (sorted(state), sorted(net.state_dict()))
    net.load_state_dict(state)
    return net.to(dtype).eval()

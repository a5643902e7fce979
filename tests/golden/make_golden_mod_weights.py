#!/usr/bin/env python
"""Generate tests/golden/mod_weights_small.npz with the GENUINE reference: taiyaki.flipflopfings.extract_mod_weights on
the seeded cases of tests/mods_support.py (random flip-flop-legal paths and float32 weights for three can_nmods, T from
1 to 60, one path without a move and one that moves at every block).  Inputs and the reference's results are stored.

    python tests/golden/make_golden_mod_weights.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import mods_support as ms  # noqa: E402
from tests.golden import make_golden  # noqa: E402


def main():
    sys.path.insert(0, make_golden.REF)
    from taiyaki import flipflopfings
    if not hasattr(np, "NAN"):          # numpy 2 dropped the alias the function uses
        np.NAN = np.nan
    out = {}
    for name, can_nmods, T, kind, seed in ms.golden_cases():
        w, path = ms.golden_inputs(can_nmods, T, kind, seed)
        res = flipflopfings.extract_mod_weights(w, path, np.array(can_nmods))
        nmove = int((path[1:] != path[:-1]).sum())
        assert res.shape == (nmove + 1, sum(can_nmods)) and np.isnan(res[0]).all(), (name, res.shape)
        assert nmove == {"nomove": 0, "allmove": T}.get(kind, nmove)
        out[name + "/weights"], out[name + "/path"] = w, path.astype(np.int8)
        out[name + "/mods"] = res.astype(np.float32)            # (selected float32 values: the cast is exact)
        assert np.array_equal(out[name + "/mods"].astype(res.dtype), res, equal_nan=True)
    np.savez_compressed(ms.GOLDEN, **out)
    print("wrote %s: %d cases, %d bytes" % (ms.GOLDEN, len(ms.golden_cases()), os.path.getsize(ms.GOLDEN)))


if __name__ == "__main__":
    main()

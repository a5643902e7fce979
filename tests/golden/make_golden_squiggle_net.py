#!/usr/bin/env python
"""Writes tests/golden/squiggle_net.npz: the reference's squiggle predictor network (bin/train_squiggle.py:
`create_convolution`, run on the genuine taiyaki.layers / taiyaki.activation) on counter-based weights and inputs, so
that tests/test_squiggle_net*.py stand without the reference.

Per case (size, depth, winlen, P, N): x (tetrahedron embeddings of `synth.randint` bases), a non-uniform dy, the
reference's float32 y, dx, dW, db and the same from its .double() copy, under this project's parameter names (the
reference's `sublayers.k.` is `k.` here).  The parameters themselves are NOT stored: `make_inputs` regenerates them from
their counters and `load_case` checks them against the stored sums.  A random weight gradient does not compress, and
three copies of it (float32, float64) would pass the size limit for a committed file, so the float64 weight gradients
are stored as their difference from the float32 ones, in float16 units of `dscale` (float32 epsilon x the largest
entry): what that loses is 2^-11 of a difference of about 1e-7, i.e. 1e-10 of the largest entry.  Plus one table written by the formatting lines of bin/predict_squiggle.py:49-52
(read from that file and executed as they stand) for the first case's first column.

`create_convolution` is taken from the script's source (the script itself imports h5py and Bio at its top, which the
function does not need).

    python tests/golden/make_golden_squiggle_net.py /path/to/taiyaki
"""
import ast
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from taiyaki_amd import synth  # noqa: E402
from taiyaki_amd.squiggle_match import embed_sequence  # noqa: E402

PATH = os.path.join(HERE, "squiggle_net.npz")
MAX_BYTES = 1 << 20             # the limit for a committed file
CASES = [(32, 4, 9, 53, 3), (16, 1, 5, 12, 2), (64, 2, 9, 40, 2)]      # size, depth, winlen, P, N
SEED = 37


def case_name(case):
    return "s%d_d%d_w%d_p%d_n%d" % tuple(case)


def reference_builder(ref):
    """create_convolution of bin/train_squiggle.py, defined over the genuine layers and activation modules"""
    sys.path.insert(0, ref)
    from taiyaki import activation, layers
    src = open(os.path.join(ref, "bin", "train_squiggle.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "create_convolution"]
    scope = {"activation": activation, "layers": layers}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "train_squiggle.py", "exec"), scope)
    return scope["create_convolution"]


def table_writer(ref):
    """lines 49-52 of bin/predict_squiggle.py as a function of (fh, seq, squiggle)"""
    lines = open(os.path.join(ref, "bin", "predict_squiggle.py")).read().split("\n")[48:52]
    assert lines[0].strip() == r"fh.write('base\tcurrent\tsd\tdwell\n')", lines[0]
    body = "\n".join(line[12:] for line in lines)       # (the lines sit inside `with` and `for`: 12 spaces)
    code = compile("def write(fh, seq, squiggle):\n" + "\n".join("    " + b for b in body.split("\n")), "predict_squiggle.py", "exec")
    scope = {"np": np}
    exec(code, scope)
    return scope["write"]


class _Seq:     # what the script's loop reads of a Bio record
    def __init__(self, seq):
        self.seq = seq


def make_inputs(case, stream):
    """x, dy and the state dict (this project's names) of a case, from counters alone"""
    size, depth, winlen, P, N = case
    bases = synth.randint(SEED, stream, P * N, 4).reshape(P, N)
    x = np.stack([embed_sequence(bases[:, n], alphabet=None) for n in range(N)], axis=1).astype(np.float32)
    dy = (2 * synth.uniform01(SEED, stream + 1, P * N * 3) - 1).reshape(P, N, 3).astype(np.float32)
    dy *= np.linspace(0.25, 2.0, P, dtype=np.float32)[:, None, None]
    state, off = {}, 0
    shapes = [(size, 3)] + [(size, size)] * depth + [(3, size)]
    for k, (cout, cin) in enumerate(shapes):
        name = "%d.conv." % k if k in (0, depth + 1) else "%d.layer.conv." % k
        nw = cout * cin * winlen
        u = synth.uniform01(SEED, stream + 2, nw + cout, offset=off)
        off += nw + cout
        scale = np.float32(1.5 / np.sqrt(cin * winlen))
        state[name + "weight"] = ((2 * u[:nw] - 1) * scale).reshape(cout, cin, winlen).astype(np.float32)
        state[name + "bias"] = ((2 * u[nw:] - 1) * np.float32(0.5)).astype(np.float32)
    return x, dy, state


def load_case(gold, case):
    """One case of the stored file: x, dy, the regenerated parameters {name: array} and, per precision, y, dx and the
    gradients {name: array}; the float64 weight gradients rebuilt from their stored differences."""
    tag, i = case_name(case), [tuple(c) for c in gold["cases"]].index(tuple(case))
    x, dy, state = make_inputs(case, 10 * (i + 1))
    assert np.array_equal(x, gold[tag + "/x"]) and np.array_equal(dy, gold[tag + "/dy"])
    out = {"x": x, "dy": dy, "params": state}
    for k, v in state.items():
        assert float(v.astype(np.float64).sum()) == float(gold[tag + "/paramsum/" + k]), k
    for prec in ("f32", "f64"):
        out[prec] = {"y": gold["%s/%s/y" % (tag, prec)], "dx": gold["%s/%s/dx" % (tag, prec)], "grad": {}}
    for k in state:
        g32 = gold["%s/f32/grad/%s" % (tag, k)]
        out["f32"]["grad"][k] = g32
        if k.endswith("weight"):
            delta = gold["%s/f64/graddelta/%s" % (tag, k)].astype(np.float64) * float(gold["%s/f64/dscale/%s" % (tag, k)])
            out["f64"]["grad"][k] = g32.astype(np.float64) + delta
        else:
            out["f64"]["grad"][k] = gold["%s/f64/grad/%s" % (tag, k)]
    return out


def run(net, x, dy):
    import torch
    xt = torch.from_numpy(x).to(next(net.parameters()).dtype).requires_grad_(True)
    y = net(xt)
    y.backward(torch.from_numpy(dy).to(y.dtype))
    grads = {name.replace("sublayers.", ""): p.grad.numpy() for name, p in net.named_parameters()}
    return y.detach().numpy(), xt.grad.numpy(), grads


def main(ref):
    import torch
    torch.set_num_threads(1)
    build = reference_builder(ref)
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for i, case in enumerate(CASES):
        size, depth, winlen, P, N = case
        x, dy, state = make_inputs(case, 10 * (i + 1))
        net = build(size, depth, winlen)
        net.load_state_dict({"sublayers." + k: torch.from_numpy(v) for k, v in state.items()})
        tag = case_name(case)
        out[tag + "/x"], out[tag + "/dy"] = x, dy
        for k, v in state.items():
            out[tag + "/paramsum/" + k] = np.float64(v.astype(np.float64).sum())
        for prec, model in (("f32", net), ("f64", build(size, depth, winlen).double())):
            if prec == "f64":
                model.load_state_dict({"sublayers." + k: torch.from_numpy(v).double() for k, v in state.items()})
            y, dx, grads = run(model, x, dy)
            assert y.dtype == (np.float32 if prec == "f32" else np.float64)
            out["%s/%s/y" % (tag, prec)], out["%s/%s/dx" % (tag, prec)] = y, dx
            for k, v in grads.items():
                if prec == "f64" and k.endswith("weight"):
                    g32 = out["%s/f32/grad/%s" % (tag, k)]
                    dscale = np.float64(np.finfo(np.float32).eps) * np.abs(v).max()
                    delta = ((v - g32.astype(np.float64)) / dscale).astype(np.float16)
                    assert np.all(np.isfinite(delta))
                    assert np.abs(g32.astype(np.float64) + delta.astype(np.float64) * dscale - v).max() <= 1e-9 * np.abs(v).max()
                    out["%s/f64/graddelta/%s" % (tag, k)], out["%s/f64/dscale/%s" % (tag, k)] = delta, dscale
                else:
                    out["%s/%s/grad/%s" % (tag, prec, k)] = v
        if i == 0:
            seq = "".join("ACGT"[b] for b in synth.randint(SEED, 10, P * N, 4).reshape(P, N)[:, 0])
            fh = io.StringIO()
            table_writer(ref)(fh, _Seq(seq), out[tag + "/f32/y"][:, 0])
            out["table/seq"] = np.frombuffer(seq.encode(), dtype=np.uint8)
            out["table/text"] = np.frombuffer(fh.getvalue().encode(), dtype=np.uint8)
    np.savez_compressed(PATH, **out)
    assert os.path.getsize(PATH) < MAX_BYTES, os.path.getsize(PATH)
    print("wrote %s (%d bytes, %d arrays)" % (PATH, os.path.getsize(PATH), len(out)))


if __name__ == "__main__":
    main(sys.argv[1])

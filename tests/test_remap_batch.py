"""`prepare_mapping_funcs.remap_batch` on the shipped mGru network (tests/golden/gru_net*.npz): its plumbing is exact
against the operators it is made of (`layers.forward_varlen`, `flipflop_remap.flipflop_remap_batch`,
`flipflop_remap.ref_to_signal_from_remapping_paths`); the network's numbers are tests/test_forward_varlen.py's concern.
No path is compared with per-read scores: a rounding-level difference in a near-tie can move a path without anything
being wrong."""
import numpy as np
import pytest
import torch

from taiyaki_amd import flipflop_remap, layers, prepare_mapping_funcs
from tests.helpers import gru_net

pytestmark = pytest.mark.gpu

NSAMPLE = [2000, 800, 1403, 1999, 1000]                 # untrimmed
TRIMS = [(0, 0), (37, 13), (0, 0), (50, 121), (0, 0)]
EMPTY = 2                                               # the read whose reference is empty


@pytest.fixture(scope="module")
def case(gpu_device):
    arrays = gru_net.load_arrays()
    net = gru_net.build_model(arrays).to(gpu_device)
    rs = np.random.RandomState(21)
    # the fixture's chunks are standardised: as currents they are 90 + 12 x, with shift 90 and scale 12 per read
    # (slightly different per read, so that a mixed-up parameter shows)
    signals, params, refs = [], [], []
    for r, (n, (ts, te)) in enumerate(zip(NSAMPLE, TRIMS)):
        shift, scale = 90.0 + r, 12.0 + 0.5 * r
        signals.append((arrays["signal"][:n, r] * scale + shift).astype(np.float32))
        params.append(dict(trim_start=ts, trim_end=te, shift=shift, scale=scale))
        nblk = -(-(n - ts - te) // gru_net.STRIDE)
        refs.append("" if r == EMPTY else "".join(rs.choice(list("ACGT"), size=int(0.4 * nblk))))
    with torch.no_grad():
        results = prepare_mapping_funcs.remap_batch(signals, refs, net, params)
    return dict(net=net, signals=signals, params=params, refs=refs, results=results, dev=gpu_device)


def _standardised(case, r):
    """What remap_batch feeds the network for read r: float32, one operation at a time."""
    p, s = case["params"][r], case["signals"][r]
    s = s[p["trim_start"]:len(s) - p["trim_end"]]
    return (s - np.float32(p["shift"])) / np.float32(p["scale"])


def test_plumbing_is_exact(case):
    good = [r for r in range(len(NSAMPLE)) if r != EMPTY]
    std = [_standardised(case, r) for r in good]
    order = np.argsort([len(s) for s in std], kind="stable")       # one launch: the plan's column order
    x = torch.zeros(max(len(s) for s in std), len(good), 1)
    for j, k in enumerate(order):
        x[:len(std[k]), j, 0] = torch.from_numpy(std[k])
    with torch.no_grad():
        out, out_len = layers.forward_varlen(case["net"], x.to(case["dev"]), [len(std[k]) for k in order])
    scores = [None] * len(good)
    for j, k in enumerate(order):
        scores[k] = out[:out_len[j], j].contiguous()
    want_score, want_path = flipflop_remap.flipflop_remap_batch(scores, [case["refs"][r] for r in good], localpen=0.0)
    want_rts = flipflop_remap.ref_to_signal_from_remapping_paths(
        want_path, [len(case["refs"][r]) for r in good], gru_net.STRIDE,
        [case["params"][r]["trim_start"] for r in good], [NSAMPLE[r] for r in good], device=case["dev"])
    for k, r in enumerate(good):
        score, path, rts = case["results"][r]
        assert score == want_score[k], r
        assert path.dtype == np.int64 and np.array_equal(path, want_path[k]), r
        assert rts.dtype == np.int32 and np.array_equal(rts, want_rts[k]), r
        assert len(path) == len(scores[k]) + 1 and len(rts) == len(case["refs"][r]) + 1
        assert (path >= 0).sum() > 0 and np.isfinite(score)


def test_a_read_without_reference_is_none_and_disturbs_nothing(case):
    assert case["results"][EMPTY] is None
    keep = [r for r in range(len(NSAMPLE)) if r != EMPTY]
    with torch.no_grad():
        without = prepare_mapping_funcs.remap_batch([case["signals"][r] for r in keep], [case["refs"][r] for r in keep],
                                                    case["net"], [case["params"][r] for r in keep])
    for got, r in zip(without, keep):
        want = case["results"][r]
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), r


def test_unusable_reads_are_none(case):
    signals, refs = case["signals"][:3], ["ACGT", "ACGT", case["refs"][0][:100]]
    params = [dict(trim_start=1500, trim_end=500, shift=90.0, scale=12.0),       # nothing left after trimming
              dict(trim_start=0, trim_end=0, shift=float("nan"), scale=12.0),
              case["params"][2]]
    with torch.no_grad():
        got = prepare_mapping_funcs.remap_batch(signals, refs, case["net"], params)
        assert got[0] is None and got[1] is None and got[2] is not None and len(got[2][2]) == 101
        assert prepare_mapping_funcs.remap_batch(signals[:2], refs[:2], case["net"], params[:2]) == [None, None]
        assert prepare_mapping_funcs.remap_batch([], [], case["net"], []) == []


def test_two_columns_per_launch_give_the_same_results(case):
    """The launch split.  The recurrences give a column the same bits in either launch (tests/test_rnn_varlen.py); the
    Convolution's and the output layer's GEMMs may sum in another order at another batch width.  The project's rule
    allows a float32 pass 2e-6 max|ref| per element beyond the reference pass's own error, with max|ref| <= 5 (the
    output layer's scale): 1e-5 per run, 2e-5 between two runs, and twice that here for the two GEMM layers.  A path's
    sum over T rows then moves by at most 4e-5 T, and so does the best path's score, whichever path that is in either
    run.  ref_to_signal: the same lengths."""
    with torch.no_grad():
        split = prepare_mapping_funcs.remap_batch(case["signals"], case["refs"], case["net"], case["params"],
                                                  max_columns=2)
    assert split[EMPTY] is None
    for r, (one, two) in enumerate(zip(case["results"], split)):
        if one is None:
            continue
        nblk = len(one[1]) - 1
        print("read %d: alignment score %.6f at max_columns 64, %.6f at 2, bound %.3g" % (r, one[0], two[0], 4e-5 * nblk))
        assert abs(one[0] - two[0]) <= 4e-5 * nblk, r
        assert len(one[1]) == len(two[1]) and len(one[2]) == len(two[2])

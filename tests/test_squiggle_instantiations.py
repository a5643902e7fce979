"""Every positions-per-lane instantiation R of the squiggle match (sq_positions_per_lane in csrc/squiggle_kernels.hip:
npos <= 64, 128, 256, 320, 512, 768, 1024 -> R = 1, 2, 4, 5, 8, 12, 16; four kernels per R), launched on batches of
reads of different lengths and compared with the reference's own answers (tests/golden/squiggle_lanes.npz, written by
make_golden_squiggle.py from the reference C) and with the float64 restatement tests/helpers/squiggle_model.py.

The cases are the second table of tests/golden/squiggle_cases.py: per R the first npos that selects it, the full
npos = 64 R and an npos whose last position sits in the middle of a lane with idle lanes behind it, one clipped case
per R (junk at both ends, localpen / minscore such that the reference's path enters late and leaves early), and the
8409-sample read of test_squiggle_match.py, whose gradient no other test compares.  The fixture holds answers only; the
inputs are regenerated from their seeds and held to the digest the fixture keeps of them.

Allowances.  The reference's fp32 C has an error of its own against float64 that grows with the read (gradient: below
1.3e-4 of a column's largest magnitude up to npos 321, up to 3.4e-4 from 450 on, 7e-4 at 8409 samples), so a constant
cannot serve every size.  `reference_error(name)` measures it per case (the CPU test prints it) and the HIP results are
allowed max(the constant of test_squiggle_match.py, FACTOR x the reference's own error on that case) against float64;
FACTOR = 4 is the ratio those constants stand in to the reference's error (5e-4 / 1.2e-4, 1e-5 / 1.8e-6).  The Viterbi
has no allowance: its path is the reference's and its score within the 1e-6 of test_hip_matches_the_reference_fixture.

What this file found when it was written: no instantiation wrong.  Over the 28 cases the HIP cost is at most 1.44 x and
the HIP gradient at most 1.33 x the reference's own error (6.2e-4 against its 7.0e-4 at 8409 samples); every path is
the reference's; the Viterbi score is the reference's float or one ulp beside it.  Three trial defects that
tests/test_squiggle_match.py does not see (the cost taken from the lane's last position at R 16, a forward column
loaded one step late at R >= 8, tied order values of the end state's candidates at R 12) each fail here.
profiles/r25_squiggle_instantiations.txt keeps the measured errors beside the reference's, and the trials.

Every launch here ends with return code 0 and status word 0 behind the synchronise (the module's entry points raise
otherwise); after a launch that did not, this module launches nothing more (the remaining tests fail at once)."""
import functools

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.golden import squiggle_cases as C
from tests.helpers import squiggle_model as M
from tests.test_squiggle_match import (COST_RTOL, GRAD_COL_TOL, REF_COST_RTOL, REF_GRAD_COL_TOL, _grad_err)

FACTOR = 4.0
RS = [r for _, r in C.LANE_RULE]
# the cases in which the reference's own gradient is beyond REF_GRAD_COL_TOL of float64 (3.4e-4 and 7.0e-4 of the
# level column's largest entry: 2675 and 8409 samples over 1000 and 1024 positions);
# test_restatement_matches_the_lanes_fixture holds every other case to that constant
REF_GRAD_BEYOND = {"clip1000", C.LONG}
# one case per R for the tests that need no more
ALONE = ["full64", "mid100", "first129", "full320", "mid450", "first513", "full1024"]
ROUTES = ["clip40", "first65", "mid202", "first257", "full512", "mid700", "mid1000"]
ABI_PATH = ["clip450", "clip700", "clip1000"]
GUARD_BYTES = 4096
GUARD_BITS = 0x7FC0BEEF         # a quiet NaN with a payload: what the test's own buffers hold before a launch
PATH_SENTINEL = -7


@pytest.fixture(scope="module")
def gold():
    return load_golden("squiggle_lanes.npz")


@functools.lru_cache(maxsize=None)
def lane_case(name):
    return C.make_lane_case(name)


def _npos(name):
    return 1024 if name == C.LONG else C.LANE_CASES[name][0]


def _offsets(case):
    return np.concatenate([[0], np.cumsum(case["siglen"])])


def _reachable(case):
    return case["siglen"] >= case["params"].shape[0] - 1


def _check_digest(gold, name):
    siglen, sums = C.digest(lane_case(name))
    assert np.array_equal(siglen, gold[name + "/siglen"]), "the regenerated reads are not the fixture's"
    np.testing.assert_allclose(sums, gold[name + "/sums"], rtol=1e-12, err_msg="the regenerated inputs are not the fixture's")


@functools.lru_cache(maxsize=None)
def f64_cost_grad(name):
    """(cost (nbatch,), grad (npos, nbatch, 3)) of the float64 restatement; the gradient of reachable reads only (zeros
    elsewhere)."""
    case = lane_case(name)
    off, ok = _offsets(case), _reachable(case)
    cost, grad = np.zeros(len(ok)), np.zeros(case["params"].shape)
    for b in range(len(ok)):
        p, s = case["params"][:, b], case["signal"][off[b]:off[b + 1]]
        f = M.forward(p, s, case["back_prob"])
        cost[b] = -f[-1, 0, -1]
        if ok[b]:
            grad[:, b] = M.grad(p, s, case["back_prob"], f=f)
    cost.setflags(write=False)
    grad.setflags(write=False)
    return cost, grad


@functools.lru_cache(maxsize=None)
def f64_viterbi(name):
    case = lane_case(name)
    vit = M.batch(M.viterbi, case, case["localpen"], case["minscore"])
    return np.array([v[0] for v in vit]), np.concatenate([v[1] for v in vit])


@functools.lru_cache(maxsize=None)
def reference_error(name):
    """The reference's own error against float64 on a case: (cost, relative, the largest over its reachable reads;
    gradient, per column over the column's largest magnitude)."""
    gold = load_golden("squiggle_lanes.npz")
    ok = _reachable(lane_case(name))
    cost, grad = f64_cost_grad(name)
    return (float(np.max(np.abs(gold[name + "/cost"][ok] - cost[ok]) / np.abs(cost[ok]))),
            _grad_err(gold[name + "/grad"][:, ok], grad[:, ok]))


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_dispatch_rule_is_the_table():
    """The lattice of one read of one sample is 2 columns of 2 x 64 R floats: the query gives R away."""
    from taiyaki_amd import _lib
    lib = _lib.lib()
    seen = set()
    for npos in range(1, 1026):
        r = C.lanes_r(npos)
        assert lib.tk_squiggle_match_workspace_bytes(1, npos, 1, 1) == 2 * 2 * 64 * r * 4, npos
        seen.add(r)
    assert C.lanes_r(1024) == 16 and C.lanes_r(1025) == 0
    assert seen == set(RS) | {0}


def test_cases_cover_every_positions_per_lane_three_ways():
    """Per R of the rule: the first npos that selects it, the full npos = 64 R and an npos in between with idle lanes
    behind the last position's (for R >= 4, where a lane has a middle: one whose last position is neither the first
    nor the last of its lane), each with reads of different lengths; one clipped case; nothing else.  (npos 1, 37
    and 300 are cases of squiggle_small.npz.)"""
    kinds = {r: set() for r in RS}
    clipped = {r: 0 for r in RS}
    everything = [(name, _npos(name), None if name == C.LONG else C.LANE_CASES[name][1]) for name in C.LANE_NAMES]
    everything += [(name, v[0], None) for name, v in C.CASES.items()]
    prev = 0
    for lim, r in C.LANE_RULE:
        for name, npos, kind in everything:
            if C.lanes_r(npos) != r:
                continue
            if kind == "clip":
                clipped[r] += 1
                assert lane_case(name)["localpen"] is not None
                continue
            if npos == prev + 1:
                kinds[r].add("first")
            if npos == lim:
                kinds[r].add("full")
            last = npos - 1
            if last // r < 63 and prev + 1 < npos < lim:
                kinds[r].add("idle")
                if r < 4 or 0 < last % r < r - 1:
                    kinds[r].add("mid")
        prev = lim
    assert set(kinds) == set(RS) == {C.lanes_r(_npos(name)) for name in C.LANE_NAMES}
    assert all(k == {"first", "full", "idle", "mid"} for k in kinds.values()), kinds
    assert all(n == 1 for n in clipped.values()), clipped
    for names in (ALONE, ROUTES):
        assert [C.lanes_r(_npos(n)) for n in names] == RS
    assert [C.lanes_r(_npos(n)) for n in ABI_PATH] == [r for r in RS if r >= 8]
    shorts = set()
    for name in C.LANE_CASES:
        case = lane_case(name)
        assert len(set(case["siglen"].tolist())) == len(case["siglen"]) > 1, name
        if C.LANE_CASES[name][1] != "clip":
            npos = _npos(name)
            assert npos - 1 in case["siglen"] and case["siglen"][-1] < npos - 1, name
            shorts.add(int(case["siglen"][-1]))
            assert any(n >= npos - 1 and n % 64 <= 1 for n in case["siglen"]), name
    assert shorts == set(C.SHORT_LENGTHS)


@pytest.mark.parametrize("name", C.LANE_NAMES)
def test_restatement_matches_the_lanes_fixture(gold, name):
    _check_digest(gold, name)
    case = lane_case(name)
    vcost, path = f64_viterbi(name)
    assert np.array_equal(path, gold[name + "/path"]), np.flatnonzero(path != gold[name + "/path"])[:10]
    np.testing.assert_allclose(vcost, gold[name + "/vcost"], rtol=1e-5)
    cost_err, grad_err = reference_error(name)
    print("%s: reference / float64: cost %.3g gradient %s" % (name, cost_err, grad_err))
    assert cost_err < REF_COST_RTOL
    assert np.all(grad_err < REF_GRAD_COL_TOL) or name in REF_GRAD_BEYOND, grad_err
    ok = _reachable(case)
    assert np.all(gold[name + "/cost"][~ok] > 1e29)


@pytest.mark.parametrize("name", [n for n, v in C.LANE_CASES.items() if v[1] == "clip"])
def test_clipped_cases_enter_late_and_leave_early(gold, name):
    """The reference's path of every read starts in the start state, enters at a position > 0, leaves from a position
    < npos - 1 and ends in the end state."""
    _check_digest(gold, name)
    case = lane_case(name)
    npos, off = _npos(name), _offsets(case)
    for b in range(len(case["siglen"])):
        path = gold[name + "/path"][off[b]:off[b + 1]]
        inside = np.flatnonzero(path >= 0)
        assert path[0] == -1 and path[-1] == -1 and len(inside) > 0, (name, b)
        assert 0 < path[inside[0]] < path[inside[-1]] < npos - 1, (name, b, path[inside[0]], path[inside[-1]])
        assert np.all(path[inside[0]:inside[-1] + 1] >= 0), (name, b)


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
_stopped = []           # the first launch of this module that did not end with return code 0 and status word 0


@pytest.fixture(autouse=True)
def _nothing_after_a_bad_status():
    if _stopped:
        pytest.fail("not run: an earlier launch of this module ended with %s" % (_stopped[0],))


def _launch(fn, *args, **kwargs):
    """An entry point of taiyaki_amd.squiggle_match: it raises on a return code or a status word that is not 0."""
    try:
        return fn(*args, **kwargs)
    except Exception as exc:
        _stopped.append((fn.__name__, repr(exc)))
        raise


def _finish(rc, status, what):
    """A launch at the C ABI: return code 0, and the status word 0 behind the synchronise."""
    from taiyaki_amd import _lib
    if rc != 0:
        _stopped.append((what, "rc", rc))
    _lib.check(rc, what)
    torch.cuda.synchronize()
    word = int(status.item())
    if word != 0:
        _stopped.append((what, "status", word))
    assert word == 0, (what, word)


def _args(case):
    return case["params"], case["signal"], case["siglen"], case["back_prob"]


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def hip_errors(name, cost, grad):
    """HIP against float64 as `reference_error` has the reference: (cost, gradient per column)."""
    ok = _reachable(lane_case(name))
    want_cost, want_grad = f64_cost_grad(name)
    return (float(np.max(np.abs(cost[ok] - want_cost[ok]) / np.abs(want_cost[ok]))),
            _grad_err(grad[:, ok], want_grad[:, ok]))


def _assert_within_allowance(name, cost, grad, what):
    cost_err, grad_err = hip_errors(name, cost, grad)
    ref_cost, ref_grad = reference_error(name)
    print("%s %s: cost HIP %.3g reference %.3g ratio %.2f; gradient HIP %s reference %s ratio %s"
          % (name, what, cost_err, ref_cost, cost_err / ref_cost, grad_err, ref_grad, grad_err / ref_grad))
    assert cost_err <= max(COST_RTOL, FACTOR * ref_cost), (cost_err, ref_cost)
    assert np.all(grad_err <= np.maximum(GRAD_COL_TOL, FACTOR * ref_grad)), (grad_err, ref_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.LANE_NAMES)
def test_cost_and_gradient_against_float64(gold, gpu_device, name):
    from taiyaki_amd import squiggle_match as sm
    _check_digest(gold, name)
    case = lane_case(name)
    cost = _launch(sm.squiggle_match_cost, *_args(case))
    grad = _launch(sm.squiggle_match_grad, *_args(case))
    assert np.all(np.isfinite(grad))
    bad = ~_reachable(case)
    print("%s: unreachable reads' cost %s, the fixture's %s" % (name, cost[bad], gold[name + "/cost"][bad]))
    assert np.array_equal(cost[bad], gold[name + "/cost"][bad])
    _assert_within_allowance(name, cost, grad, "cost, gradient")


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.LANE_NAMES)
def test_viterbi_path_is_the_references(gold, gpu_device, name):
    from taiyaki_amd import squiggle_match as sm
    _check_digest(gold, name)
    case = lane_case(name)
    vcost, path = _launch(sm.squiggle_match_path, *_args(case), case["localpen"], case["minscore"])
    want = gold[name + "/path"]
    print("%s: Viterbi score HIP / reference - 1: %s" % (name, vcost / gold[name + "/vcost"] - 1.0))
    assert np.array_equal(path, want), (np.flatnonzero(path != want)[:10], path[path != want][:10], want[path != want][:10])
    np.testing.assert_allclose(vcost, gold[name + "/vcost"], rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALONE)
def test_each_read_alone_equals_it_in_its_batch(gpu_device, name):
    """Bit for bit: cost, gradient, Viterbi score and path of a read do not depend on where it stands in a batch."""
    from taiyaki_amd import squiggle_match as sm
    case = lane_case(name)
    off = _offsets(case)
    cost = _launch(sm.squiggle_match_cost, *_args(case))
    grad = _launch(sm.squiggle_match_grad, *_args(case))
    vcost, path = _launch(sm.squiggle_match_path, *_args(case), case["localpen"], case["minscore"])
    for b in range(len(case["siglen"])):
        one = (case["params"][:, b:b + 1], case["signal"][off[b]:off[b + 1]], case["siglen"][b:b + 1], case["back_prob"])
        assert np.array_equal(_bits(_launch(sm.squiggle_match_cost, *one)), _bits(cost[b:b + 1])), (name, b)
        assert np.array_equal(_bits(_launch(sm.squiggle_match_grad, *one)), _bits(grad[:, b:b + 1])), (name, b)
        v1, p1 = _launch(sm.squiggle_match_path, *one, case["localpen"], case["minscore"])
        assert np.array_equal(_bits(v1), _bits(vcost[b:b + 1])), (name, b)
        assert np.array_equal(p1, path[off[b]:off[b + 1]]), (name, b)


def _guarded_bytes(nbytes, dev):
    """(whole buffer, its first nbytes): uint8, every 32-bit word GUARD_BITS, GUARD_BYTES more than nbytes."""
    assert nbytes % 4 == 0
    whole = torch.full(((nbytes + GUARD_BYTES) // 4,), GUARD_BITS, dtype=torch.int32, device=dev).view(torch.uint8)
    return whole, whole[:nbytes]


def _guard_intact(whole, nbytes):
    return bool((whole[nbytes:].view(torch.int32) == GUARD_BITS).all().item())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROUTES)
def test_both_routes_to_the_gradient_agree(gpu_device, name):
    """cost_dev(lattice=buf) then grad_dev(lattice=buf) -- the autograd path: the storing forward, then the backward
    sweep alone -- against grad_dev on its own, bit for bit, with the lattice in the test's own NaN-filled buffer of
    exactly lattice_bytes and a guard behind it.  The storing forward's cost is held to float64 like the plain one's."""
    from taiyaki_amd import squiggle_match as sm
    case = lane_case(name)
    dev = gpu_device
    p, s, n = (torch.from_numpy(case[k]).to(dev) for k in ("params", "signal", "siglen"))
    nbytes = sm.lattice_bytes(p, s)
    assert nbytes == (len(case["signal"]) + len(case["siglen"])) * 2 * 64 * C.lanes_r(_npos(name)) * 4
    whole, buf = _guarded_bytes(nbytes, dev)
    cost = _launch(sm.cost_dev, p, s, n, case["back_prob"], lattice=buf)
    assert _guard_intact(whole, nbytes), "the storing forward wrote behind its lattice"
    lattice = buf.view(torch.float32)
    assert not bool(torch.isnan(lattice).any().item()), "columns of the lattice were not stored"
    grad = _launch(sm.grad_dev, p, s, n, case["back_prob"], lattice=buf)
    assert _guard_intact(whole, nbytes)
    alone = _launch(sm.grad_dev, p, s, n, case["back_prob"])
    assert np.array_equal(_bits(grad.cpu().numpy()), _bits(alone.cpu().numpy()))
    plain = _launch(sm.cost_dev, p, s, n, case["back_prob"])
    print("%s: storing forward's cost equals the plain forward's bit for bit: %s" % (name, torch.equal(cost, plain)))
    _assert_within_allowance(name, cost.cpu().numpy(), grad.cpu().numpy(), "storing forward, backward alone")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ABI_PATH)
def test_path_at_the_c_abi_with_the_tests_own_workspace(gold, gpu_device, name):
    """tk_squiggle_match_path_dev with a workspace of exactly the queried size, poisoned, a guard behind it, and a
    `signal` longer than sum(siglen): the same path, the guard untouched, the path's trailing entries as given."""
    from taiyaki_amd import _lib
    case = lane_case(name)
    dev, L = gpu_device, _lib.lib()
    npos, nbatch = case["params"].shape[:2]
    used, extra = len(case["signal"]), 101
    rng = np.random.RandomState(7)
    signal = torch.from_numpy(np.concatenate([case["signal"], rng.normal(size=extra).astype(np.float32)])).to(dev)
    params, siglen = torch.from_numpy(case["params"]).to(dev), torch.from_numpy(case["siglen"]).to(dev)
    sig_off = torch.from_numpy(_offsets(case).astype(np.int64)).to(dev)
    nsignal = used + extra
    wsb = int(L.tk_squiggle_match_workspace_bytes(2, npos, nbatch, nsignal))
    assert wsb >= nsignal * (64 * C.lanes_r(npos) + 4) and wsb % 4 == 0
    whole, ws = _guarded_bytes(wsb, dev)
    cost = torch.full((nbatch,), float("nan"), device=dev)
    path = torch.full((nsignal,), PATH_SENTINEL, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.tk_squiggle_match_path_dev(_lib.ptr(params), _lib.ptr(signal), _lib.ptr(siglen), _lib.ptr(sig_off), npos,
                                      nbatch, nsignal, case["back_prob"], case["localpen"], case["minscore"],
                                      _lib.ptr(cost), _lib.ptr(path), _lib.ptr(ws), wsb, _lib.ptr(status),
                                      _lib.stream_ptr())
    _finish(rc, status, "tk_squiggle_match_path_dev")
    assert _guard_intact(whole, wsb), "a store behind the workspace"
    path = path.cpu().numpy()
    assert np.array_equal(path[:used], gold[name + "/path"]), np.flatnonzero(path[:used] != gold[name + "/path"])[:10]
    assert np.all(path[used:] == PATH_SENTINEL), "path entries behind sum(siglen) were written"
    np.testing.assert_allclose(cost.cpu().numpy(), gold[name + "/vcost"], rtol=1e-6)

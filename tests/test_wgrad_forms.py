"""Every load form and chain cut of the weight-gradient kernels (csrc/wgrad_common.h, instantiated by lstm_wgrad.hip and
gru_wgrad.hip), by name.  An entry of the table is (cell, loads, parts): the cell, which of wgrad_kernel's load forms the
launcher picks (tk_lab_*_wgrad_loads) and whether a run's rows are cut into one partial result or two
(tk_lab_*_wgrad_plan).  Every GPU call of this file is listed in `_gpu_calls`; a CPU test asks the two hooks for each
call's entry and proves that the calls reach all ten entries and the geometries named there.

On the GPU every call goes through the C ABI of the release libraries, in both directions, with dw_ih, dw_hh and the
bias results between guard bands over a sentinel and prefilled with NaN, and a workspace of exactly the size the query
returns, poisoned with NaN, a guard band behind it.  The accuracy criterion is tests/test_lstm_wgrad.py's: per result
the error against float64 on the host, relative to the largest reference entry, at most twice that of the GEMM path on
the same device tensors, plus 2e-6; the inputs are those tests' `_case`.  Each case prints one line that starts with
`r32|` (profiles/r32_wgrad_forms.txt keeps one run)."""
import ctypes
import functools
import os

import pytest
import torch

from taiyaki_amd import _lib
from tests import test_gru_wgrad as tg
from tests import test_lstm_wgrad as tl

CUS = 256
OK = 0
GUARD = 64                      # floats of sentinel on each side of a result and behind the workspace
SENTINEL = 7.0
TILE, CHAIN_ROWS = 128, 8192    # csrc/wgrad_common.h: WG_TILE, WG_CHAIN
GUARDED, FAST, VEC4 = 0, 1, 2   # ... and its load forms
LOADS = {GUARDED: "GUARDED", FAST: "FAST", VEC4: "VEC4"}
CELLS = ("lstm", "gru")
GATES = {"lstm": 4, "gru": 3}
OPS = {"lstm": ("dg", "x", "y"), "gru": ("dg", "dq", "x", "y")}
OUTS = {"lstm": ("w_ih", "w_hh", "b"), "gru": ("w_ih", "w_hh", "b_ih", "b_hh")}

TABLE = {(cell, loads, parts) for cell, forms in (("lstm", (FAST, GUARDED)), ("gru", (FAST, VEC4, GUARDED)))
         for loads in forms for parts in (1, 2)}

# (T, N, H, I, cu_count): more than 8192 rows per run, so every run is cut in two
CHAIN = [(643, 13, 16, 16, 1), (1269, 13, 16, 16, 4), (67, 123, 128, 128, 8), (66, 125, 96, 20, 6), (66, 125, 96, 21, 6)]
CHAIN_PLANS = {     # runs, parts, rows per run, rows per part, tiles down for (lstm, gru)
    CHAIN[0]: (1, 2, 8368, 4192, (1, 1)),       # 8359 rows: the second part ends ragged
    CHAIN[1]: (2, 2, 8256, 4128, (1, 1)),       # the last run has 8241 rows; neither 8256 nor 4128 is a multiple of 13
    CHAIN[2]: (1, 2, 8256, 4128, (4, 3)),
    CHAIN[3]: (1, 2, 8256, 4128, (3, 3)),
    CHAIN[4]: (1, 2, 8256, 4128, (3, 3)),
}
CHAIN_LOADS = {CHAIN[0]: (GUARDED, VEC4), CHAIN[1]: (GUARDED, VEC4), CHAIN[2]: (FAST, FAST), CHAIN[3]: (GUARDED, VEC4),
               CHAIN[4]: (GUARDED, GUARDED)}
LSTM_RAGGED = [(20, 13, 192, 192), (9, 11, 96, 21), (7, 5, 15, 3)]
ALIGN = [("lstm", (13, 20, 128, 128)), ("gru", (13, 20, 128, 128)), ("gru", (25, 70, 96, 20))]
GRU_SPLIT = [(13, 20, 128, 128), (25, 70, 96, 20), (9, 12, 96, 21)]        # FAST, VEC4, GUARDED
NONFINITE = [(13, 20, 128, 128), (25, 70, 96, 20)]


def _gpu_calls():
    """(group, cell, T, N, H, I, cu_count, aligned) of every kind of call the GPU tests below make."""
    for cell in CELLS:
        for s in CHAIN:
            yield ("chain", cell) + s + (True,)
        yield ("chain", cell) + CHAIN[0][:4] + (CUS, True)
    for s in LSTM_RAGGED:
        yield ("ragged", "lstm") + s + (CUS, True)
    for cell, s in ALIGN:
        for aligned in (True, False):
            yield ("align", cell) + s + (CUS, aligned)
    for s in GRU_SPLIT:
        yield ("split", "gru") + s + (CUS, True)
    for cell in CELLS:
        for s in NONFINITE:
            yield ("nonfinite", cell) + s + (CUS, True)


# ---------------------------------------------------------------------------------------------------------------------
# the hooks, and the table on the CPU
# ---------------------------------------------------------------------------------------------------------------------

def _lab(cell):
    """The lab build of the cell's library, for its host-side hooks only: the calls go through the release library."""
    if cell == "lstm":
        return _lib._load(os.path.join(_lib.CSRC, _lib.WGRAD_LAB_LIBNAME),
                          dict(_lib.WGRAD_SIGNATURES, **_lib.WGRAD_LAB_SIGNATURES))
    return _lib._load(os.path.join(_lib.CSRC, _lib.GRU_WGRAD_LAB_LIBNAME),
                      dict(_lib.GRU_WGRAD_SIGNATURES, **_lib.GRU_WGRAD_LAB_SIGNATURES))


def _release(cell):
    assert not _lib.is_lab()
    return _lib.wgrad_lib() if cell == "lstm" else _lib.gru_wgrad_lib()


def _loads(cell, H, I, aligned):
    return getattr(_lab(cell), "tk_lab_%s_wgrad_loads" % cell)(H, I, int(aligned))


def _plan(cell, T, N, H, I, cus):
    out = (ctypes.c_size_t * 8)()
    assert getattr(_lab(cell), "tk_lab_%s_wgrad_plan" % cell)(T, N, H, I, cus, out)
    return dict(zip(("tiles_m", "tiles_n", "runs", "parts", "run_rows", "part_rows", "grid", "slabs"), out))


def _entry(cell, T, N, H, I, cus, aligned):
    p = _plan(cell, T, N, H, I, cus)
    return (cell, _loads(cell, H, I, aligned), p["parts"]), p


def loads_rule(cell, aligned, H, I):
    """wgrad_loads restated: whole tiles and aligned operands take the 16-byte loads; widths that are multiples of 4
    take them with ragged tiles where the cell has that instantiation (the GRU); everything else is guarded."""
    if aligned and H % TILE == 0 and I % TILE == 0:
        return FAST
    if aligned and H % 4 == 0 and I % 4 == 0 and cell == "gru":
        return VEC4
    return GUARDED


def test_loads_hook_agrees_with_the_python_rule():
    sizes = (1, 2, 3, 4, 15, 16, 20, 21, 96, 124, 127, 128, 129, 192, 256, 384)
    seen = set()
    for cell in CELLS:
        for aligned in (False, True):
            for H in sizes:
                if cell == "gru" and H % 2:
                    continue        # (the GRU admits no odd H)
                for I in sizes:
                    got = _loads(cell, H, I, aligned)
                    assert got == loads_rule(cell, aligned, H, I), (cell, aligned, H, I, got)
                    seen.add((cell, got))
    assert seen == {(cell, loads) for cell, loads, _ in TABLE}
    # the release libraries have no such hook
    for name in (_lib.WGRAD_LIBNAME, _lib.GRU_WGRAD_LIBNAME):
        R = ctypes.CDLL(os.path.join(_lib.CSRC, name))
        assert not hasattr(R, "tk_lab_lstm_wgrad_loads") and not hasattr(R, "tk_lab_gru_wgrad_loads")


def test_the_gpu_cases_reach_every_entry_and_geometry():
    calls = list(_gpu_calls())
    reached = {}
    for group, cell, T, N, H, I, cus, aligned in calls:
        entry, p = _entry(cell, T, N, H, I, cus, aligned)
        assert p["tiles_n"] == -(-I // TILE) + -(-H // TILE) and p["tiles_m"] == -(-GATES[cell] * H // TILE)
        assert T * N <= 16500 and GATES[cell] * H <= 768
        reached.setdefault(entry, []).append((group, cell, T, N, H, I, cus, aligned, p))
    assert set(reached) == TABLE and len(TABLE) == 10, TABLE - set(reached)
    flat = [c for v in reached.values() for c in v]

    def some(pred):
        return any(pred(*c) for c in flat)

    assert some(lambda g, cell, T, N, H, I, cus, al, p: p["runs"] > 1 and p["parts"] == 2)
    # a ragged tile down M, alone and below whole ones
    assert some(lambda g, c, T, N, H, I, cus, al, p: GATES[c] * H % TILE and p["tiles_m"] == 1)
    assert some(lambda g, c, T, N, H, I, cus, al, p: GATES[c] * H % TILE and p["tiles_m"] > 1)
    assert some(lambda g, c, T, N, H, I, cus, al, p: I > TILE)      # more than one x tile
    assert some(lambda g, c, T, N, H, I, cus, al, p: H > TILE)      # more than one y tile
    # the LSTM's guarded form with several tiles each way of which the last are ragged
    assert some(lambda g, c, T, N, H, I, cus, al, p: c == "lstm" and _loads(c, H, I, al) == GUARDED and p["tiles_m"] > 1
                and I > TILE and I % TILE and H > TILE and H % TILE)
    # the guarded form chosen by alignment alone: the same shape, aligned, takes another form
    for cell, shape, other in (("lstm", (128, 128), FAST), ("gru", (128, 128), FAST), ("gru", (96, 20), VEC4)):
        assert some(lambda g, c, T, N, H, I, cus, al, p: c == cell and (H, I) == shape and not al
                    and _loads(c, H, I, al) == GUARDED and _loads(c, H, I, True) == other), (cell, shape)


def test_chain_cut_plans_are_these():
    """The plans of the chain-cut cases, literally (from the rule of wgrad_plan)."""
    for s, (runs, parts, run_rows, part_rows, tiles_m) in CHAIN_PLANS.items():
        T, N, H, I, cus = s
        for c, cell in enumerate(CELLS):
            entry, p = _entry(cell, T, N, H, I, cus, True)
            assert (p["runs"], p["parts"], p["run_rows"], p["part_rows"]) == (runs, parts, run_rows, part_rows), (s, cell, p)
            assert p["tiles_m"] == tiles_m[c] and p["slabs"] == runs * parts
            assert entry == (cell, CHAIN_LOADS[s][c], 2), (s, entry)
            assert p["run_rows"] > CHAIN_ROWS >= p["part_rows"]
    assert 643 * 13 == 8359 and 8359 - 4192 == 4167 and 4167 % 16         # the second part ends ragged
    assert 1269 * 13 - 8256 == 8241 and 8256 % 13 and 4128 % 13             # boundaries inside a time step
    p = _plan("gru", 66, 125, 96, 20, 6)
    assert 2 * 96 == 192 and 128 < 192 < 256 and p["tiles_m"] == 3        # the seam at 192 inside the second tile
    for cell in CELLS:      # the first shape with CUs to spare: 105 runs, one part
        entry, p = _entry(cell, 643, 13, 16, 16, CUS, True)
        assert (p["runs"], p["parts"], p["run_rows"]) == (105, 1, 80) and entry[2] == 1


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the reference, on the host
# ---------------------------------------------------------------------------------------------------------------------

def _host_case(cell, T, N, H, I):
    """tests/test_lstm_wgrad.py's and tests/test_gru_wgrad.py's `_case` (computed once, shared, never written)."""
    if cell == "lstm":
        dg, x, y, ref = tl._case(T, N, H, I)
        return dict(dg=dg, x=x, y=y), ref
    dg, dq, x, y, ref = tg._case(T, N, H, I)
    return dict(dg=dg, dq=dq, x=x, y=y), ref


def _gemms(cell, ops, reverse):
    if cell == "lstm":
        return tl._gemms(ops["dg"], ops["x"], ops["y"], reverse)
    return tg._gemms(ops["dg"], ops["dq"], ops["x"], ops["y"], reverse)


def _errors(got, ref):
    return {k: (got[k].double().cpu() - r).abs().max().item() / (r.abs().max().item() or 1.0) for k, r in ref.items()}


@functools.lru_cache(maxsize=None)
def _gru_cancelling_case(T, N, H, I):
    """tests/test_lstm_split_gemm.py's cancelling input for the GRU: dG and dq are minus themselves in the second half of
    the batch, x and y are 1 + 2^-10 randn, so the products of the leading parts cancel within every time step and dW_ih
    and dW_hh -- the rows that come from dq across the seam too -- are made of the correction terms."""
    g = torch.Generator().manual_seed(177 + T + N + H + I)
    hg, hq = torch.randn(T, N // 2, 3 * H, generator=g), torch.randn(T, N // 2, H, generator=g)
    dg, dq = torch.cat([hg, -hg], 1).contiguous(), torch.cat([hq, -hq], 1).contiguous()
    x = 1 + 2.0 ** -10 * torch.randn(T, N, I, generator=g)
    y = 1 + 2.0 ** -10 * torch.randn(T, N, H, generator=g)
    ops = dict(dg=dg, dq=dq, x=x, y=y)
    return ops, {reverse: tg._reference(dg, dq, x, y, reverse) for reverse in (False, True)}


@pytest.mark.parametrize("T,N,H,I", GRU_SPLIT)
def test_the_gru_cancelling_input_cancels(T, N, H, I):
    """The precondition of tests/test_lstm_split_gemm.py on these tensors: the largest entry of dW_ih and of dW_hh is
    below 0.05 max|dG| sqrt(T N) (it holds about sixtyfold)."""
    ops, ref = _gru_cancelling_case(T, N, H, I)
    bound = 0.05 * ops["dg"].abs().max().item() * (T * N) ** 0.5
    for r in ref.values():
        for k in ("w_ih", "w_hh"):
            print("cancelling %s %s: largest %.3g, bound %.3g" % ((T, N, H, I), k, r[k].abs().max().item(), bound))
            assert r[k].abs().max().item() < bound, (k, r[k].abs().max().item(), bound)


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------

def _off(t):
    """A copy of t that starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 8, device=t.device)
    shift = 1 + (-(flat.data_ptr() // 4)) % 4
    v = flat[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _aligned(ops):
    return all(t.data_ptr() % 16 == 0 for t in ops.values())


def _call(cell, ops, reverse, cus=CUS, shifted=None, finite=True):
    """One call of the release library on device tensors.  Every result lies between two guard bands (`shifted`: that
    result 4 bytes past a 16-byte boundary) and holds NaN before; the workspace is exactly the size asked, NaN before,
    with a guard band behind it.  After: the bands are intact and (`finite`) every result element is finite."""
    W = _release(cell)
    T, N, H = ops["y"].shape
    I = ops["x"].shape[2]
    dev = ops["y"].device
    G = GATES[cell] * H
    assert ops["dg"].shape == (T, N, G) and ops["x"].shape[:2] == (T, N)
    wsb = getattr(W, "tk_%s_weight_grad_workspace_bytes" % cell)(T, N, H, I, cus)
    assert wsb > 0 and wsb % 16 == 0
    ws = torch.full((wsb // 4 + GUARD,), float("nan"), device=dev)
    ws[wsb // 4:] = SENTINEL
    assert ws.data_ptr() % 16 == 0
    bufs, outs = {}, {}
    for k in OUTS[cell]:
        shape = (G,) if k.startswith("b") else (G, I if k == "w_ih" else H)
        n, s = G * (shape[1] if len(shape) == 2 else 1), int(k == shifted)
        bufs[k] = torch.full((GUARD + s + n + GUARD,), SENTINEL, device=dev)
        outs[k] = bufs[k][GUARD + s:GUARD + s + n].view(shape)
        outs[k].fill_(float("nan"))
        assert outs[k].data_ptr() % 16 == 4 * s
    p = [_lib.ptr(ops[k]) for k in OPS[cell]]
    o = [_lib.ptr(outs[k]) for k in OUTS[cell]]
    rc = getattr(W, "tk_%s_weight_grad_dev" % cell)(*p, T, N, H, I, int(reverse), cus, *o, _lib.ptr(ws), wsb,
                                                    _lib.stream_ptr())
    assert rc == OK
    torch.cuda.synchronize()
    assert bool((ws[wsb // 4:] == SENTINEL).all()), "the band behind the workspace"
    for k, buf in bufs.items():
        n = outs[k].numel()
        s = int(k == shifted)
        assert bool((buf[:GUARD + s] == SENTINEL).all()) and bool((buf[GUARD + s + n:] == SENTINEL).all()), ("guard bands", k)
        if finite:
            assert bool(torch.isfinite(outs[k]).all()), ("every element is overwritten with a finite value", k)
    return {k: v.clone() for k, v in outs.items()}


def _line(group, cell, shape, cus, aligned, figures):
    T, N, H, I = shape
    entry, p = _entry(cell, T, N, H, I, cus, aligned)
    print("\nr32|%s|%s|%s|parts %d|(T, N, H, I) = %s cus %d aligned %d|%d runs of %d rows, %d parts of %d, tiles %d x %d|%s"
          % (group, cell, LOADS[entry[1]], entry[2], shape, cus, aligned, p["runs"], p["run_rows"], p["parts"],
             p["part_rows"], p["tiles_m"], p["tiles_n"], figures))
    return entry


def _fmt(e):
    return " ".join("%s %.3g" % kv for kv in e.items())


def _compare(group, cell, shape, cus, ops, ref, dev, keys=None):
    """Both directions against float64 with the GEMM path as the yardstick; returns the results and the GEMMs' errors."""
    ops = {k: v.to(dev) for k, v in ops.items()}
    assert _aligned(ops)
    outs, e_gemm, e_hip = {}, {}, {}
    for reverse in (False, True):
        e_gemm[reverse] = _errors(_gemms(cell, ops, reverse), ref[reverse])
        outs[reverse] = _call(cell, ops, reverse, cus)
        e_hip[reverse] = _errors(outs[reverse], ref[reverse])
    _line(group, cell, shape, cus, True, "kernel fwd %s rev %s|GEMMs fwd %s rev %s"
          % (_fmt(e_hip[False]), _fmt(e_hip[True]), _fmt(e_gemm[False]), _fmt(e_gemm[True])))
    for reverse in (False, True):
        assert set(e_hip[reverse]) == set(OUTS[cell])
        for k in keys or OUTS[cell]:
            assert e_hip[reverse][k] <= 2 * e_gemm[reverse][k] + 2e-6, (cell, shape, cus, reverse, k, e_hip[reverse][k],
                                                                        e_gemm[reverse][k])
        if cell == "gru":
            assert torch.equal(outs[reverse]["b_hh"][:2 * shape[2]], outs[reverse]["b_ih"][:2 * shape[2]])
    return outs, e_gemm


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("T,N,H,I,cus", CHAIN)
def test_chain_cut_matches_float64_as_the_gemms_do(gpu_device, cell, T, N, H, I, cus):
    """More than 8192 rows per run: every run is cut into two partial results (test_chain_cut_plans_are_these)."""
    assert _entry(cell, T, N, H, I, cus, True)[0][2] == 2
    ops, ref = _host_case(cell, T, N, H, I)
    _compare("chain", cell, (T, N, H, I), cus, ops, ref, gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS)
def test_one_run_in_two_parts_agrees_with_105_runs(gpu_device, cell):
    """(643, 13, 16, 16) at cu_count = 1 (one run, two parts) and at 256 (105 runs, one part): both match float64 and
    they agree within the same bound, as test_forced_runs_agree_and_match_float64 asks of its runs."""
    shape = CHAIN[0][:4]
    ops, ref = _host_case(cell, *shape)
    assert _entry(cell, *shape, CUS, True)[0][2] == 1 and _entry(cell, *shape, 1, True)[0][2] == 2
    cut, e_gemm = _compare("chain", cell, shape, 1, ops, ref, gpu_device)
    many, _ = _compare("chain", cell, shape, CUS, ops, ref, gpu_device)
    for reverse in (False, True):
        for k, r in ref[reverse].items():
            diff = (cut[reverse][k] - many[reverse][k]).abs().max().item() / r.abs().max().item()
            assert diff <= 2 * e_gemm[reverse][k] + 2e-6, (reverse, k, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", LSTM_RAGGED)
def test_lstm_guarded_form_on_ragged_tiles(gpu_device, T, N, H, I):
    """M = 768 with two x and two y tiles of which the second holds 64 columns; M = 384 with I = 21; M = 60, I = 3 with
    an odd H: the LSTM has no 16-byte form for ragged tiles and takes the guarded loads at all three."""
    assert _entry("lstm", T, N, H, I, CUS, True)[0] == ("lstm", GUARDED, 1)
    ops, ref = _host_case("lstm", T, N, H, I)
    _compare("ragged", "lstm", (T, N, H, I), CUS, ops, ref, gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("cell,shape", ALIGN)
def test_each_tensor_four_bytes_off_alignment(gpu_device, cell, shape):
    """Each operand in turn 4 bytes past a 16-byte boundary (the launcher then takes the guarded loads), then each
    result in turn: the bits of the aligned call.  The loads differ; the arithmetic does not."""
    H, I = shape[2:]
    assert _loads(cell, H, I, True) != GUARDED and _loads(cell, H, I, False) == GUARDED
    ops = {k: v.to(gpu_device) for k, v in _host_case(cell, *shape)[0].items()}
    assert _aligned(ops)
    calls = 0
    for reverse in (False, True):
        want = _call(cell, ops, reverse)
        for name in OPS[cell]:
            moved = dict(ops, **{name: _off(ops[name])})
            assert not _aligned(moved)
            got = _call(cell, moved, reverse)
            for k in OUTS[cell]:
                assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (reverse, name, k)
            calls += 1
        for name in OUTS[cell]:
            got = _call(cell, ops, reverse, shifted=name)
            for k in OUTS[cell]:
                assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (reverse, name, k)
            calls += 1
    _line("align", cell, shape, CUS, False, "%d calls with one tensor off alignment give the aligned call's bits" % calls)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", GRU_SPLIT)
def test_gru_cancelling_leading_parts_leave_the_corrections(gpu_device, T, N, H, I):
    """The GRU cell on tests/test_lstm_split_gemm.py's cancelling input, one shape per load form: the operand that comes
    from dq across the seam, and the 16-byte staging that loads column 0 and zeroes it.  db_ih and db_hh are about 0
    here and have no scale: the other cases cover them."""
    ops, ref = _gru_cancelling_case(T, N, H, I)
    bound = 0.05 * ops["dg"].abs().max().item() * (T * N) ** 0.5
    for r in ref.values():
        assert max(r["w_ih"].abs().max().item(), r["w_hh"].abs().max().item()) < bound      # (they did cancel)
    assert _entry("gru", T, N, H, I, CUS, True)[0][1] == {(128, 128): FAST, (96, 20): VEC4, (96, 21): GUARDED}[(H, I)]
    _compare("split cancelling", "gru", (T, N, H, I), CUS, ops, ref, gpu_device, keys=("w_ih", "w_hh"))


@pytest.mark.gpu
def test_gru_magnitudes_far_from_one(gpu_device):
    """dG, dq x 1e-6 and x, y x 1e3: the parts are relative to each element, not to the tile."""
    shape = (13, 20, 128, 128)
    ops = dict(_host_case("gru", *shape)[0])
    ops = {k: v * (1e-6 if k in ("dg", "dq") else 1e3) for k, v in ops.items()}
    ref = {reverse: tg._reference(ops["dg"], ops["dq"], ops["x"], ops["y"], reverse) for reverse in (False, True)}
    _compare("split magnitudes", "gru", shape, CUS, ops, ref, gpu_device)


def _only(got, clean, hit, what):
    """`hit`: result -> boolean mask of the elements that hold no finite value; every other element is clean's bits."""
    for k in clean:
        mask = hit.get(k)
        if mask is None:
            assert torch.equal(got[k].view(torch.int32), clean[k].view(torch.int32)), (what, k)
            continue
        mask = mask.to(got[k].device)
        assert bool(mask.any()) and not bool(torch.isfinite(got[k][mask]).any()), (what, k)
        assert torch.equal(got[k][~mask].view(torch.int32), clean[k][~mask].view(torch.int32)), (what, k)


def _mask(shape, row=None, col=None):
    m = torch.zeros(shape, dtype=torch.bool)
    if col is not None:
        m[:, col] = True
    elif len(shape) == 1:
        m[row] = True
    else:
        m[row, :] = True
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("T,N,H,I", NONFINITE)
def test_a_non_finite_element_stays_where_the_header_says(gpu_device, cell, T, N, H, I):
    """One non-finite element at a step that is neither the first nor the last.  inf in dgates at column m: row m of
    dW_ih, row m of dW_hh and the bias sums' entry m hold no finite value (the GRU: m below 2H, where dW_hh's rows come
    from dgates).  nan in x at column i: column i of dW_ih.  -inf in y at column j: column j of dW_hh.  The GRU's dq,
    nan at column j: row 2H + j of dW_hh and db_hh[2H + j].  Every other element is the clean call's bits."""
    G = GATES[cell] * H
    t0, n0 = T // 2, N // 3
    assert 0 < t0 < T - 1
    m, i, j = H + 3, I - 1, H // 2 + 1
    assert m < 2 * H
    ops = {k: v.to(gpu_device) for k, v in _host_case(cell, T, N, H, I)[0].items()}
    bias = ("b",) if cell == "lstm" else ("b_ih", "b_hh")
    places = [("dg", m, float("inf"), dict(w_ih=_mask((G, I), row=m), w_hh=_mask((G, H), row=m),
                                           **{b: _mask((G,), row=m) for b in bias})),
              ("x", i, float("nan"), dict(w_ih=_mask((G, I), col=i))),
              ("y", j, float("-inf"), dict(w_hh=_mask((G, H), col=j)))]
    if cell == "gru":
        places.append(("dq", j, float("nan"), dict(w_hh=_mask((G, H), row=2 * H + j), b_hh=_mask((G,), row=2 * H + j))))
    for reverse in (False, True):
        clean = _call(cell, ops, reverse)
        for name, col, value, hit in places:
            bad = ops[name].clone()
            bad[t0, n0, col] = value
            got = _call(cell, dict(ops, **{name: bad}), reverse, finite=False)
            _only(got, clean, hit, (reverse, name))
    _line("nonfinite", cell, (T, N, H, I), CUS, True, "%d placements, both directions: only the rows and columns named"
          % len(places))

"""The tall form of the weight-gradient kernel (csrc/wgrad_common.h, wgrad_kernel<Cell, FAST, true>): a workgroup owns
two row tiles over half of a run's partial results where a square one owns one tile over all of them.  The launcher
takes it where the loads are FAST, the row tiles come in pairs and the parts of a run in halves (wgrad_tall); a CPU test
restates that rule from the two lab hooks.  Every partial result is made of the same sums in the same order in either
form, so on the GPU the aligned call (tall by the rule) gives the bits of the same call with every operand 4 bytes off
alignment (guarded loads, always square), and both meet tests/test_lstm_wgrad.py's accuracy criterion against float64.
The calls, the guard bands and the NaN-poisoned results and workspace are tests/test_wgrad_forms.py's.

Which form a launch took cannot be seen through the C ABI: profiles/r43_wgrad_tall_test_trace.txt keeps a kernel trace
of this file that shows both kernels."""
import pytest
import torch

from tests import test_wgrad_forms as tf

FAST = tf.FAST
# (cell, T, N, H, I, cu_count)
TALL = [("lstm", 67, 123, 128, 128, 8),     # 1 run of 8256 rows in 2 parts of 4128; K = 8241 ends the second part ragged
        ("lstm", 134, 123, 128, 128, 16),   # 2 runs x 2 parts
        ("gru", 67, 123, 256, 128, 18)]     # M = 768: three pairs of row tiles, the seam at 512 between two of them
SQUARE = ("lstm", 520, 64, 128, 128, 8)     # 1 run in 5 parts
FLAGSHIP = ("lstm", 800, 128, 256, 256, 256)
PLANS = {TALL[0]: (4, 1, 2, 8256, 4128), TALL[1]: (4, 2, 2, 8256, 4128), TALL[2]: (6, 1, 2, 8256, 4128),
         SQUARE: (4, 1, 5, 33280, 6656), FLAGSHIP: (8, 8, 2, 12800, 6400)}     # tiles down, runs, parts, rows per run and part


def tall_rule(cell, T, N, H, I, cus, aligned=True):
    """wgrad_tall restated from the hooks: FAST loads, an even number of row tiles, an even number of parts per run."""
    (_, loads, parts), p = tf._entry(cell, T, N, H, I, cus, aligned)
    return loads == FAST and p["tiles_m"] % 2 == 0 and parts % 2 == 0


def test_the_rule_takes_these_cases():
    for case, want in PLANS.items():
        p = tf._plan(*case)
        assert (p["tiles_m"], p["runs"], p["parts"], p["run_rows"], p["part_rows"]) == want, (case, p)
    for case in TALL + [FLAGSHIP]:
        assert tall_rule(*case), case
        assert not tall_rule(*case, aligned=False), case        # (the guarded loads are always square)
    assert not tall_rule(*SQUARE) and tf._loads(*SQUARE[:1], SQUARE[3], SQUARE[4], True) == FAST and PLANS[SQUARE][2] % 2
    # the ragged end and the part boundary inside a time step; the GRU's seam at 2H between two pairs of tiles
    assert 67 * 123 == 8241 and 8241 % 16 and 8256 % 123 and 4128 % 123
    assert (2 * 256) % (2 * tf.TILE) == 0
    # an odd number of row tiles stays square whatever the parts: the GRU at H 128
    assert not tall_rule("gru", 67, 123, 128, 128, 6) and tf._plan("gru", 67, 123, 128, 128, 6)["parts"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("cell,T,N,H,I,cus", TALL)
def test_tall_matches_float64_and_the_square_forms_bits(gpu_device, cell, T, N, H, I, cus):
    """(a) the accuracy criterion in both directions; (b) the aligned call's results, as bits, are those of the call with
    every operand 4 bytes off alignment."""
    assert tall_rule(cell, T, N, H, I, cus)
    ops, ref = tf._host_case(cell, T, N, H, I)
    outs, _ = tf._compare("tall", cell, (T, N, H, I), cus, ops, ref, gpu_device)
    dev_ops = {k: v.to(gpu_device) for k, v in ops.items()}
    moved = {k: tf._off(v) for k, v in dev_ops.items()}
    assert not any(t.data_ptr() % 16 == 0 for t in moved.values())
    for reverse in (False, True):
        got = tf._call(cell, moved, reverse, cus)
        for k in tf.OUTS[cell]:
            same = torch.equal(got[k].view(torch.int32), outs[reverse][k].view(torch.int32))
            print("tall|%s %s cus %d reverse %d %s: bits of the square form %s" % (cell, (T, N, H, I), cus, reverse, k, same))
            assert same, (cell, reverse, k)


@pytest.mark.gpu
def test_an_odd_number_of_parts_stays_square(gpu_device):
    cell, T, N, H, I, cus = SQUARE
    assert not tall_rule(*SQUARE)
    ops, ref = tf._host_case(cell, T, N, H, I)
    tf._compare("tall: odd parts", cell, (T, N, H, I), cus, ops, ref, gpu_device)

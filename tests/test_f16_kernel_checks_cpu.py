"""The checks of tests/f16_kernel_ref.py bite, and a right kernel can pass them: for every case tests/test_gpu_f16_kernels.py runs
on the GPU (the glue kernels and the conv16 epilogue and addressing forms), a float32 CPU computation of the op rounded once to the output type passes every check (the rms rule against itself,
the sigmoid bound with c = |v| + 8), and every numpy mutant of the op that the case's data can tell apart is refused.  No element
is left out of any check."""
import numpy as np
import pytest

import f16_kernel_ref as R


@pytest.mark.parametrize("case_id", R.CASE_IDS + R.CONV_CASE_IDS)
def test_float32_stand_in_passes_and_mutants_are_refused(case_id):
    c = R.case(case_id)
    good = c.buffer(np.float32)
    fig = R.check(c, good)
    mask, _ = c.compute(np.float64, None)
    assert fig["n"] == int(mask.sum()) - (int(c.zero.sum()) if getattr(c, "zero", None) is not None else 0)   # nothing masked out
    assert fig["n"] > 0
    muts = R.mutants_of(c)
    assert muts, "no mutant for " + c.name
    for m in muts:
        bad = c.buffer(np.float32, m)
        assert not np.array_equal(c.to_bits(bad), c.to_bits(good)), "%s: mutant %s changes nothing" % (c.name, m)
        with pytest.raises(AssertionError):
            R.check(c, bad)


def test_every_op_has_a_case_and_a_mutant():
    ops = {R.case(i).op for i in R.CASE_IDS}
    assert ops == set(range(len(R.OPS)))


def test_the_named_conv_mutants_are_exercised():
    """every wrong variant the conv cases are there to catch is refused by at least one of them (the loop above ran them)"""
    seen = {m for i in R.CONV_CASE_IDS for m in R.mutants_of(R.case(i))}
    assert {"residual_at_output_pitch", "lab_before_act", "pad_nonzero", "tap_dropped_last_column", "taps_swapped", "source_at_cin_pitch",
            "phase_b_a"} <= seen
    routes = {R.case(i).route for i in R.CONV_CASE_IDS}
    assert routes == {R.K_CONV16, R.K_CONV16V2, R.K_GEMM16P, R.K_CONV16V2 | R.ROUTE_DOT}


def test_a_phase_that_touches_another_phases_pixels_is_refused():
    c = R.case("conv16x-phase-dot")
    before = np.concatenate([c.in_place, np.zeros(64, np.float32)])
    done = c.buffer(np.float32).ravel()          # the map after all four phases
    own = c.phase_pixels(1, 0)
    after = before.copy()
    after[own] = done[own]
    fig = c.check_step(before, after, 1, 0)
    assert fig["n"] == own.size
    for a, b in ((0, 1), (0, 0), (1, 1)):
        with pytest.raises(AssertionError):
            c.check_step(before, after, a, b)
    skipped = after.copy()
    skipped[own[5]] = before[own[5]]             # one pixel of the phase never updated
    with pytest.raises(AssertionError):
        c.check_step(before, skipped, 1, 0)
    twice = after.copy()
    twice[own[5]] = 0.5 * (after[own[5]] + 2 * after[own[5]] - before[own[5]])   # one pixel updated a second time
    with pytest.raises(AssertionError):
        c.check_step(before, twice, 1, 0)
    spare = after.copy()
    spare[-1] = 1.0
    with pytest.raises(AssertionError):
        c.check_step(before, spare, 1, 0)


def test_a_write_outside_the_output_is_refused():
    c = R.case("upsample_into16-shift1-scale0")
    out = c.buffer(np.float32).reshape(c.shape())
    for r, col in ((0, 0), (c.out_rows, c.ip[4]), (c.out_rows + 63, c.out_ld - 1)):   # another slice, the first and last spare row
        bad = out.copy()
        bad[r, col] = 0.5
        with pytest.raises(AssertionError):
            R.check(c, bad)


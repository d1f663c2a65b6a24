"""The checks of tests/fpn_kernel_ref.py bite, and a right kernel can pass them: for every case tests/test_gpu_fpn_kernels.py runs
on the GPU, a float32 CPU computation of the plain form passes every check, so does a float32 computation in the kernels' own form
(pre-summed float32 phase / class weights, composed per-image weights, float32 accumulation), whose rms error stays within twice the
plain form's, and every listed mutant -- one plausible error applied to the kernels' form -- is refused by at least one case.  No
element of any buffer is left out of a check.

MUTANT_FLOOR holds, per mutant, how it is refused and a floor for the largest err / bound over the cases that refuse it: the
figures of the table in docs/HISTORY.md rounded down to one digit, asserted here as lower bounds, so a change that weakens a
case's hold on a mutant shows.  The rms rule is applied per output buffer (the conv output, the pool sums and the composed
weights each on their own)."""
import numpy as np
import pytest

import fpn_kernel_ref as R

# mutant -> (how at least one case refuses it, the largest err / bound over the refusing cases is at least this)
MUTANT_FLOOR = {
    "phase_pxpy": ("bound", 6e3), "phase_taps_swapped": ("bound", 1e4), "rowclass3_interior": ("bound", 8e3),
    "quarter_index_off": ("bound", 9e3), "lower_parity_inverted": ("bound", 3e4), "lower_at_yx": ("bound", 4e4),
    "bias_twice": ("bound", 5e3), "fine_scale_img0": ("bound", 3e3), "wf_img0": ("bound", 3e3), "compose_no_se": ("bound", 3e4),
    "compose_pad_nonzero": ("pad", 0), "pool_premask": ("bound", 7e3), "se_tiles_max_tiles": ("nan", 0),
    "se_tiles_max_pix": ("bound", 2e4), "head_levels_reversed": ("bound", 4e3), "upsample_yp1": ("bound", 1e8),
    "lateral_scale_after_add": ("bound", 1e5), "tail_dydx_transposed": ("bound", 3e7), "tail_no_relu": ("bound", 6e5),
    "tail_rows_swapped": ("bound", 2e7),
}


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_float32_stand_in_and_the_kernels_form_pass_every_check(case_id):
    c = R.case(case_id)
    plain = c.buffers(np.float32)
    fig = R.check(c, plain, f32=plain)
    assert fig["n"] == sum(int(o.mask.sum()) for o in c.reference()) > 0   # nothing masked out
    kern = c.buffers(np.float32, form="kernel")
    figk = R.check(c, kern, f32=plain)    # (the rms rule inside: the kernels' form within twice the plain float32 form)
    assert figk["worst"] <= 1
    ratios = {k: round(v, 3) for k, v in figk.items() if k.startswith("ratio")}   # kernel form / plain form, per output buffer
    assert all(r <= 2 for r in ratios.values())
    print("FIG %s plain worst=%.3g kernel-form worst=%.3g rms ratios=%s" % (case_id, fig["worst"], figk["worst"], ratios))


def refusal(c, bad):
    """how check() refuses the buffers `bad`: None if it does not"""
    try:
        R.check(c, bad)
    except AssertionError as e:
        msg = str(e)
        if "outside the op's output" in msg:
            return "canary"
        if "pad elements" in msg:
            return "pad"
        if "non-finite" in msg:
            return "nan"
        if "rms error" in msg:
            return "rms"
        return "bound"
    return None


def excess(c, bad):
    """the largest err / bound of the buffers over all outputs (inf for a non-finite value)"""
    worst = 0.0
    for o, b in zip(c.reference(), bad):
        m = o.mask & ~o.zero
        g = np.asarray(b, np.float32).reshape(o.shape)[m].astype(np.float64)
        if not np.isfinite(g).all():
            return float("inf")
        worst = max(worst, float(np.max(np.abs(g - o.v[m]) / o.bound[m])))
    return worst


@pytest.mark.parametrize("mut", list(R.MUTANTS))
def test_every_mutant_is_refused(mut):
    refused = []
    for case_id in R.MUTANTS[mut]:
        c = R.case(case_id)
        good, bad = c.buffers(np.float32, form="kernel"), c.buffers(np.float32, mut, form="kernel")
        changed = any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(good, bad))
        assert changed, "%s: mutant %s changes nothing" % (c.name, mut)
        how = refusal(c, bad)
        if how:
            refused.append((case_id, how, excess(c, bad)))
    assert refused, "no case refuses %s: the cases are too weak" % mut
    print("MUTANT %-24s %s" % (mut, "; ".join("%s: %s, %.3g bounds" % r for r in refused)))
    how, floor = MUTANT_FLOOR[mut]
    assert how in {h for _, h, _ in refused}, (mut, refused)
    assert max(x for _, _, x in refused) >= floor, (mut, refused)


def test_every_op_has_a_case_and_every_listed_mutant_a_case():
    assert {R.case(i).op for i in R.CASE_IDS} == set(R.OPS)
    assert set(MUTANT_FLOOR) == set(R.MUTANTS)
    assert len(R.MUTANTS) >= 20 and all(set(v) <= set(R.CASE_IDS) and v for v in R.MUTANTS.values())
    assert {R.case(i).info for i in R.CASE_IDS if R.case(i).op == "phase"} == set(R.INSTANCE_NAMES)


def test_a_write_outside_the_output_is_refused():
    c = R.case("phase-340")
    good = c.buffers(np.float32)
    y, pool = c.reference()
    spots = [(0, y.shape[0] - 64, 0), (0, y.shape[0] - 1, 23)]                       # the first and last spare row of y
    unwritten = np.flatnonzero(~pool.mask[:pool.shape[0] - 64].any(axis=1))          # a tile an image does not have
    assert unwritten.size
    spots.append((1, int(unwritten[0]), 5))
    for k, r, col in spots:
        bad = [b.copy() for b in good]
        bad[k][r, col] = 0.5
        assert refusal(c, bad) == "canary"


def test_the_tail_spans_saturated_logits_and_the_reference_conv_is_the_plain_one():
    c = R.case("tail")
    c.reference()
    assert 10 <= c.logit_span <= 16   # about +-12: both saturated ends and the middle
    # conv3 against a direct loop at a few pixels: the reference itself is the plain zero-padded conv
    rng = np.random.default_rng(0)
    x, w = rng.uniform(-1, 1, (5, 4, 3)), rng.uniform(-1, 1, (2, 3, 3, 3))
    got = R.conv3(x, w, np.float64)
    for (yy, xx) in ((0, 0), (4, 3), (2, 1)):
        want = np.zeros(2)
        for dy in range(3):
            for dx in range(3):
                sy, sx = yy + dy - 1, xx + dx - 1
                if 0 <= sy < 5 and 0 <= sx < 4:
                    want += w[:, :, dy, dx] @ x[sy, sx]
        assert np.allclose(got[yy, xx], want, rtol=0, atol=1e-13)

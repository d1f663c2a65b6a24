"""The checks of tests/cls_kernel_ref.py bite, and a right kernel can pass them: for every case tests/test_gpu_cls_kernels.py runs on
the GPU, the float32 CPU form (torch) passes every check, and every listed mutant -- one plausible error applied to the float32
form -- is refused by at least one case.  No element of any buffer is left out of a check.

MUTANT_FLOOR holds, per mutant, how it is refused and a floor for the largest err / bound over the cases that refuse it: what
this file measures on the CPU, rounded down to one digit, asserted as a lower bound so that a change which weakens a case's hold
on a mutant shows (0 where the refusal is not a bound: a NaN where an unwritten tile keeps the canary or a pad channel reaches the
output, an index, a bit pattern).  The blocks' bounds are wide (a right kernel sits at 1e-4 .. 2e-2 of them): the weakest hold, the
squeeze-excite slope, is still 30 bounds."""
import numpy as np
import pytest
import torch

import cls_kernel_ref as R

# mutant -> (how at least one case refuses it, the largest err / bound over the refusing cases is at least this)
MUTANT_FLOOR = {
    "dw_tap_dropped": ("bound", 2e4), "dw_taps_transposed": ("bound", 6e4), "stride_in_w": ("bound", 7e4), "pool_div_hin": ("bound", 5e3),
    "se_scale_prev_crop": ("bound", 2e3), "se_slope_sixth": ("bound", 3e1), "shortcut_missing": ("bound", 8e3), "shortcut_twice": ("bound", 8e3),
    "exp_bias_next_slice": ("bound", 6e4), "last_tile_unwritten": ("nan", 0), "exp_pad_nonzero": ("nan", 0),
    "pad0": ("bound", 8e5), "u8_no_bgr": ("bound", 6e5), "col64_zero": ("bound", 2e5), "tile_rows_swapped": ("bound", 1e6),
    "chunk_twice": ("bound", 1e5), "fc2_remainder_dropped": ("bound", 2e5), "residual_before_clamp": ("bound", 7e4),
    "maxpool_col_plus2": ("exact", 0), "tie_to_higher": ("index", 0),
}


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_float32_cpu_form_passes_every_check(case_id):
    c = R.case(case_id)
    f32 = c.buffers(torch.float32)
    fig = R.check(c, f32, f32=f32)
    assert fig["n"] == sum(int(o.mask.sum()) for o in c.reference()) > 0   # nothing masked out
    assert fig["worst"] <= 1
    for o, b in zip(c.reference(), f32):
        assert b.shape == o.shape and not o.mask[-64:].any()
        arith = o.mask & ~o.zero
        assert o.kind != "arith" or (o.bound[arith] > 0).all()
    print("FIG %s float32 worst err/bound=%.3g" % (case_id, fig["worst"]))


def refusal(c, bad):
    """how check() refuses the buffers `bad`: None if it does not"""
    try:
        R.check(c, bad)
    except AssertionError as e:
        msg = str(e)
        for key, how in (("outside the op's output", "canary"), ("pad elements", "pad"), ("non-finite", "nan"), ("rms error", "rms"),
                         ("indices differ", "index"), ("bits differ", "exact")):
            if key in msg:
                return how
        return "bound"
    return None


def excess(c, bad):
    """the largest err / bound of the buffers over the arithmetic outputs (inf for a non-finite value)"""
    worst = 0.0
    for o, b in zip(c.reference(), bad):
        m = o.mask & ~o.zero
        if o.kind != "arith":
            continue
        with np.errstate(invalid="ignore"):
            g = b.view(np.float32).reshape(o.shape)[m].astype(np.float64)
        if not np.isfinite(g).all():
            return float("inf")
        worst = max(worst, float(np.max(np.abs(g - o.v[m]) / o.bound[m])))
    return worst


@pytest.mark.parametrize("mut", list(R.MUTANTS))
def test_every_mutant_is_refused(mut):
    refused = []
    for case_id in R.MUTANTS[mut]:
        c = R.case(case_id)
        good, bad = c.buffers(torch.float32), c.buffers(torch.float32, mut)
        assert any(not np.array_equal(a, b) for a, b in zip(good, bad)), "%s: mutant %s changes nothing" % (c.name, mut)
        how = refusal(c, bad)
        if how:
            refused.append((case_id, how, excess(c, bad)))
    assert refused, "no case refuses %s: the cases are too weak" % mut
    print("MUTANT %-24s %s" % (mut, "; ".join("%s: %s, %.3g bounds" % r for r in refused)))
    how, floor = MUTANT_FLOOR[mut]
    assert how in {h for _, h, _ in refused}, (mut, refused)
    assert max(x for _, _, x in refused) >= floor, (mut, refused)


def test_every_listed_mutant_has_a_floor_and_the_cases_cover_the_entries():
    assert set(MUTANT_FLOOR) == set(R.MUTANTS) and len(R.MUTANTS) >= 20
    assert all(v and set(v) <= set(R.CASE_IDS) for v in R.MUTANTS.values())
    assert {R.case(i).op for i in R.GLUE_IDS} == set(R.GLUE_OPS)
    assert len(R.BLOCK_IDS) == 22 + 18 and len(R.STEM_IDS) == 3


def test_the_stated_instances_are_what_the_shape_function_picks():
    """every block case's bracketed instance against nn::cls_block_shape restated; the fused cases reach all three workgroup
    shapes, each with k 3 and 5, stride 1 and 2 and squeeze-excite on and off"""
    seen = {}
    for i in R.BLOCK_IDS:
        c = R.case(i)
        want = R.cls_route(c.k, c.sh, c.cin, c.mid, c.cout, c.H, c.W)[0] if c.form else R.SERIES
        assert c.info == want, (i, c.info, want)
        assert c.form or c.info == R.SERIES
        if c.info != R.SERIES:
            seen.setdefault(c.info, set()).add((c.k, c.sh, c.se))
    for inst in (R.SWZ9, R.PAD9, R.PAD5):
        combos = seen[inst]
        assert {k for k, _, _ in combos} == {3, 5} and {se for _, _, se in combos} == {True, False}, (inst, combos)
        assert {sh for _, sh, _ in combos} == {1, 2}, (inst, combos)
    # the 96 KB switch: the two cases sit next to each other, one row of pixels apart
    (pb, sb, xb), (pa, sa, xa) = (R.cls_route(3, 1, 8, 32, 8, h, 16)[1] for h in (43, 44))
    assert 0 <= 96 * 1024 - (pb + sb + xb) < 2208 and 0 < (pa + sa + xa) - 96 * 1024 < 2208
    # 40 / 41 / 72 / 73 row tiles
    tiles = lambda i: (R.case(i).Ho * R.case(i).W + 15) // 16   # noqa: E731
    assert [tiles(i) for i in ("edge-40tiles-pad5", "edge-41tiles-pad9-k3", "edge-72tiles-swz-k5se", "edge-72tiles-swz-k3", "refused-73tiles")] == [40, 41, 72, 72, 73]


def test_a_write_outside_the_output_is_refused():
    for cid, k, r, col in (("blk2-f1", 0, 3 * 6 * 96, 0), ("blk2-f1", 0, 3 * 6 * 96 + 63, 7), ("avgpool-120", 0, 0, 120), ("avgpool-120", 0, 5, 239),
                           ("softmax-2", 0, 8, 0), ("se-c200-r0-a1", 1, 685, 3), ("argmax-257", 1, 8, 0)):
        c = R.case(cid)
        bad = [b.copy() for b in c.buffers(torch.float32)]
        bad[k][r, col] = np.float32(0.5).view(np.uint32)
        assert refusal(c, bad) == "canary", (cid, r, col)
    c = R.case("se-c200-r0-a0")       # a scale past C that is not +0
    bad = [b.copy() for b in c.buffers(torch.float32)]
    bad[0][1, 200] = np.float32(-0.0).view(np.uint32)
    assert refusal(c, bad) == "pad"


def test_the_references_are_the_plain_operations():
    """the depthwise conv and the stem against direct loops at a few pixels; the squeeze-excite cases reach both clamps and the
    linear part of the hard-sigmoid (asserted where the reference is built)"""
    rng = np.random.default_rng(0)
    x, w, b = rng.uniform(-1, 1, (1, 5, 4, 3)), rng.uniform(-1, 1, (3, 5, 5)), rng.uniform(-1, 1, 3)
    got = R.dwconv(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), 2).numpy()
    assert got.shape == (1, 3, 4, 3)
    for (oy, ox) in ((0, 0), (2, 3), (1, 2)):
        want = b.copy()
        for dy in range(5):
            for dx in range(5):
                sy, sx = 2 * oy + dy - 2, ox + dx - 2
                if 0 <= sy < 5 and 0 <= sx < 4:
                    want += w[:, dy, dx] * x[0, sy, sx]
        assert np.allclose(got[0, oy, ox], want, rtol=0, atol=1e-13)
    c = R.case("stem16")
    y = c.reference()[0]
    offs = R.offsets(c.imgs)
    i, (h, ww) = 4, c.imgs[4]                      # the 5 x 3 image: output 3 x 2
    oo = R.offsets([((a + 1) // 2, (bb + 1) // 2) for a, bb in c.imgs])
    img = c.x4[offs[i]:offs[i + 1], :3].astype(np.float64).reshape(h, ww, 3)
    for (oy, ox) in ((0, 0), (2, 1)):
        want = c.b.astype(np.float64).copy()
        for dy in range(3):
            for dx in range(3):
                sy, sx = 2 * oy + dy - 1, 2 * ox + dx - 1
                if 0 <= sy < h and 0 <= sx < ww:
                    want += c.w[:, :, dy, dx].astype(np.float64) @ img[sy, sx]
        assert np.allclose(y.v[oo[i] + oy * 2 + ox, :16], want, rtol=0, atol=1e-13)
    for cid in R.CASE_IDS:
        cc = R.case(cid)
        if getattr(cc, "se", False) or cid.startswith("se-"):
            cc.reference()
            assert min(cc.regions) > 0

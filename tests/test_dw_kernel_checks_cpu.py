"""The checks of tests/dw_kernel_ref.py bite, and a right kernel can pass them: for every case tests/test_gpu_dw_kernels.py runs on
the GPU the float32 CPU form (torch) passes every check with no element of any buffer left out, and every listed mutant -- one
plausible error applied to the float32 form -- is refused by at least one named case.  The case table is held to the host-side
plan (tests/plan_driver.py: nn::dw_plan, nn::lc_plan, nn::gemm_plan compiled with g++): the instance each case names is the one the
plan picks, the cases reach every instance the networks reach, and the instances of dwconv()'s switch that no case reaches are
pinned by name.

MUTANT_FLOOR holds, per mutant, how it is refused and a floor for the largest err / bound over the cases that refuse it: what this
file measures on the CPU, rounded down to one digit, asserted as a lower bound so that a change which weakens a case's hold on a
mutant shows (0 where the refusal is not a bound: a NaN where an unwritten strip keeps the canary or a foreign partial is summed
in, a pad element that is not +0, a changed word outside the output).  The blocks' composed bounds are wide (a right kernel sits at
1e-3 .. 0.1 of them), so a wrong scale is refused by tens to hundreds of bounds only; the rms rule is the tight check there.

"4-row strips where the plan says 3" is two mutants (dw_kernel_ref.strips_mutant): the row kernel instantiated with R + 1, and
k_se_fc handed strip_R = R + 1.  Both kernels count an image's strips from the image's own height, so they bite on the one height
at which ceil(H / 3) != ceil(H / 4): the wide 4-row image every 6-row batch carries (test_the_case_table_against_the_plan holds
that).  On the 3-row maps (det-s6.1-h3, rec-s6.2-h3, rec-s6.3-h3) no image can tell R = 3 from 4: every image is one strip tall."""
import ctypes as C

import numpy as np
import pytest
import torch

import dw_kernel_ref as R
import plan_driver
from retto_amd import _lib
from test_cls_kernel_checks_cpu import excess, refusal

# mutant -> (how at least one case refuses it, the largest err / bound over the refusing cases is at least this)
MUTANT_FLOOR = {
    "tap_dropped_strip_end": ("bound", 5e5), "taps_transposed": ("bound", 2e6), "stride_swapped": ("bound", 3e6),
    "row_below_next_image": ("bound", 1e6), "col_right_wraps": ("bound", 3e6), "bias_after_act": ("bound", 6e5),
    "lab_before_act": ("bound", 3e5), "pad_passthrough": ("pad", 0), "last_strip_unwritten": ("nan", 0), "pool_row_major": ("bound", 5e5),
    "pool_foreign_block": ("nan", 0), "mean_div_max": ("bound", 5e5), "pool_unremapped": ("canary", 0), "scale_prev_image": ("bound", 2e2),
    "strips_r4": ("nan", 0), "se_fc_strip_r4": ("bound", 3e3),
    "hsig_slope_02": ("bound", 1e2), "row_table_equal_images": ("bound", 2e1), "scale_twice": ("bound", 5e5),
}
# instances of dwconv()'s switch that no case reaches: the 32-channel-slab forms of layers narrower than the networks' wide blocks
# (the classifier's series and the thin blocks' unfused fallback run some of them, under tests/test_gpu_cls_kernels.py and
# tests/test_gpu_rec_kernels.py), and the pooled (2, 1) form on 2-row strips (rec s6.0 always lands on 6 rows: 3-row strips)
UNREACHED = [
    "rows<3,2,2,1,0,8>", "rows<3,2,2,1,1,8>", "rows<3,2,2,2,1,8>", "rows<3,3,1,1,0,8>", "rows<3,3,1,1,1,8>", "rows<3,3,1,2,0,8>",
    "rows<3,3,1,2,1,8>", "rows<3,3,2,1,0,8>", "rows<3,3,2,1,1,8>", "rows<3,3,2,2,1,8>", "rows<3,4,1,1,1,8>", "rows<3,4,1,2,0,8>",
    "rows<3,4,1,2,1,8>", "rows<5,2,2,1,0,8>", "rows<5,2,2,1,1,16>", "rows<5,2,2,1,1,8>", "rows<5,2,2,2,0,8>", "rows<5,2,2,2,1,8>",
    "rows<5,3,1,1,0,8>", "rows<5,3,1,1,1,8>", "rows<5,3,1,2,0,8>", "rows<5,3,1,2,1,8>", "rows<5,3,2,1,0,8>", "rows<5,3,2,1,1,8>",
    "rows<5,4,1,1,0,8>", "rows<5,4,1,1,1,8>", "rows<5,4,1,2,0,8>", "rows<5,4,1,2,1,8>",
]
# what the three networks launch under the default switches, and the row instances RT_DW_SWEEP=0 adds
REACHED_DEFAULT = ["rows<3,4,1,1,0,8>", "rows<3,3,2,2,0,8>", "rows<3,2,2,2,0,8>", "rows<5,4,1,1,0,16>", "rows<5,3,1,1,0,16>",
                   "rows<5,4,1,1,1,16>", "rows<5,3,1,1,1,16>", "rows<5,2,2,2,0,16>", "rows<5,2,2,2,1,16>", "rows<5,3,2,2,0,8>",
                   "rows<5,3,2,2,1,8>", "sweep 1", "sweep 2", "sweep 3", "sweep 4", "sweep 5", "sweep 6"]
REACHED_SWEEP_OFF = ["rows<3,4,1,1,0,16>", "rows<3,4,1,2,0,16>", "rows<5,3,2,1,0,16>", "rows<5,3,2,1,1,16>", "rows<5,2,2,1,0,16>"]
KERNEL = {"rows32": R.ROWS32, "rows64": R.ROWS64, "sweep": R.SWEEP}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return plan_driver.build(tmp_path_factory)


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
        assert (o.bound[arith] > 0).all()
        # every word is either checked against the reference, or must be +0, or must keep the canary: check() does all three
        assert ((b == R.CANARY) | o.mask).all()
    print("FIG %s float32 worst err/bound=%.3g" % (case_id, fig["worst"]))


def _dw_answer(plan):
    names = {v: k for k, v in KERNEL.items()}
    return "%s %d %d %d %d %d %d %d" % (names[plan[0]], plan[1] if plan[0] == R.SWEEP else 0, *plan[2:])


def test_the_case_table_against_the_plan(driver):
    """every depthwise case's plan (instance, strip layout, grid) is nn::dw_plan's; the cases reach every instance on the list and
    leave exactly UNREACHED"""
    cases = [R.case(i) for i in R.DW_IDS]
    q = ["dw %d %d %d %d %d %d %d %d" % (4 if c.form else 0, c.K, c.sh, c.sw, c.Cp, c.maxHo, c.maxWo, c.pooled) for c in cases]
    got = plan_driver.run(driver, q)
    bad = ["%s: plan %s, the case says %s" % (c.name, g, _dw_answer(c.plan)) for c, g in zip(cases, got) if g != _dw_answer(c.plan)]
    assert not bad, "\n".join(bad)
    lib, plan = _lib.load(), (C.c_int * 8)()       # the library's host-only entry gives the same answer (it is what the GPU test asserts from)
    for c in cases:
        assert lib.rt_debug_dw_plan(c.K, c.sh, c.sw, c.Cp, c.maxHo, c.maxWo, int(c.pooled), c.form, plan) == 0 and tuple(plan) == c.plan, c.name
    reached = {c.instance for c in cases}
    assert set(REACHED_DEFAULT) <= {c.instance for c in cases if c.form}
    assert set(REACHED_SWEEP_OFF) <= {c.instance for c in cases if not c.form}
    assert len(R.all_instances()) == 50 and reached <= R.all_instances()
    assert sorted(R.all_instances() - reached) == sorted(UNREACHED)
    assert reached == set(REACHED_DEFAULT) | set(REACHED_SWEEP_OFF)
    # the XCD remap: for each slab width, pooled and not, a batch that takes it beside one that does not
    for lanes in (8, 16):
        for pooled in (0, 1):
            took = {c.remap for c in cases if c.plan[0] != R.SWEEP and c.plan[3] == lanes and c.pooled == pooled}
            assert took == {True, False}, (lanes, pooled, took)
    # shapes: a 1-pixel-wide and a 1-row image, widths off the 4-pixel strip, a partial last row strip, pooled images of one and of several blocks
    for c in cases:
        assert any(w == 1 for _, w in c.outs) and any(h == 1 for h, _ in c.outs) and any(w % 4 for _, w in c.outs)
        assert any(h % c.plan[2] for h, _ in c.outs) and any(h < c.plan[2] for h, _ in c.outs)
        assert c.x.size <= 500000 and (c.Cp == c.C or np.abs(c.x[:, c.C:]).min() > 0)
        if c.pooled:
            nblk = [R.strip_blocks(h, w, c.plan[2], c.plan[4])[1] for h, w in c.outs]
            assert min(nblk) == 1 and 1 < max(nblk) <= c.plan[5] and min(nblk) < c.plan[5]   # (a slot some image does not own)
    # every pooled launch on 3-row strips of a 6-row map holds an image whose block count depends on R being 3 (strips_r4)
    for c in cases:
        if c.pooled and c.maxHo == 6:
            assert c.plan[2] == 3
            nb = lambda h, w, r: R.strip_blocks(h, w, r, c.plan[4])[1]   # noqa: E731
            assert any(nb(h, w, 4) < nb(h, w, 3) <= c.plan[5] for h, w in c.outs), c.name
    for a, b in R.TWINS:
        ca, cb = R.case(a), R.case(b)
        assert ca.form == 1 and cb.form == 0 and ca.plan[0] == R.SWEEP and cb.plan[0] != R.SWEEP
        assert np.array_equal(ca.x, cb.x) and np.array_equal(R.case(a).x, ca.x)


def _lc_q(c):
    return "lc 3 %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d 2 1 1" % (
        4 if c.form else 0, c.K, c.sh, c.sw, c.Cp, c.cin, c.cout, (c.cout + 15) // 16 * 16, c.act, 1 if c.lab else 0, int(c.se), c.maxHo,
        c.maxWo, c.rows, c.min_pix)


def _gemm_q(Cp, M, cin, cout, se, n_img=5):
    return "plan 0 1 0 0 256 %d %d %d %d %d %d 0 0 0 %d 2 2 1 %d %d" % (Cp, M, cin, cout, (cout + 15) // 16 * 16, R.chan_pitch(cout), se, n_img, Cp)


def test_the_block_cases_against_the_plan(driver):
    """the 13 wide block shapes, each unfused; squeeze-excite folded exactly where the case says so, on the GEMM form its name
    carries; FOLD_M is where gemm_plan() first takes each folded form (found here by scanning the plan)"""
    from retto_amd import synth
    wide = {(k, cin, cout, sh, sw, bool(se)) for blocks in (synth.DET_BLOCKS, synth.REC_BLOCKS) for _, k, cin, cout, sh, sw, se in blocks
            if cin >= 96}
    assert len(wide) == 13
    cases = [R.case(i) for i in R.BLOCK_IDS]
    assert {(c.K, c.cin, c.cout, c.sh, c.sw, c.se) for c in cases} == wide
    got = plan_driver.run(driver, [_lc_q(c) for c in cases])
    for c, g in zip(cases, got):
        f = g.split()
        assert f[0] == "unfused", (c.name, g)
        assert int(f[1]) == (128 if c.scaled == "fold" else 0), (c.name, g)
        assert " ".join(f[2:]) == _dw_answer(c.plan), (c.name, g)
        assert c.se == (c.scaled is not None)
    # the folded forms: the smallest M at which the plan takes each
    for Cp, cin, cout, form in ((192, 192, 384, "wide_128x128"), (384, 384, 384, "wide_128x128"), (256, 240, 480, "wide_128x128"),
                                (480, 480, 480, "wide_128x128"), (256, 240, 480, "wide_128x240"), (480, 480, 480, "wide_128x240")):
        Ms = list(range(1, 40001))
        rows = plan_driver.run(driver, ["se_rows 0 1 0 %d %d %d %d %d 2 128" % (Cp, M, cin, cout, (cout + 15) // 16 * 16) for M in Ms])
        plans = plan_driver.run(driver, [_gemm_q(Cp, M, cin, cout, 1) for M in Ms])
        first = next(M for M, r, p in zip(Ms, rows, plans) if r == "128" and p.split()[0] == form and p.split()[4] == "1")
        assert first == R.FOLD_M[form], (cin, cout, form, first)
        assert rows[first - 2] == "0" or plans[first - 2].split()[0] != form
    for c in cases:
        if c.scaled == "fold":
            form = "wide_128x240" if "fold240" in c.name else "wide_128x128"
            assert 0 <= c.rows - R.FOLD_M[form] < 6 and c.min_pix >= 128, (c.name, c.rows)
            assert plan_driver.run(driver, [_gemm_q(c.Cp, c.rows, c.cin, c.cout, 1, len(c.imgs))])[0].split()[0] == form
            px = [h * w for h, w in c.outs]
            assert all(128 <= p <= 140 for p in px[:4]) and px[4] > 4096      # a 128-row tile spans two images; one large image
            if c.plan[2] == 3:      # 3-row strips (the rec folds, 6 rows): a line whose block count depends on R being 3
                assert c.maxHo == 6 and any(R.strip_blocks(h, w, 4, c.plan[4])[1] < R.strip_blocks(h, w, 3, c.plan[4])[1] for h, w in c.outs), c.name
        if "minpix" in c.name:
            assert c.rows >= R.FOLD_M["wide_128x128"] and c.min_pix < 128 and c.scaled == "place"
    # the 3-int table form is out of reach of a test of seconds
    assert plan_driver.run(driver, ["se_rows 0 1 0 480 131071 480 480 480 2 128", "se_rows 0 1 0 480 131072 480 480 480 2 128"]) == ["128", "256"]


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


def test_every_listed_mutant_has_a_floor():
    assert set(MUTANT_FLOOR) == set(R.MUTANTS) and len(R.MUTANTS) >= 15
    assert all(v and set(v) <= set(R.CASE_IDS) for v in R.MUTANTS.values())


def test_a_write_outside_the_output_is_refused():
    half = np.float32(0.5).view(np.uint32)
    c = R.case("det-s6.1-h10-pool")
    good = c.buffers(torch.float32)
    po = c.reference()[1]
    foreign = int(np.flatnonzero(~po.mask[:-64].any(1))[0])          # a partial-sum slot an image does not own
    pout = c.reference()[0].shape[0] - 64
    for k, r, col in ((0, pout, 0), (0, pout + 63, c.Cp - 1), (1, foreign, 5), (1, po.shape[0] - 1, 0), (2, len(c.imgs), 0)):
        bad = [b.copy() for b in good]
        bad[k][r, col] = half
        assert refusal(c, bad) == "canary", (k, r, col)
    c = R.case("rec-s5.1-h12")                                       # pad channels 240 .. 256: +0, not -0
    bad = [b.copy() for b in c.buffers(torch.float32)]
    bad[0][3, 250] = np.float32(-0.0).view(np.uint32)
    assert refusal(c, bad) == "pad"
    c = R.case("blk-rec-s5.0")                                       # the block output's columns 240 .. 256 keep the canary
    bad = [b.copy() for b in c.buffers(torch.float32)]
    bad[0][0, 250] = half
    assert refusal(c, bad) == "canary"


def test_the_references_are_the_plain_operations():
    """the depthwise conv against direct loops at a few pixels of a strided ragged batch, the partial sums against a walk over
    the strips, and every squeeze-excite case reaches both clamps and the linear part of the hard-sigmoid"""
    rng = np.random.default_rng(0)
    imgs = [(5, 4), (3, 7)]
    x, w = rng.uniform(-1, 1, (20 + 21, 3)), rng.uniform(-1, 1, (5, 5, 3))
    got = R.dwconv(torch.from_numpy(x), imgs, torch.from_numpy(w), 5, 2, 1).numpy()
    assert got.shape == (3 * 4 + 2 * 7, 3)
    for img, off, ooff, (H, W), pts in ((0, 0, 0, (5, 4), ((0, 0), (2, 3), (1, 2))), (1, 20, 12, (3, 7), ((0, 0), (1, 6)))):
        for oy, ox in pts:
            want = np.zeros(3)
            for dy in range(5):
                for dx in range(5):
                    sy, sx = 2 * oy + dy - 2, ox + dx - 2
                    if 0 <= sy < H and 0 <= sx < W:
                        want += w[dy, dx] * x[off + sy * W + sx]
            assert np.allclose(got[ooff + oy * W + ox], want, rtol=0, atol=1e-13)
    c = R.case("det-s6.0-h5-pool")
    y, po, mo = c.reference()
    _, _, Rr, _, spb, chunks, _, _ = c.plan
    oo = R.offsets(c.outs)
    for i, (Ho, Wo) in enumerate(c.outs):
        sy = (Ho + Rr - 1) // Rr
        want = np.zeros((chunks, c.Cp))
        for oy in range(Ho):
            for ox in range(Wo):
                want[((ox // 4) * sy + oy // Rr) // spb] += y.v[oo[i] + oy * Wo + ox]
        rows = po.mask[i * chunks:(i + 1) * chunks].any(1)
        assert np.allclose(po.v[i * chunks:(i + 1) * chunks][rows], want[rows], rtol=0, atol=1e-12) and not want[~rows].any()
        assert np.allclose(mo.v[i], y.v[oo[i]:oo[i + 1]].mean(0), rtol=0, atol=1e-14)
    for cid in R.BLOCK_IDS:
        cc = R.case(cid)
        if cc.se and cc.rows < 20000:
            cc.reference()
            assert min(cc.regions) > 0

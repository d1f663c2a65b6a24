"""The checks of tests/ctc_head_ref.py bite, and a right head can pass them: for every case tests/test_gpu_ctc_head.py runs on the
GPU the float32 stand-in passes check(), and each of the seven numpy mutants of the head is refused by exactly the cases (and, on
the tie case, the planted sets) written down here -- so a case edited later cannot silently stop biting."""
import numpy as np
import pytest

import ctc_head_ref as R

TIES = "ties-N400"
MULTI_TILE = [i for i in R.CASE_IDS if R.case(i).N > R.TILE]


def _ids(pred):
    return [i for i in R.CASE_IDS if pred(R.case(i))]


# mutant -> the cases that refuse it
REFUSED_BY = {
    # every planted set, and the all-equal rows (expected index 0)
    "tie_to_higher": [TIES] + ["equal-N%d" % n for n in R.EQUAL_COUNTS],
    "tie_by_quarter": [TIES],
    # the sets that span 128-column tiles; all-equal rows of more than one tile
    "tiles_merged_with_ge": [TIES, "equal-N129", "equal-N6625"],
    # wherever there are pad columns: a 0 beside all-negative logits wins (idx >= N), beside others it joins the sum; the
    # large-logit case asks nothing of prob beyond (0, 1]
    "pad_columns_take_part": _ids(lambda c: c.N % 16 != 0 and c.prob_rule != "finite"),
    # one tile: nothing is left (idx out of range); more: the last tile's share of the sum is missing, or the argmax itself
    "last_tile_dropped": list(R.CASE_IDS),
    "sum_of_winning_tile_only": MULTI_TILE,
    # (all-equal rows have equal tile maxima: nothing to rescale)
    "sum_not_rescaled": [i for i in MULTI_TILE if not i.startswith("equal")],
}
ALL_SETS = list(R.TIE_SETS)
# mutant -> the planted sets of the tie case whose rows refuse it
SETS_REFUSING = {
    "tie_to_higher": ALL_SETS,
    # the lower column in the higher lane quarter: 28 % 16 // 4 = 3 against 32 -> 0, 300 -> 3 against 390 -> 1
    "tie_by_quarter": [(28, 32), (300, 390)],
    # the sets whose members lie in different 128-column tiles ((230, 250) spans 240-column tiles only)
    "tiles_merged_with_ge": [(70, 170), (110, 140), (300, 390), (150, 399), (0, 200), (5, 133, 261, 389)],
    "pad_columns_take_part": [],          # 400 = 25 * 16: no pad column
    # the planted rows' other tiles hold exp(-3) and less of the sum each, far above TOL_PROB
    "last_tile_dropped": ALL_SETS,
    "sum_of_winning_tile_only": ALL_SETS,
    # (a set with a member in every tile has four equal tile maxima)
    "sum_not_rescaled": [s for s in ALL_SETS if s != (5, 133, 261, 389)],
}


def _rows_refused(c, idx, prob):
    bad = R.violations(c, idx, prob)
    return np.unique(np.concatenate(list(bad.values()))) if bad else np.zeros(0, np.int64)


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_float32_stand_in_passes(case_id):
    c = R.case(case_id)
    assert c.decisive().mean() >= R.MIN_DECISIVE
    R.check(c, *c.standin())


@pytest.mark.parametrize("name", R.MUTANTS)
def test_mutant_is_refused_by_the_cases_it_names(name):
    assert set(REFUSED_BY) == set(SETS_REFUSING) == set(R.MUTANTS)
    refused = []
    for i in R.CASE_IDS:
        c = R.case(i)
        idx, prob = c.mutant(name)
        rows = _rows_refused(c, idx, prob)
        if len(rows):
            refused.append(i)
            with pytest.raises(AssertionError):
                R.check(c, idx, prob)
        if i == TIES:
            assert R.planted_sets_hit(c, rows) == SETS_REFUSING[name]
    assert refused == [i for i in R.CASE_IDS if i in REFUSED_BY[name]]
    assert refused


def test_the_named_cases_bite():
    """the pairs the cases were built for"""
    assert (28, 32) in SETS_REFUSING["tie_by_quarter"]
    assert {(110, 140), (300, 390), (150, 399), (0, 200), (5, 133, 261, 389)} <= set(SETS_REFUSING["tiles_merged_with_ge"])
    pad = set(REFUSED_BY["pad_columns_take_part"])
    assert {"equal-N%d" % n for n in R.EQUAL_COUNTS} | {"negative-N%d" % n for n in R.NEGATIVE_COUNTS} <= pad
    for n in R.NEGATIVE_COUNTS:   # beside all-negative logits the pad column wins outright
        c = R.case("negative-N%d" % n)
        assert (c.ref()["logits"] < -10).all()
        idx, _ = c.mutant("pad_columns_take_part")
        assert (idx >= c.N).all()


def test_planted_ties_are_what_they_claim():
    """in fp64 a planted row's maximum is shared by exactly the planted classes and beats the next distinct value by more than
    2 B; the sets are pairwise disjoint, their columns bit-equal, and they sit where the kernels' mapping says"""
    c = R.case(TIES)
    r = c.ref()
    flat = [k for s in R.TIE_SETS for k in s]
    assert len(flat) == len(set(flat)) and max(flat) == R.TIE_N - 1
    all_rows = [row for _, rows in c.planted for row in rows]
    assert len(all_rows) == len(set(all_rows)) == R.TIE_ROWS_PER_SET * len(R.TIE_SETS)
    for s, rows in c.planted:
        assert len(rows) == R.TIE_ROWS_PER_SET
        for k in s[1:]:
            assert np.array_equal(c.W[:, k].view(np.uint32), c.W[:, s[0]].view(np.uint32))
            assert c.bias[k].view(np.uint32) == c.bias[s[0]].view(np.uint32)
        for row in rows:
            lg = r["logits"][row]
            assert tuple(np.flatnonzero(lg == lg.max())) == tuple(sorted(s))
            assert lg.max() - lg[lg < lg.max()].max() > 2 * r["bound"][row]
            assert r["top"][row] == min(s)
    rows_used = np.array(all_rows)
    assert len(set(rows_used // 128)) == 3 and len(set(rows_used % 16)) == 16   # every row block, every lane row
    quarter = lambda k: k % 16 // 4     # noqa: E731
    lane = lambda k: (k // 128, quarter(k))   # noqa: E731  (form 0: a lane holds one quarter of every group of its tile)
    assert lane(8) == lane(9) and 8 // 16 == 9 // 16
    assert lane(40) == lane(56) and 56 // 16 == 40 // 16 + 1
    assert (quarter(64), quarter(68)) == (0, 1) and 64 // 16 == 68 // 16
    assert (quarter(80), quarter(88)) == (0, 2) and 80 // 16 == 88 // 16
    assert (quarter(28), quarter(32)) == (3, 0)
    assert 20 // 128 == 100 // 128 and (20 % 128 // 64, 100 % 128 // 64) == (0, 1)      # two waves of a 128 x 128 tile
    assert 70 // 240 == 170 // 240 and (70 % 240 // 80, 170 % 240 // 80) == (0, 2)      # two waves of a 256 x 240 tile
    assert (110 // 128, 140 // 128) == (0, 1) and 110 // 240 == 140 // 240
    assert (230 // 240, 250 // 240) == (0, 1) and 230 // 128 == 250 // 128
    assert 300 // 128 == 2 and 390 // 128 == 3 and R.TIE_N - 3 * 128 == 16                # into the last, 16-column tile
    assert [k // 128 for k in (5, 133, 261, 389)] == [0, 1, 2, 3] and len({k % 128 for k in (5, 133, 261, 389)}) == 1


def test_measured_standin_is_reproduced():
    worst = max(R.deviation(R.case(i), R.case(i).standin()[1]) for i in R.CLASS_COUNT_IDS)
    assert abs(worst / R.MEASURED_STANDIN - 1) <= 0.1, worst
    assert R.TOL_PROB == min(4 * R.MEASURED_STANDIN, 1.2e-5)


def test_reference_and_grid():
    """reference() returns what it says, and the cases are the grid the suite promises"""
    c = R.case("classes-N17")
    logits, bound, top, prob = R.reference(c.A, c.W, c.bias)
    assert logits.dtype == np.float64 and logits.shape == (300, 17) and bound.shape == top.shape == prob.shape == (300,)
    a, w = c.A.astype(np.float64), c.W.astype(np.float64)
    assert np.array_equal(bound, (R.U * 128 * (np.abs(a) @ np.abs(w) + np.abs(c.bias.astype(np.float64)))).max(1))
    p = np.exp(logits - logits.max(1, keepdims=True))
    assert np.array_equal(top, p.argmax(1)) and np.allclose(prob, (p / p.sum(1, keepdims=True)).max(1), rtol=1e-14)
    shapes = {(R.case(i).M, R.case(i).N) for i in R.CASE_IDS}
    assert {(300, n) for n in R.CLASS_COUNTS} | {(m, n) for n in R.ROW_COUNT_CLASSES for m in R.ROW_COUNTS} <= shapes
    assert all(R.case(i).A.shape[1] == R.K == 120 for i in R.CASE_IDS)
    for n in R.EQUAL_COUNTS:
        e = R.case("equal-N%d" % n)
        assert not e.A.any() and len(set(e.bias.tolist())) == 1 and (e.ref()["top"] == 0).all()
    big = R.case("large-N97")
    assert np.array_equal(big.A, R.case("classes-N97").A * np.float32(40)) and np.array_equal(big.W, R.case("classes-N97").W)


def test_check_refuses_each_rule_on_its_own():
    c = R.case("classes-N129")
    idx, prob = c.standin()
    for bad_idx in (-1, 129, R.NO_CLASS):
        i = idx.copy()
        i[7] = bad_idx
        with pytest.raises(AssertionError):
            R.check(c, i, prob)
    i = idx.copy()
    i[299] = (i[299] + 1) % 129
    with pytest.raises(AssertionError):
        R.check(c, i, prob)
    for f in (1 + 2 * R.TOL_PROB, 1 - 2 * R.TOL_PROB, np.nan):
        p = prob.copy()
        p[150] *= np.float32(f)
        with pytest.raises(AssertionError):
            R.check(c, idx, p)
    e = R.case("equal-N97")
    idx, prob = e.standin()
    R.check(e, idx, prob)
    p = prob.copy()
    p[3] = np.nextafter(p[3], np.float32(1))
    R.check(e, idx, p)                           # 1 ulp
    p[3] = prob[3] * np.float32(1 + 1e-6)        # 8 ulp
    with pytest.raises(AssertionError):
        R.check(e, idx, p)

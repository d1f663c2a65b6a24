"""Rec flip (retto_amd/csrc/rec_flip.h) on the GPU: view 1 of a line against view 0 of its host-rotated copy byte for byte, the
views' scores against the numpy restatement of rec_flip_ref bit for bit, the choice against rt_rec_flip_choose, the selection
against the taken view's rows (fp32, f16, under rec windows), both outcomes as the CPU oracle predicts them, the pipeline
(rt_run_regions with word boxes and candidates) against the debug entry, the threshold, the entry points, the no-op paths and
the setter's guards.

The fixture: six crops of seeded block noise (blocks a sixth of the crop's height, so that the thumbnail keeps their contrast:
plain pixel noise averages to grey at these sizes and the two views' scores then differ by less than 1e-3), sizes 48x320,
30x200, 17x333, 48x96, 64x500 and 9x40, at max_wh_ratio 9.0 (W = 432, T = 54).  The seed was picked with the CPU oracle
(oracle/nets_torch.py over oracle resize_norm_image): at seed 9 every line's two views differ by at least 1e-2 in their oracle
score -- 50 times REC_ATOL = 2e-4 of test_gpu_parity.py, so GPU rounding cannot turn a choice -- and both outcomes occur.  The
oracle's (kept tokens, score) per line, view 0 then view 1, and the view it takes:
    48x320   (14, 0.24543197)  (20, 0.13487515)   view 0
    30x200   (21, 0.03840549)  (26, 0.02347927)   view 0
    17x333   (30, 0.11914799)  (37, 0.13245358)   view 1
    48x96    (10, 0.35165614)  ( 9, 0.22073983)   view 0
    64x500   (22, 0.11848068)  (18, 0.14306115)   view 1
    9x40     ( 5, 0.02487397)  ( 5, 0.01227789)   view 0
"""
import ctypes as C
import math

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, synth

import rec_flip_ref as FR

pytestmark = pytest.mark.gpu

SIZES = [(48, 320), (30, 200), (17, 333), (48, 96), (64, 500), (9, 40)]
SEED, RATIO, W_WANT, T_WANT = 9, 9.0, 432, 54
ORACLE_SCORES = [((14, 0.24543197), (20, 0.13487515)), ((21, 0.03840549), (26, 0.02347927)), ((30, 0.11914799), (37, 0.13245358)),
                 ((10, 0.35165614), (9, 0.22073983)), ((22, 0.11848068), (18, 0.14306115)), ((5, 0.02487397), (5, 0.01227789))]
ORACLE_TAKEN = [0, 0, 1, 0, 1, 0]
N = len(SIZES)


def _block_noise(h, w, rng, b=None):
    b = max(1, (h + 5) // 6) if b is None else b
    g = rng.integers(0, 256, ((h + b - 1) // b, (w + b - 1) // b, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((b, b, 1), np.uint8))[:h, :w])


def _crops():
    rng = np.random.default_rng(SEED)
    return [_block_noise(h, w, rng) for h, w in SIZES]


def _twelve():
    """the six crops, then their host-rotated copies"""
    c = _crops()
    return c + [FR.rotate180(x) for x in c]


BOTH = [1] * N + [0] * N


def _session(**kw):
    return retto_amd.RettoSession(retto_amd.synthetic_session_config(0, **kw))


@pytest.fixture(scope="module")
def s32():
    s = _session(lanes=1)
    yield s
    s.close()


@pytest.fixture(scope="module")
def run32(s32):
    """the twelve lines in ONE debug_rec_flip call on the fp32 session, computed once"""
    return s32.debug_rec_flip(_twelve(), BOTH, RATIO)


def _calls(prof, name):
    return prof.get(name, (0.0, 0))[1]


def _f32(x):
    return np.float32(x).tobytes()


# ---- 1. the view ---------------------------------------------------------------------------------------------------------------
def test_view_1_is_view_0_of_the_rotated_crop(run32):
    out = run32
    assert (out["W"], out["T"]) == (W_WANT, T_WANT) and out["view_idx"].shape == (3 * N, T_WANT)
    assert out["view1"] == {j: 2 * N + j for j in range(N)}
    for j in range(N):
        v1, r0 = out["view1"][j], j + N
        assert out["view_idx"][v1].tobytes() == out["view_idx"][r0].tobytes(), j
        assert out["view_prob"][v1].tobytes() == out["view_prob"][r0].tobytes(), j
        assert out["view_idx"][j].tobytes() != out["view_idx"][v1].tobytes() or out["view_prob"][j].tobytes() != out["view_prob"][v1].tobytes(), j
    assert np.isfinite(out["view_prob"]).all()


# ---- 2. the scores and the choice ----------------------------------------------------------------------------------------------
def test_scores_and_choice(run32):
    out = run32
    lib = _lib.load()
    for v in range(3 * N):
        n, s = FR.score(out["view_idx"][v], out["view_prob"][v])
        print("view %2d: %2d tokens, score %r" % (v, n, float(s)))
        assert int(out["view_ntok"][v]) == n, v
        assert _f32(out["view_score"][v]) == _f32(s) or (np.isnan(s) and np.isnan(out["view_score"][v])), v
    for j in range(N):
        v1 = out["view1"][j]
        want = lib.rt_rec_flip_choose(int(out["view_ntok"][j]), C.c_float(float(out["view_score"][j])),
                                      int(out["view_ntok"][v1]), C.c_float(float(out["view_score"][v1])))
        assert int(out["taken"][j]) == want == FR.choose(out["view_ntok"][j], out["view_score"][j], out["view_ntok"][v1], out["view_score"][v1]), j
    assert (out["taken"][N:] == 0).all()


# ---- 3. the selection ----------------------------------------------------------------------------------------------------------
def _assert_selection(out):
    """the lines' final idx / prob / z5 rows are the taken view's rows of the same pass; a line read one way keeps its view 0;
    and a line that took view 1 ends with the rows of its host-rotated copy, line j + N of the same pass"""
    n = len(out["taken"])
    assert n == 2 * N and out["view_z5"].shape == (3 * N, T_WANT, 120)
    for j in range(n):
        both = j in out["view1"]
        assert both == bool(BOTH[j]) and (both or out["taken"][j] == 0)
        src = out["view1"][j] if both and out["taken"][j] else j
        for a in ("idx", "prob", "z5"):
            assert out[a][j].tobytes() == out["view_" + a][src].tobytes(), (j, a)
            if both and out["taken"][j]:
                assert out[a][j].tobytes() == out[a][j + N].tobytes(), (j, a)
                assert out[a][j].tobytes() != out["view_" + a][j].tobytes(), (j, a)
    assert np.isfinite(out["z5"]).all() and np.isfinite(out["view_z5"]).all()
    assert 0 < int(out["taken"][:N].sum()) < N   # both kinds of copy ran


def test_selection(run32, s32):
    _assert_selection(run32)
    # no line read both ways: the group's former path; the views are the lines and nothing is taken
    plain = s32.debug_rec_flip(_twelve(), [0] * (2 * N), RATIO)
    assert plain["view1"] == {} and (plain["taken"] == 0).all() and plain["view_idx"].shape == (2 * N, T_WANT)
    for a in ("idx", "prob", "z5"):
        assert plain[a].tobytes() == plain["view_" + a].tobytes(), a


def test_selection_f16():
    s = _session(lanes=1, dtype="f16")
    try:
        lines = _twelve()
        _assert_selection(s.debug_rec_flip(lines, BOTH, RATIO))
    finally:
        s.close()


def test_selection_under_windows(s32):
    lines = _twelve()
    s32.set_rec_windows(128, 32)   # every line is 432 wide: several units each
    try:
        assert len(retto_amd.rec_window_plan(W_WANT, 128, 32)["origins"]) > 1
        s32.profile_enable()
        out = s32.debug_rec_flip(lines, BOTH, RATIO)
        prof = s32.profile_get()
        assert _calls(prof, "rec_window_cut") == 1 and _calls(prof, "rec_window_stitch") == 1 and _calls(prof, "net/rec") == 1
        assert _calls(prof, "rec_flip_rotate") == 1 and _calls(prof, "rec_flip_select") == 1
        _assert_selection(out)
    finally:
        s32.set_rec_windows(0)


# ---- 4. both outcomes occur, as the oracle predicts ----------------------------------------------------------------------------
def test_outcomes_are_the_oracles(run32):
    out = run32
    for (a, b), t in zip(ORACLE_SCORES, ORACLE_TAKEN):
        assert abs(a[1] - b[1]) >= 1e-2 and FR.choose(a[0], a[1], b[0], b[1]) == t
    assert sum(ORACLE_TAKEN) >= 2 and N - sum(ORACLE_TAKEN) >= 2
    for j in range(N):
        print("line %d: GPU (%d, %.8f) (%d, %.8f), oracle %r" % (j, out["view_ntok"][j], out["view_score"][j], out["view_ntok"][out["view1"][j]],
                                                                  out["view_score"][out["view1"][j]], ORACLE_SCORES[j]))
    assert out["taken"][:N].tolist() == ORACLE_TAKEN


# ---- the pages of tests 5 - 8: regions on noise pages ----------------------------------------------------------------------------
def _rect(x0, y0, w, h):
    return [x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h]


def _turned(q):
    """the same region, its corners named from the opposite one: the crop comes out upside down"""
    return q[4:] + q[:4]


# Shapes.  The fp32 GEMM behind the rec network picks its kernel by the row count of the pass (gemm_plan.cpp: thresholds at 8192,
# 16384, 65536 and 131072 rows), and two kernels round differently in the low bits.  A flip call runs more rows than the flip-off
# call, so "equals the flip-off call bit for bit" can only hold where both passes stay on the same kernels.  Here every region
# is at most 320 : 48, so all six lines are 320 wide: the flip-off pass has 6 lines, the flip passes 9 and 12 views, which is
# 23 040 .. 46 080 rows at the first rec stage and in proportion at every later one -- inside one range of every threshold.
# With one width, ONE debug_rec_flip call over all the crops is also the pipeline's rec group line for line.
REGION_PAGES = [((100, 260), [_rect(10, 8, 200, 32), _turned(_rect(20, 56, 120, 30))]),
                ((90, 240), [_rect(16, 6, 160, 32), _rect(30, 50, 180, 30)]),
                ((110, 280), [_turned(_rect(8, 10, 240, 40)), _rect(12, 64, 90, 24)])]


def _region_pages(seed):
    pages = []
    for i, ((h, w), _) in enumerate(REGION_PAGES):
        pages.append(_block_noise(h, w, np.random.default_rng(seed + i), 5))
    return pages, [q for _, q in REGION_PAGES]


def _option_session(lanes=1):
    cfg = retto_amd.synthetic_session_config(0, lanes=lanes)
    cfg.rec_processor_config.return_candidates = 2
    cfg.rec_processor_config.return_word_box = True
    return retto_amd.RettoSession(cfg)


def _word_key(w):
    return (w.text, w.kind, w.first_token, w.n_tokens, w.first_col, w.last_col, np.ascontiguousarray(w.box.as_array(), np.float32).tobytes())


def _rec_same(x, y):
    """two rec results bit for bit: tokens, score, text, words, candidates"""
    assert np.array_equal(x.tokens, y.tokens) and x.text == y.text and (_f32(x.score) == _f32(y.score) or (np.isnan(x.score) and np.isnan(y.score)))
    assert (x.words is None) == (y.words is None) and (x.candidates is None) == (y.candidates is None)
    if x.words is not None:
        assert [_word_key(w) for w in x.words] == [_word_key(w) for w in y.words]
    if x.candidates is not None:
        assert np.array_equal(x.token_cols, y.token_cols)
        assert [[(i, t, _f32(p)) for i, t, p in c] for c in x.candidates] == [[(i, t, _f32(p)) for i, t, p in c] for c in y.candidates]


def _front_same(a, b):
    """boxes, det scores, cls labels and cls scores of two results bit for bit"""
    assert len(a.det_result) == len(b.det_result)
    for x, y in zip(a.det_result, b.det_result):
        assert np.array_equal(x.boxes.as_array(), y.boxes.as_array()) and _f32(x.score) == _f32(y.score)
    assert [c.label.label for c in a.cls_result] == [c.label.label for c in b.cls_result]
    assert [_f32(c.label.score) for c in a.cls_result] == [_f32(c.label.score) for c in b.cls_result]


def _page_ratio_and_geometry(s, crops):
    """one page of at most batch_num lines: the batch's max_wh_ratio and per line (W, resized_w), as rec_plan derives them"""
    rc = s.config.rec_processor_config
    rh, rw = int(rc.image_shape[1]), int(rc.image_shape[2])
    assert len(crops) <= int(rc.batch_num)
    ratio = np.float32(rw) / np.float32(rh)
    for c in crops:
        ratio = max(ratio, np.float32(c.shape[1]) / np.float32(c.shape[0]))
    W = s._hd.lib.rt_resize_norm_width(rh, rw, float(ratio))
    return float(ratio), [(W, min(int(math.ceil(float(rh) * float(c.shape[1]) / float(c.shape[0]))), W)) for c in crops]


def _cls_rotated(s, cl):
    return cl.label.label == 180 and np.float32(cl.label.score) >= np.float32(s.config.cls_processor_config.thresh)


# ---- 5. the pipeline -------------------------------------------------------------------------------------------------------------
def _figures(what, j, g, ref):
    """how far a line of a flip call is from the same line of the flip-off call, printed before the bit-for-bit assertion"""
    same_tok = np.array_equal(g.tokens, ref.tokens)
    dp = 0.0
    if same_tok and g.candidates is not None and len(g.tokens):
        dp = max(abs(float(a[0][2]) - float(b[0][2])) for a, b in zip(g.candidates, ref.candidates))
    print("%s line %d: tokens %s, |score - off| = %.3e (%r vs %r), worst |token prob - off| = %.3e"
          % (what, j, "equal" if same_tok else "DIFFER", abs(float(g.score) - float(ref.score)), float(g.score), float(ref.score), dp))


@pytest.fixture(scope="module")
def pipe_runs():
    """the region pages through rt_run_regions with flip off and with set_rec_flip(2.0), word boxes and two candidates on, and
    the call's one rec group through debug_rec_flip, computed once"""
    from oracle import ref_lib as R
    pages, quads = _region_pages(300)
    s = _option_session()
    try:
        off = s.run_regions(pages, quads)
        s.set_rec_flip(2.0)
        assert s.rec_flip == 2.0
        on = s.run_regions(pages, quads)
        dic = s._dictionary()
        crops, geoms, ratios, rotated = [], [], [], []
        for page, q, a in zip(pages, quads, on):
            cs = s.crop_images(page, np.array(q, np.float32))
            rot = [bool(_cls_rotated(s, cl)) for cl in a.cls_result]
            cs = [R.rotate180(c) if r else c for c, r in zip(cs, rot)]
            ratio, geom = _page_ratio_and_geometry(s, cs)
            crops += cs; geoms += geom; ratios.append(ratio); rotated += rot
        assert len(set(ratios)) == 1 and len(set(g[0] for g in geoms)) == 1 and len(crops) == 6   # one width for the call's lines
        dbg = s.debug_rec_flip(crops, [1] * len(crops), ratios[0])   # the call's one rec group, line for line
        T = dbg["T"]
        probs = np.zeros((len(crops), T, len(dic)), np.float32)   # the final rows as rt_ctc_decode takes them: one class a step
        for j in range(len(crops)):
            probs[j, np.arange(T), dbg["idx"][j]] = dbg["prob"][j]
        _idx, _pr, toks, scores = s.ctc_decode(probs)
    finally:
        s.close()
    return {"pages": pages, "quads": quads, "off": off, "on": on, "dic": dic, "geoms": geoms, "rotated": rotated, "dbg": dbg,
            "toks": toks, "scores": scores}


def _lines(r):
    """(j, page, quad, line of the flip call, line of the flip-off call) over the call's lines"""
    j = 0
    for page, q, a, b in zip(r["pages"], r["quads"], r["on"], r["off"]):
        for k, (g, ref) in enumerate(zip(a.rec_result, b.rec_result)):
            yield j, page, q[k], g, ref
            j += 1


def test_pipeline_equals_the_debug_entry(pipe_runs):
    r = pipe_runs
    dbg, dic = r["dbg"], r["dic"]
    T = dbg["T"]
    for a, b in zip(r["on"], r["off"]):
        _front_same(a, b)
        assert all(x.flip is None for x in b.rec_result)
    outcomes = []
    for j, page, quad, g, ref in _lines(r):
        assert g.flip is not None and g.flip.outcome in (1, 2), j
        assert g.flip.outcome == 1 + int(dbg["taken"][j]), j
        v1 = dbg["view1"][j]
        assert _f32(g.flip.score0) == _f32(dbg["view_score"][j]) and _f32(g.flip.score1) == _f32(dbg["view_score"][v1]), j
        assert np.array_equal(g.tokens, r["toks"][j]) and g.text == "".join(dic[int(i)] for i in r["toks"][j]), j
        assert _f32(g.score) == _f32(r["scores"][j]) or (np.isnan(g.score) and np.isnan(r["scores"][j])), j
        outcomes.append(g.flip.outcome)
        # the words: (cls rotated) XOR (view 1 taken) is the line's rot180, whatever the outcome
        rot180 = r["rotated"][j] ^ (g.flip.outcome == 2)
        cols = g.token_cols.tolist()
        want = retto_amd.debug_word_boxes(synth.synth_models(0)[3], g.tokens, cols, T, r["geoms"][j][0], r["geoms"][j][1], quad, rot180,
                                          page.shape[1], page.shape[0], page.shape[1], page.shape[0])
        assert [_word_key(w) for w in g.words] == [_word_key(w) for w in want], j
        assert len(g.candidates) == len(g.tokens) == len(cols)
        for c, t, col in zip(g.candidates, g.tokens, cols):
            assert c[0][0] == int(t) == int(dbg["idx"][j][col]) and _f32(c[0][2]) == _f32(dbg["prob"][j][col]), (j, col)
    print("outcomes:", outcomes)
    assert 1 in outcomes and 2 in outcomes


def test_kept_lines_equal_the_flip_off_call(pipe_runs):
    """A line with outcome 1 equals the flip-off call bit for bit, in tokens, score, text, words and candidates."""
    kept = [(j, g, ref) for j, _page, _quad, g, ref in _lines(pipe_runs) if g.flip.outcome == 1]
    assert kept
    for j, g, ref in kept:
        _figures("kept", j, g, ref)
    for j, g, ref in kept:
        _rec_same(g, ref)


# ---- 6. the threshold ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold_runs():
    """the region pages with flip off and with cls_below = the median classifier score of the flip-off call"""
    pages, quads = _region_pages(300)
    s = _option_session()
    try:
        off = s.run_regions(pages, quads)
        scores = np.array([c.label.score for r in off for c in r.cls_result], np.float32)
        below = np.float32(np.median(scores))
        s.set_rec_flip(float(below))
        s.profile_enable()
        on = s.run_regions(pages, quads)
        prof = s.profile_get()
    finally:
        s.close()
    return {"pages": pages, "quads": quads, "off": off, "on": on, "scores": scores, "below": below, "prof": prof}


def test_threshold_flags_exactly_the_lines_below_it(threshold_runs):
    r = threshold_runs
    flagged = 0
    for a, b in zip(r["on"], r["off"]):
        _front_same(a, b)
        for g, cl in zip(a.rec_result, a.cls_result):
            if np.float32(cl.label.score) < r["below"]:
                assert g.flip is not None and g.flip.outcome in (1, 2)
                flagged += 1
            else:
                assert g.flip is None
    print("cls scores", r["scores"].tolist(), "cls_below", float(r["below"]), "flagged", flagged)
    assert 0 < flagged < len(r["scores"])
    assert _calls(r["prof"], "rec_flip_rotate") == 1 and _calls(r["prof"], "rec_flip_select") == 1


def test_unflagged_lines_equal_the_flip_off_call(threshold_runs):
    """The lines at or above the threshold report 0 and are bit-identical to the flip-off call."""
    rest = [(j, g, ref) for j, _page, _quad, g, ref in _lines(threshold_runs) if g.flip is None]
    assert rest
    for j, g, ref in rest:
        _figures("unflagged", j, g, ref)
    for j, g, ref in rest:
        _rec_same(g, ref)


# ---- 7. entry points and no-op paths ---------------------------------------------------------------------------------------------
def test_entry_points_and_no_op_paths():
    from oracle import ref_lib as R
    from retto_amd import workload
    s = _session(lanes=2)
    try:
        planted = [workload.planted_page(320, 480, 4, seed=31, ratio_range=(3.0, 10.0)),
                   workload.planted_page(352, 640, 5, seed=32, ratio_range=(3.0, 10.0))]
        pages = [p for p, _ in planted]
        maps = [workload.planted_map(*R.resize_either_dims(*p.shape[:2]), p.shape[0], p.shape[1], rects) for p, rects in planted]
        hs, ws = [p.shape[0] for p in pages], [p.shape[1] for p in pages]
        s.profile_enable()
        off = s.run_batch(pages, det_map_override=maps)
        prof = s.profile_get()
        assert _calls(prof, "rec_flip_rotate") == 0 and _calls(prof, "rec_flip_select") == 0 and _calls(prof, "rec_flip_score") == 0
        assert sum(len(r.rec_result) for r in off) >= 4 and all(x.flip is None for r in off for x in r.rec_result)
        s.set_rec_flip(1e-30)   # on, and no classifier score is below it: no line is flagged
        s.profile_enable()
        none = s.run_batch(pages, det_map_override=maps)
        prof = s.profile_get()
        assert _calls(prof, "rec_flip_rotate") == 0 and _calls(prof, "rec_flip_select") == 0 and _calls(prof, "rec_flip_score") == 0
        for a, b in zip(none, off):
            _front_same(a, b)
            for x, y in zip(a.rec_result, b.rec_result):
                assert x.flip is None
                _rec_same(x, y)
        s.set_rec_flip(2.0)
        s.profile_enable()
        ran = s.run_batch(pages, det_map_override=maps)
        prof = s.profile_get()
        assert _calls(prof, "rec_flip_rotate") == _calls(prof, "rec_flip_select") == 2   # one group on each lane
        got = s.wait_batch(s.submit_batch_raw(pages, hs, ws, det_map_override=maps))
        for a, b, c in zip(got, ran, off):
            _front_same(a, b)
            _front_same(a, c)
            for x, y in zip(a.rec_result, b.rec_result):
                assert x.flip is not None and y.flip is not None and x.flip.outcome == y.flip.outcome in (1, 2)
                assert _f32(x.flip.score0) == _f32(y.flip.score0) and _f32(x.flip.score1) == _f32(y.flip.score1)
                _rec_same(x, y)
    finally:
        s.close()


# ---- 8. the setter ---------------------------------------------------------------------------------------------------------------
def test_setter_guards():
    from oracle import ref_lib as R
    from retto_amd import workload
    s = _session(lanes=2)
    try:
        for bad in (float("nan"), -1.0, float("inf")):
            with pytest.raises(retto_amd.InvalidArgument) as e:
                s.set_rec_flip(bad)
            assert "cls_below" in str(e.value) and "rt_set_rec_flip" in str(e.value), str(e.value)
        assert s.rec_flip == 0.0
        s.set_rec_flip(0.95)
        assert s.rec_flip == np.float32(0.95)
        page, rects = workload.planted_page(320, 480, 4, seed=31, ratio_range=(3.0, 10.0))
        pmap = workload.planted_map(*R.resize_either_dims(320, 480), 320, 480, rects)
        ticket = s.submit_batch_raw([page, page], [320, 320], [480, 480], det_map_override=[pmap, pmap])
        with pytest.raises(retto_amd.InvalidArgument) as e:   # refused while the ticket is in flight
            s.set_rec_flip(0.0)
        assert "in flight" in str(e.value)
        got = s.wait_batch(ticket)
        assert s.rec_flip == np.float32(0.95) and len(got) == 2
        s.set_rec_flip(0.0)
        assert s.rec_flip == 0.0
    finally:
        s.close()

"""Lexicon snap inside the pipeline on the MI355X (rt_lexicon_set_snap, rt_results_rec_lexicon_snapped): on
test_gpu_lexicon_pipeline.py's page, boxes and session settings -- three lanes, word boxes on, candidates = 3.  Each line gets a
lexicon built from its perturbed variants WITHOUT its greedy token string, so the winner differs from the greedy text and a
snapped line shows: its tokens, text, time steps, candidates, score and words are those of match 0 aligned to the line, every
other line and every det and cls result is what it is without snap, bit for bit, and so are the matches of every line.

Words: a snapped line's words equal, quads bit for bit, what rt_debug_word_boxes gives for the returned tokens and time steps
with the line's own geometry: its quad, the crop dims of that quad, the rec width W of the line's batch and the width the crop
is resized to inside it (line_geometry restates how the pipeline plans them)."""
import numpy as np
import pytest

import retto_amd
from retto_amd import synth

import crop_source_cases as CS
from test_gpu_charset_pipeline import reference_rows
from test_gpu_lexicon_pipeline import _session, bits, matches_of, variants

pytestmark = pytest.mark.gpu

TINY = 1e-30          # a threshold every line with a match reaches
STATIC = ("boxes", "det_scores", "labels", "cls_scores")


def prepare(s):
    page, m = CS.page_with_tall_line()
    B = np.stack([d.boxes.as_array() for d in s.run_batch([page], det_map_override=[m])[0].det_result])
    assert len(B) == 6
    ref = s.run_regions([page], [B])[0]
    rows = reference_rows(s, page, B)
    lexs = []
    for k, g in enumerate(ref.rec_result):   # the line's variants without its greedy token string
        lex = [e for e in variants(g.tokens, rows[k]) if e != [int(t) for t in g.tokens]]
        assert lex
        lexs.append(lex)
    ids = [s.create_lexicon(ids=lex) for lex in lexs]
    every = [e for lex in lexs for e in lex]
    every = [e for i, e in enumerate(every) if e not in every[:i]]
    all_id = s.create_lexicon(ids=every)
    dup = s.create_lexicon(ids=lexs[4] + lexs[4])    # every entry twice: match 0's posterior is at most 0.5
    off = s.run_regions([page], [B], lexicons=[ids])[0]
    assert CS.digest(off) == CS.digest(ref) and all(g.lexicon_snapped is False for g in off.rec_result)
    return {"page": page, "map": m, "B": B, "ref": ref, "rows": rows, "lexs": lexs, "ids": ids, "every": every, "all": all_id,
            "dup": dup, "off": off, "geom": line_geometry(s, B)}


@pytest.fixture(scope="module")
def session():
    s = _session()
    s.case = prepare(s)
    yield s
    s.close()


@pytest.fixture()
def snap_on(session):
    """every lexicon snaps wherever it has a match, but the doubled one, which needs 0.75"""
    c = session.case
    for k in c["ids"] + [c["all"]]:
        session.set_lexicon_snap(k, TINY)
    session.set_lexicon_snap(c["dup"], 0.75)
    yield session
    for k in c["ids"] + [c["all"], c["dup"]]:
        session.set_lexicon_snap(k, 0.0)


def line_geometry(s, B):
    """per line (W, resized_w) as the pipeline plans them for the quads B of one page: the crops' dims (rt_crop_dims), lines in
    batches of rec batch_num by descending h / w, a batch's W from the widest of its lines (never below the rec shape's own
    ratio; float32, rt_resize_norm_width), resized_w = min(ceil(rec_h * w / h), W)"""
    import ctypes as C
    import math
    lib = s._hd.lib
    n = len(B)
    b = np.ascontiguousarray(B, np.float32).reshape(-1, 8)
    ws = np.zeros(n, np.int32); hs = np.zeros(n, np.int32)
    assert lib.rt_crop_dims(b.ctypes.data_as(C.c_void_p), n, ws.ctypes.data_as(C.c_void_p), hs.ctypes.data_as(C.c_void_p)) == 0
    rc = s.config.rec_processor_config
    rh, rw, bn = int(rc.image_shape[1]), int(rc.image_shape[2]), int(rc.batch_num)
    order = sorted(range(n), key=lambda i: -(float(hs[i]) / float(ws[i])))   # (stable, as the pipeline's sort)
    out = [None] * n
    for s0 in range(0, n, bn):
        batch = order[s0:s0 + bn]
        ratio = np.float32(rw) / np.float32(rh)
        for i in batch:
            ratio = max(ratio, np.float32(ws[i]) / np.float32(hs[i]))
        W = lib.rt_resize_norm_width(rh, rw, float(ratio))
        for i in batch:
            out[i] = (W, min(int(math.ceil(float(rh) * float(ws[i]) / float(hs[i]))), W))
    return out


def _line(d, k):
    return {key: v[k] for key, v in d.items()}


def check_snapped_line(s, g, lexicon, T, quad, page, what, cl, geom):
    """a snapped line (cl: its cls result, geom: its (W, resized_w)) against its match 0"""
    rot180 = cl.label.label == 180 and np.float32(cl.label.score) >= np.float32(0.9)   # (rt_config.cls_thresh)
    assert g.lexicon_snapped is True, what
    e, text, _ll, _p = g.lexicon_matches[0]
    assert g.tokens.tolist() == lexicon[e] and g.text == text == "".join(s._dictionary()[i] for i in lexicon[e]), what
    cols = g.token_cols.tolist()
    assert len(cols) == len(g.tokens) and all(a < b for a, b in zip(cols, cols[1:])) and 0 <= cols[0] and cols[-1] < T, (what, cols, T)
    assert all(c[0][0] == int(t) for c, t in zip(g.candidates, g.tokens)), what
    assert all(0.0 <= c[0][2] <= 1.0 for c in g.candidates), what
    assert all(i != c[0][0] for c in g.candidates for i, _t, _p2 in c[1:]), what
    assert abs(np.mean([c[0][2] for c in g.candidates]) - g.score) <= 1e-6, what      # (as test_gpu_candidates.py computes it)
    want = retto_amd.debug_word_boxes(synth.synth_models(0)[3], g.tokens, cols, T, geom[0], geom[1], quad, rot180, page.shape[1],
                                      page.shape[0], page.shape[1], page.shape[0])
    key = lambda w: (w.text, w.kind, w.first_token, w.n_tokens, w.first_col, w.last_col,
                     np.ascontiguousarray(w.box.as_array(), np.float32).tobytes())
    assert len(g.words) == len(want) >= 1, what
    for x, y in zip(g.words, want):
        assert key(x) == key(y), (what, x, y)


def test_every_lexicon_line_takes_its_aligned_winner(snap_on):
    s, c = snap_on, snap_on.case
    page, B, off = c["page"], c["B"], c["off"]
    on = s.run_regions([page], [B], lexicons=[c["ids"]])[0]
    a, b = CS.digest(on), CS.digest(off)
    for key in STATIC:
        assert a[key] == b[key], key
    assert bits(matches_of(on)) == bits(matches_of(off))
    changed = 0
    for k, g in enumerate(on.rec_result):
        check_snapped_line(s, g, c["lexs"][k], len(c["rows"][k]), B[k], page, k, on.cls_result[k], c["geom"][k])
        changed += g.text != off.rec_result[k].text
    assert changed == 6    # no lexicon holds its line's greedy string
    # some lines only: the others, and the page's det and cls results, are bit-identical to the run without snap
    lx = [c["ids"][0], 0, c["ids"][2], 0, c["dup"], -1]
    some = s.run_regions([page], [B], lexicons=[lx])[0]
    d = CS.digest(some)
    for key in STATIC:
        assert d[key] == b[key], key
    for k in (1, 3, 5):
        assert _line(d, k) == _line(b, k) and some.rec_result[k].lexicon_snapped is None and some.rec_result[k].lexicon_matches is None
    for k in (0, 2):
        assert _line(d, k) == _line(a, k) and some.rec_result[k].lexicon_snapped is True
    # the doubled lexicon: match 0's posterior stays below the 0.75 it would need, so the line is the plain one
    g = some.rec_result[4]
    assert g.lexicon_snapped is False and 0.0 < g.lexicon_matches[0][3] <= 0.5 + 1e-6 and _line(d, 4) == _line(b, 4)
    s.set_lexicon_snap(c["dup"], float(np.float32(g.lexicon_matches[0][3])))     # the measured posterior itself is reached (>=)
    low = s.run_regions([page], [B], lexicons=[lx])[0]
    check_snapped_line(s, low.rec_result[4], c["lexs"][4] + c["lexs"][4], len(c["rows"][4]), B[4], page, "doubled", low.cls_result[4],
                       c["geom"][4])
    assert low.rec_result[4].lexicon_matches[0][0] < len(c["lexs"][4])    # the first copy
    assert bits(matches_of(low)) == bits(matches_of(some))


def test_threshold_above_a_lines_posterior_leaves_the_line_alone(snap_on):
    """the chosen line is the one with the doubled lexicon: its best entry's posterior is at most 0.5, so a threshold just above
    the measured value exists; the next float32 up leaves the line alone, the value itself is reached (>=)"""
    s, c = snap_on, snap_on.case
    page, B, off = c["page"], c["B"], c["off"]
    lx = c["ids"][:4] + [c["dup"]] + c["ids"][5:]
    s.set_lexicon_snap(c["dup"], 0.0)
    base = s.run_regions([page], [B], lexicons=[lx])[0]
    post = np.float32(base.rec_result[4].lexicon_matches[0][3])
    assert 0.0 < post <= 0.5 + 1e-6 and base.rec_result[4].lexicon_snapped is False
    s.set_lexicon_snap(c["dup"], float(np.nextafter(post, np.float32(2.0))))
    r = s.run_regions([page], [B], lexicons=[lx])[0]
    assert r.rec_result[4].lexicon_snapped is False and _line(CS.digest(r), 4) == _line(CS.digest(off), 4)
    assert [g.lexicon_snapped for g in r.rec_result] == [True, True, True, True, False, True]
    assert bits(matches_of(r)) == bits(matches_of(base))
    s.set_lexicon_snap(c["dup"], float(post))
    assert s.lexicon_snap(c["dup"]) == float(post) and s.lexicon_snap(99) == 0.0
    assert s.run_regions([page], [B], lexicons=[lx])[0].rec_result[4].lexicon_snapped is True


def test_every_entry_point_gives_the_same_snapped_lines(snap_on):
    s, c = snap_on, snap_on.case
    page, m, B = c["page"], c["map"], c["B"]
    explicit = s.run_regions([page], [B], lexicons=[[c["all"]] * 6])[0]
    want = CS.digest(explicit, boxes=False)
    flags = [g.lexicon_snapped for g in explicit.rec_result]
    assert flags == [True] * 6
    for k, g in enumerate(explicit.rec_result):
        check_snapped_line(s, g, c["every"], len(c["rows"][k]), B[k], page, ("all", k), explicit.cls_result[k], c["geom"][k])
    s.set_rec_lexicon(c["all"])
    try:
        a = s.run_batch([page], det_map_override=[m])[0]
        t = s.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[m])
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            s.set_lexicon_snap(c["all"], 0.5)    # like every other call while a ticket is out
        w = s.wait_batch(t)[0]
        d = s.run_regions([page], [B])[0]
        two = s.run_regions([page, page], [B, B], lexicons=[None, [0, -1, 0, c["ids"][3], 0, 0]])
        for r in (a, w, d, two[0]):
            assert CS.digest(r, boxes=False) == want and [g.lexicon_snapped for g in r.rec_result] == flags
            assert bits(matches_of(r)) == bits(matches_of(explicit))
        assert [g.lexicon_snapped for g in two[1].rec_result] == [None, True, None, True, None, None]
        assert _line(CS.digest(two[1], boxes=False), 1) == _line(want, 1)
    finally:
        s.set_rec_lexicon(0)
    assert s.lexicon_snap(c["all"]) == pytest.approx(TINY)


def test_a_charset_beside_the_lexicon(snap_on):
    """the charset writes first and a snap that fires overwrites its rows; where it does not fire the charset's decode stands"""
    s, c = snap_on, snap_on.case
    page, B = c["page"], c["B"]
    n = len(s._dictionary())
    half = s.create_charset(ids=np.flatnonzero(np.random.default_rng(2024).random(n) < 0.5).tolist())
    S = set(s.charset_classes(half).tolist())
    cs = [0, half, 0, 0, half, half]
    lx = [c["ids"][0], c["ids"][1], 0, 0, c["dup"], 0]
    only_cs = s.run_regions([page], [B], charsets=[cs])[0]
    only_lx = s.run_regions([page], [B], lexicons=[lx])[0]
    both = s.run_regions([page], [B], charsets=[cs], lexicons=[lx])[0]
    dc, dl, db = CS.digest(only_cs), CS.digest(only_lx), CS.digest(both)
    assert bits(matches_of(both)) == bits(matches_of(only_lx))     # the lexicon reads the model's own distribution
    assert [g.lexicon_snapped for g in both.rec_result] == [True, True, None, None, False, None]
    assert _line(db, 0) == _line(dl, 0)
    # line 1: the snap wins over the charset -- tokens, text, time steps, rank 0, score and words are the lexicon-only run's
    g, h = both.rec_result[1], only_lx.rec_result[1]
    check_snapped_line(s, g, c["lexs"][1], len(c["rows"][1]), B[1], page, "charset and snap", both.cls_result[1], c["geom"][1])
    for key in ("tokens", "text", "rec_scores", "words"):
        assert db[key][1] == dl[key][1], key
    assert g.token_cols.tolist() == h.token_cols.tolist()
    assert [np.float32(x[0][2]).tobytes() for x in g.candidates] == [np.float32(x[0][2]).tobytes() for x in h.candidates]
    assert all(i in S or i == -1 for x in g.candidates for i, _t, _p in x[1:])     # ranks >= 1 keep the charset's restriction
    # lines 4 and 5: no snap fires, the charset's decode stands
    for k in (4, 5):
        assert _line(db, k) == _line(dc, k)
    for k in (2, 3):
        assert _line(db, k) == _line(CS.digest(c["ref"]), k)


def test_argument_errors_and_thresholds_back_to_zero(session):
    s, c = session, session.case
    with pytest.raises(retto_amd.InvalidArgument, match=r"rt_lexicon_set_snap: unknown lexicon id 99"):
        s.set_lexicon_snap(99, 0.5)
    with pytest.raises(retto_amd.InvalidArgument, match=r"unknown lexicon id 0"):
        s.set_lexicon_snap(0, 0.5)
    for bad in (float("nan"), 1.5, -0.25, float("inf")):
        with pytest.raises(retto_amd.InvalidArgument, match=r"min_posterior \S+ is outside \[0, 1\]"):
            s.set_lexicon_snap(c["ids"][0], bad)
    assert s.lexicon_snap(c["ids"][0]) == 0.0
    s.set_lexicon_snap(c["ids"][0], 1.0)
    assert s.lexicon_snap(c["ids"][0]) == 1.0
    s.set_lexicon_snap(c["ids"][0], 0.0)
    # every threshold 0 again: the pipeline is the one without snap
    r = s.run_regions([c["page"]], [c["B"]], lexicons=[c["ids"]])[0]
    assert CS.digest(r) == CS.digest(c["ref"]) and all(g.lexicon_snapped is False for g in r.rec_result)
    assert bits(matches_of(r)) == bits(matches_of(c["off"]))

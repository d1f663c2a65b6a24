"""Rec charsets inside the pipeline on the MI355X (rt_charset_create, rt_set_rec_charset, rt_run_regions_charsets): on
test_gpu_regions.py's page and its six boxes, three lanes, word boxes and candidates on.  Lines without a charset are compared bit
for bit with a run without charsets; restricted lines are teacher-forced from the probability rows the same session's rt_rec
returns for them."""
import numpy as np
import pytest

import retto_amd
from retto_amd import synth
from oracle import ref_lib as OR

import crop_source_cases as CS
import ctc_candidates_ref as R

pytestmark = pytest.mark.gpu

PIPE_TOL = 2e-4   # test_gpu_candidates.py: the project's bar for the rec softmax against the same session's rt_rec rows


def _session(**kw):
    cfg = retto_amd.synthetic_session_config(0, crop_source="Original", max_side_len=CS.SMALL_LIMIT, lanes=3, **kw)
    cfg.rec_processor_config.return_word_box = True
    cfg.rec_processor_config.return_candidates = 3
    return retto_amd.RettoSession(cfg)


def make_sets(s):
    """the charsets of these tests: ten classes by their dictionary text; 300, about half and all of the classes by id"""
    ents = s._dictionary()
    n = len(ents)
    rng = np.random.default_rng(2024)
    ten = sorted(rng.choice(np.arange(1, n - 1), 10, replace=False).tolist())
    half = np.flatnonzero(rng.random(n) < 0.5).tolist()
    three_hundred = np.random.default_rng(30002).choice(np.arange(1, n), 300, replace=False).tolist()
    ids = {"ten": s.create_charset("".join(ents[c] for c in ten)), "half": s.create_charset(ids=half),
           "full": s.create_charset(ids=range(n)), "three_hundred": s.create_charset(ids=three_hundred)}
    assert len(s.charset_classes(ids["three_hundred"])) == 301
    assert set(ten) <= set(s.charset_classes(ids["ten"]).tolist())   # (duplicate entries of a character join as well)
    assert s.charset_classes(ids["half"]).tolist() == sorted(set(half) | {0})
    assert s.charset_classes(ids["full"]).tolist() == list(range(n))
    return ids


@pytest.fixture(scope="module")
def session():
    s = _session()
    s.sets = make_sets(s)
    yield s
    s.close()


@pytest.fixture(scope="module")
def page_and_boxes(session):
    page, m = CS.page_with_tall_line()
    r = session.run_batch([page], det_map_override=[m])[0]
    B = np.stack([d.boxes.as_array() for d in r.det_result])
    assert len(B) == 6
    return page, m, B, session.run_regions([page], [B])[0]


def _line(d, k):
    return {key: v[k] for key, v in d.items()}


def _in_set(g, S):
    return set(g.tokens.tolist()) <= S and all(i in S or i == -1 for tok in g.candidates for i, _t, _p in tok)


def test_charsets_on_two_regions_only(session, page_and_boxes):
    page, _m, B, ref = page_and_boxes
    cs = [0, session.sets["ten"], 0, 0, session.sets["half"], 0]
    r = session.run_regions([page], [B], charsets=[cs])[0]
    a, b = CS.digest(r), CS.digest(ref)
    for key in ("boxes", "det_scores", "labels", "cls_scores"):
        assert a[key] == b[key], key
    for k in (0, 2, 3, 5):
        assert _line(a, k) == _line(b, k), (k, CS.differing(a, b))
    for k in (1, 4):
        S = set(session.charset_classes(cs[k]).tolist())
        g = r.rec_result[k]
        assert _in_set(g, S) and g.words is not None and len(g.candidates) == len(g.tokens) == len(g.token_cols)
        assert all(c[0][0] == int(t) for c, t in zip(g.candidates, g.tokens))
        if len(g.tokens):
            assert abs(np.mean([c[0][2] for c in g.candidates]) - g.score) <= 1e-6
    assert not set(ref.rec_result[1].tokens.tolist()) <= set(session.charset_classes(cs[1]).tolist())   # the restriction bit
    # 0 for every region is rt_run_regions itself
    assert CS.digest(session.run_regions([page], [B], charsets=[[0] * 6])[0]) == b


def test_permuting_quads_and_charsets_permutes_the_results(session, page_and_boxes):
    page, _m, B, _ = page_and_boxes
    cs = np.array([0, session.sets["ten"], 0, session.sets["full"], session.sets["half"], 0])
    perm = [3, 0, 5, 1, 4, 2]
    a = CS.digest(session.run_regions([page], [B], charsets=[cs])[0])
    b = CS.digest(session.run_regions([page], [B[perm]], charsets=[cs[perm]])[0])
    for key in a:
        assert b[key] == [a[key][k] for k in perm], key


def test_session_default_through_every_entry_point(session, page_and_boxes):
    page, m, B, ref = page_and_boxes
    ten = session.sets["ten"]
    S = set(session.charset_classes(ten).tolist())
    plain = CS.digest(session.run_batch([page], det_map_override=[m])[0])
    explicit = CS.digest(session.run_regions([page], [B], charsets=[[ten] * 6])[0], boxes=False)
    session.set_rec_charset(ten)
    try:
        a = session.run_batch([page], det_map_override=[m])[0]
        assert all(_in_set(g, S) for g in a.rec_result) and sum(len(g.tokens) for g in a.rec_result) > 0
        da = CS.digest(a)
        assert {k: da[k] for k in explicit} == explicit
        t = session.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[m])
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            session.set_rec_charset(0)    # like every other call while a ticket is out
        assert CS.digest(session.wait_batch(t)[0]) == da
        assert CS.digest(session.run_regions([page], [B])[0], boxes=False) == explicit
        assert CS.digest(session.run_regions([page], [B], charsets=[[-1] * 6])[0], boxes=False) == explicit
        mixed = session.run_regions([page, page], [B, B], charsets=[None, [0, -1, 0, 0, 0, 0]])
        assert CS.digest(mixed[0], boxes=False) == explicit
        d1, dr = CS.digest(mixed[1]), CS.digest(ref)
        assert _line(d1, 1) == {k: v[1] for k, v in CS.digest(session.run_regions([page], [B])[0]).items()}
        assert all(_line(d1, k) == _line(dr, k) for k in (0, 2, 3, 4, 5))
    finally:
        session.set_rec_charset(0)
    assert CS.digest(session.run_batch([page], det_map_override=[m])[0]) == plain
    assert CS.digest(session.run_regions([page], [B])[0]) == CS.digest(ref)


def test_unknown_ids_are_rejected_and_the_session_lives_on(session, page_and_boxes):
    page, _m, B, ref = page_and_boxes
    with pytest.raises(retto_amd.InvalidArgument, match=r"page 1 region 2: unknown charset id 99"):
        session.run_regions([page, page], [B, B], charsets=[None, [0, 0, 99, 0, 0, 0]])
    with pytest.raises(retto_amd.InvalidArgument, match=r"page 0 region 5: unknown charset id -2"):
        session.run_regions([page], [B], charsets=[[0, 0, 0, 0, 0, -2]])
    with pytest.raises(retto_amd.InvalidArgument, match=r"unknown charset id 99"):
        session.set_rec_charset(99)
    with pytest.raises(retto_amd.InvalidArgument, match=r"U\+0041"):
        session.create_charset("A")   # the synthetic dictionary has no Latin entry
    assert len(session.charset_classes(99)) == 0
    assert CS.digest(session.run_regions([page], [B])[0]) == CS.digest(ref)


# ---------------------------------------------------------------- teacher-forced
def reference_rows(session, page, B):
    """per region the probability rows [T, classes] the same session's rt_rec returns for it: the crops, the cls rotation and
    the rec batches formed as the pipeline forms them (oracle.pipeline), the networks the session's own"""
    from oracle.pipeline import OracleSession
    o = OracleSession(*synth.synth_models(0), max_side_len=CS.SMALL_LIMIT)
    o.cls_worker = session.worker.cls
    calls = []

    def rec_worker(t):
        calls.append(session.worker.rec(t))
        return calls[-1]
    o.rec_worker = rec_worker
    crops = [OR.get_crop_img(page, b) for b in B]
    dims = [c.shape[:2] for c in crops]
    o.cls_process(crops, dims)
    o.rec_process(crops, dims)
    order = sorted(range(len(crops)), key=lambda i: -(float(dims[i][0]) / float(dims[i][1])))
    rows = [None] * len(crops)
    for bi, p in enumerate(calls):
        for j, i in enumerate(order[6 * bi:6 * bi + 6]):
            rows[i] = p[j]
    return rows


def masked_reference(p, S):
    """(argmax over S per step, its probability normalised over S, the smallest normalised top-2 gap of the line)"""
    S = np.asarray(sorted(S))
    pS = p[:, S].astype(np.float64)
    norm = pS / pS.sum(axis=1, keepdims=True)
    top = np.sort(norm, axis=1)
    gap = float((top[:, -1] - top[:, -2]).min()) if len(S) > 1 else np.inf
    return S[np.argmax(pS, axis=1)], norm.max(axis=1), gap


# The sets and the page were picked on the MI355X from the reference rows alone (rt_rec of the session, no charset code): on
# page_with_tall_line(seed = 2) the smallest normalised top-2 gap of the six lines is 8.5e-4 over every class, 7.1e-3 over the 300
# classes and 2.9e-4 .. 1.6e-2 over the half set (one line below 2 PIPE_TOL = 4e-4: skipped); sets of ten classes were clear on
# every line of fourteen pages (gap >= 4.6e-3).  On test_gpu_regions.py's own page (seed 7) only one line in six is clear over
# every class, so the teacher-forced lines are another seed of the same page.  Measured: 23 of the 24 lines compared, 1 skipped.
TF_PAGE_SEED = 2
TF_SETS = ("ten", "three_hundred", "half", "full")


def test_restricted_lines_teacher_forced(session):
    page, m = CS.page_with_tall_line(TF_PAGE_SEED)
    B = np.stack([d.boxes.as_array() for d in session.run_batch([page], det_map_override=[m])[0].det_result])
    assert len(B) == 6
    ref = session.run_regions([page], [B])[0]
    rows = reference_rows(session, page, B)
    compared = skipped = 0
    for name in TF_SETS:
        cid = session.sets[name]
        S = session.charset_classes(cid).tolist()
        r = session.run_regions([page], [B], charsets=[[cid] * 6])[0]
        for k, g in enumerate(r.rec_result):
            am, pm, gap = masked_reference(rows[k], S)
            if not gap > 2 * PIPE_TOL:
                skipped += 1
                continue
            kc = R.kept_cols(am)
            assert g.tokens.tolist() == [int(am[t]) for t in kc], (name, k)
            assert [int(c) for c in g.token_cols] == kc, (name, k)
            assert all(abs(c[0][2] - pm[t]) <= PIPE_TOL for c, t in zip(g.candidates, kc)), (name, k)
            if name == "full":   # every class allowed: the unrestricted decode
                assert g.tokens.tolist() == ref.rec_result[k].tokens.tolist(), k
            compared += 1
    print("teacher-forced: %d lines compared, %d skipped" % (compared, skipped))
    assert compared >= 5 and skipped * 10 <= compared + skipped, (compared, skipped)


def test_fp16_mobile_session(page_and_boxes):
    page, _m, B, _ = page_and_boxes
    s = _session(dtype="f16")
    try:
        sets = make_sets(s)
        ref = CS.digest(s.run_regions([page], [B])[0])
        cs = [sets["half"], 0, 0, sets["ten"], 0, sets["ten"]]
        r = s.run_regions([page], [B], charsets=[cs])[0]
        a = CS.digest(r)
        assert all(_line(a, k) == _line(ref, k) for k in (1, 2, 4))
        for k in (0, 3, 5):
            assert _in_set(r.rec_result[k], set(s.charset_classes(cs[k]).tolist())), k
        assert sum(len(r.rec_result[k].tokens) for k in (0, 3, 5)) > 0
        # the cap: RT_MAX_CHARSETS per session
        for _ in range(retto_amd._lib.MAX_CHARSETS - len(sets)):
            s.create_charset(ids=[1])
        with pytest.raises(retto_amd.CapacityError, match="RT_MAX_CHARSETS"):
            s.create_charset(ids=[1])
        assert CS.digest(s.run_regions([page], [B], charsets=[cs])[0]) == a
    finally:
        s.close()

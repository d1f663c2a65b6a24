"""Rec lexicons inside the pipeline on the MI355X (rt_lexicon_create, rt_set_rec_lexicon, rt_run_regions_lexicons,
rt_results_rec_lexicon): on test_gpu_regions.py's page and its six boxes, three lanes, word boxes and candidates on.  Everything
but the matches is compared bit for bit with a run without lexicons; the matches are teacher-forced from the probability rows the
same session's rt_rec returns for the lines, through ctc_lexicon_ref.check_outputs.

The teacher-forced reference is log(p) of rt_rec's fp32 softmax rows, which come from the fused head, another GEMM launch than the
lexicons' recomputed logits, so its own error joins the kernels': measured on the MI355X over the six lines x their lexicons,
worst |loglik - reference| = 2.310e-5 and |posterior - reference| = 9.107e-7 in the fp32 session (each line against its own lexicon;
1.51e-5 / 7.1e-7 against the lexicon of all lines, 1.55e-5 / 5.3e-7 with charsets beside), 1.567e-5 and 1.332e-6 in the fp16-dtype
session (the same fp32 rule over features an fp16 network computed twice, batched differently); each tolerance is four times its
figure."""
import numpy as np
import pytest

import retto_amd

import crop_source_cases as CS
import ctc_lexicon_ref as LR
from test_gpu_charset_pipeline import reference_rows

pytestmark = pytest.mark.gpu

MEASURED_WORST = 2.310e-5        # fp32 session: worst |loglik - reference| over the teacher-forced lines
MEASURED_WORST_F16 = 1.567e-5    # fp16-dtype session
MEASURED_WORST_POST = 9.107e-7       # ... and worst |posterior - reference|
MEASURED_WORST_POST_F16 = 1.332e-6
PIPE_TOL, PIPE_PTOL = 4 * MEASURED_WORST, 4 * MEASURED_WORST_POST
PIPE_TOL_F16, PIPE_PTOL_F16 = 4 * MEASURED_WORST_F16, 4 * MEASURED_WORST_POST_F16


def _session(**kw):
    cfg = retto_amd.synthetic_session_config(0, crop_source="Original", max_side_len=CS.SMALL_LIMIT, lanes=3, **kw)
    cfg.rec_processor_config.return_word_box = True
    cfg.rec_processor_config.return_candidates = 3
    return retto_amd.RettoSession(cfg)


def variants(tokens, p):
    """a line's lexicon: its greedy tokens (the first 20 of a longer line) and perturbed variants -- a token dropped, doubled (equal
    neighbours), replaced by the step's runner-up class, two neighbours swapped, the halves -- without repeats, at most 31 long"""
    base = [int(t) for t in tokens][:20] or [int(np.argsort(p.sum(axis=0))[-2]) or 1]
    runner = [int(c) for c in np.argsort(p, axis=1)[:, -2]]
    out = [base]
    for j in range(len(base)):
        out.append(base[:j] + base[j + 1:])
        out.append(base[:j] + [base[j]] + base[j:])
        out.append(base[:j] + [runner[(j * len(runner)) // len(base)] or base[j]] + base[j + 1:])
        if j + 1 < len(base):
            out.append(base[:j] + [base[j + 1], base[j]] + base[j + 2:])
    out += [base[:len(base) // 2], base[len(base) // 2:], base + base[-1:]]
    seen, lex = set(), []
    for e in out:
        if e and len(e) <= LR.MAX_LEN and tuple(e) not in seen:
            seen.add(tuple(e)); lex.append(e)
    return lex


def prepare(s):
    """the page, its six boxes, the plain regions run, rt_rec's rows per line, and one lexicon per line plus the one that holds
    them all, created on the session"""
    page, m = CS.page_with_tall_line()
    B = np.stack([d.boxes.as_array() for d in s.run_batch([page], det_map_override=[m])[0].det_result])
    assert len(B) == 6
    ref = s.run_regions([page], [B])[0]
    rows = reference_rows(s, page, B)
    lexs = [variants(g.tokens, rows[k]) for k, g in enumerate(ref.rec_result)]
    ids = [s.create_lexicon(ids=lex) for lex in lexs]
    every = [e for lex in lexs for e in lex]
    every = [e for i, e in enumerate(every) if e not in every[:i]]
    all_id = s.create_lexicon(ids=every)
    assert ids == list(range(1, 7)) and all_id == 7
    got = s.lexicon_entries(ids[2])
    assert [e for e, _t in got] == lexs[2] and got[0][1] == "".join(s._dictionary()[c] for c in lexs[2][0])
    return {"page": page, "map": m, "B": B, "ref": ref, "rows": rows, "lexs": lexs, "ids": ids, "every": every, "all": all_id}


@pytest.fixture(scope="module")
def session():
    s = _session()
    s.case = prepare(s)
    yield s
    s.close()


def as_out(rec_result):
    """a page's lexicon_matches in the layout ctc_lexicon_ref.check_outputs reads (no table: the pipeline returns matches only)"""
    m = np.empty((len(rec_result), LR.MATCHES), LR.MATCH)
    m["entry"] = LR.CANARY_ENTRY; m["loglik"] = LR.CANARY_F; m["posterior"] = LR.CANARY_F
    n = np.zeros(len(rec_result), np.int32)
    for k, g in enumerate(rec_result):
        for j, (e, _text, ll, post) in enumerate(g.lexicon_matches or []):
            m[k][j] = (e, ll, post)
        n[k] = len(g.lexicon_matches or [])
    return {"table": None, "matches": m, "n": n}


def teacher_forced(rows, line_lex, lexicons):
    """ctc_lexicon_ref.reference from rt_rec's probability rows: lp = log(p) in fp64"""
    ref = []
    for p, k in zip(rows, line_lex):
        if k == 0:
            ref.append(None)
            continue
        # (a probability that underflowed to 0 in rt_rec's fp32 softmax is taken as the smallest positive float32: an entry through
        # such a class is hundreds of nats below the line's matches and only has to stay feasible in the reference)
        ll = LR.loglik64(np.log(np.maximum(p.astype(np.float64), float(np.finfo(np.float32).smallest_subnormal))), lexicons[k - 1])
        with np.errstate(invalid="ignore"):
            ref.append((ll, np.where(np.isneginf(ll), 0.0, np.exp(ll - LR._lse(ll))) if np.isfinite(ll).any() else np.zeros(len(ll))))
    return ref


def matches_of(r):
    return [g.lexicon_matches for g in r.rec_result]


def bits(ms):
    return [None if m is None else [(e, t, np.float32(ll).tobytes(), np.float32(p).tobytes()) for e, t, ll, p in m] for m in ms]


def check_page(s, r, line_lex, tol, ptol, what):
    c = s.case
    lexicons = c["lexs"] + [c["every"]]
    tpl = [len(p) for p in c["rows"]]
    for g, k in zip(r.rec_result, line_lex):
        assert (g.lexicon_matches is None) == (k == 0)
        for e, text, _ll, _p in g.lexicon_matches or []:
            assert text == "".join(s._dictionary()[i] for i in lexicons[k - 1][e])
    wl, wp = LR.check_outputs(as_out(r.rec_result), teacher_forced(c["rows"], line_lex, lexicons), tpl, line_lex, lexicons, tol, ptol, what)
    print("%s: worst |loglik - reference| %.3e, worst |posterior - reference| %.3e" % (what, wl, wp))
    return wl


def test_matches_teacher_forced_and_the_rest_bit_identical(session):
    c = session.case
    r = session.run_regions([c["page"]], [c["B"]], lexicons=[c["ids"]])[0]
    assert CS.digest(r) == CS.digest(c["ref"]), CS.differing(CS.digest(r), CS.digest(c["ref"]))   # tokens, scores, boxes, cls, words, candidates
    assert all(g.lexicon_matches is None for g in c["ref"].rec_result)
    check_page(session, r, c["ids"], PIPE_TOL, PIPE_PTOL, "own lexicons")
    won = sum(1 for g, ref in zip(r.rec_result, c["ref"].rec_result) if len(ref.tokens) and g.lexicon_matches[0][0] == 0)
    print("lines whose greedy text wins its lexicon: %d of 6" % won)
    assert all(len(g.lexicon_matches) == min(LR.MATCHES, sum(len(p) >= LR.need(e) for e in lex))
               for g, p, lex in zip(r.rec_result, c["rows"], c["lexs"]))
    # the lexicon of all lines on every line
    r2 = session.run_regions([c["page"]], [c["B"]], lexicons=[[c["all"]] * 6])[0]
    assert CS.digest(r2) == CS.digest(c["ref"])
    check_page(session, r2, [7] * 6, PIPE_TOL, PIPE_PTOL, "the lexicon of all lines")


def test_session_default_through_every_entry_point(session):
    c = session.case
    page, m, B = c["page"], c["map"], c["B"]
    plain = CS.digest(session.run_batch([page], det_map_override=[m])[0])
    explicit = session.run_regions([page], [B], lexicons=[[c["all"]] * 6])[0]
    want = bits(matches_of(explicit))
    assert all(w for w in want)
    session.set_rec_lexicon(c["all"])
    try:
        a = session.run_batch([page], det_map_override=[m])[0]
        assert bits(matches_of(a)) == want and CS.digest(a) == plain
        t = session.submit_batch_raw([page], [page.shape[0]], [page.shape[1]], det_map_override=[m])
        with pytest.raises(retto_amd.InvalidArgument, match="in flight"):
            session.set_rec_lexicon(0)    # like every other call while a ticket is out
        w = session.wait_batch(t)[0]
        assert bits(matches_of(w)) == want and CS.digest(w) == plain
        assert bits(matches_of(session.run_regions([page], [B])[0])) == want
        assert bits(matches_of(session.run_regions([page], [B], lexicons=[[-1] * 6])[0])) == want
        two = session.run_regions([page, page], [B, B], lexicons=[None, [0, -1, 0, c["ids"][3], 0, 0]])
        assert bits(matches_of(two[0])) == want
        assert [g is None for g in matches_of(two[1])] == [True, False, True, False, True, True]
        assert bits(matches_of(two[1]))[1] == want[1]
        check_page(session, two[1], [0, 7, 0, c["ids"][3], 0, 0], PIPE_TOL, PIPE_PTOL, "per region")
        assert CS.digest(two[1]) == CS.digest(c["ref"])
    finally:
        session.set_rec_lexicon(0)
    after = session.run_batch([page], det_map_override=[m])[0]
    assert CS.digest(after) == plain and all(x is None for x in matches_of(after))


def test_a_region_with_a_charset_and_a_lexicon(session):
    """the charset changes the line's decode, the lexicon reads the model's own distribution: each as it is without the other"""
    c = session.case
    page, B = c["page"], c["B"]
    n = len(session._dictionary())
    half = session.create_charset(ids=np.flatnonzero(np.random.default_rng(2024).random(n) < 0.5).tolist())
    cs = [0, half, 0, 0, half, 0]
    lx = [c["ids"][0], c["ids"][1], 0, 0, c["all"], -1]
    only_cs = session.run_regions([page], [B], charsets=[cs])[0]
    only_lx = session.run_regions([page], [B], lexicons=[lx])[0]
    both = session.run_regions([page], [B], charsets=[cs], lexicons=[lx])[0]
    assert CS.digest(both) == CS.digest(only_cs) and CS.digest(only_cs) != CS.digest(c["ref"])
    assert CS.digest(only_lx) == CS.digest(c["ref"])
    assert bits(matches_of(both)) == bits(matches_of(only_lx))
    assert [x is None for x in matches_of(both)] == [False, False, True, True, False, True]
    check_page(session, both, [c["ids"][0], c["ids"][1], 0, 0, 7, 0], PIPE_TOL, PIPE_PTOL, "with charsets")


def test_unknown_ids_are_rejected_and_the_session_lives_on(session):
    c = session.case
    page, B = c["page"], c["B"]
    with pytest.raises(retto_amd.InvalidArgument, match=r"page 1 region 2: unknown lexicon id 99"):
        session.run_regions([page, page], [B, B], lexicons=[None, [0, 0, 99, 0, 0, 0]])
    with pytest.raises(retto_amd.InvalidArgument, match=r"page 0 region 5: unknown lexicon id -2"):
        session.run_regions([page], [B], lexicons=[[0, 0, 0, 0, 0, -2]])
    with pytest.raises(retto_amd.InvalidArgument, match=r"unknown lexicon id 99"):
        session.set_rec_lexicon(99)
    with pytest.raises(retto_amd.InvalidArgument, match=r"U\+0041 in entry 0"):
        session.create_lexicon(["A"])   # the synthetic dictionary has no Latin entry
    assert session.lexicon_entries(99) == []
    r = session.run_regions([page], [B], lexicons=[c["ids"]])[0]
    assert CS.digest(r) == CS.digest(c["ref"]) and all(x for x in matches_of(r))


def test_fp16_session_and_the_lexicon_cap():
    s = _session(dtype="f16")
    try:
        s.case = c = prepare(s)
        r = s.run_regions([c["page"]], [c["B"]], lexicons=[c["ids"]])[0]
        assert CS.digest(r) == CS.digest(c["ref"])
        check_page(s, r, c["ids"], PIPE_TOL_F16, PIPE_PTOL_F16, "fp16 session")
        # the cap: RT_MAX_LEXICONS per session
        for _ in range(retto_amd._lib.MAX_LEXICONS - 7):
            s.create_lexicon(ids=[[1]])
        with pytest.raises(retto_amd.CapacityError, match="RT_MAX_LEXICONS"):
            s.create_lexicon(ids=[[1]])
        assert bits(matches_of(s.run_regions([c["page"]], [c["B"]], lexicons=[c["ids"]])[0])) == bits(matches_of(r))
    finally:
        s.close()

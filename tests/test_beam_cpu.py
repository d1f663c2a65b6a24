"""Rec beams (retto_amd/csrc/ctc_beam.h) without a GPU: the rule in plain fp32 loops (rt_debug_ctc_beam_host) against the fp64
restatement in ctc_beam_ref.py on the grid of test_gpu_beam.py, by that test's own checker; the exhaustive case in which a beam
that never overflows must return the full CTC likelihood of every string -- what proves the merge; the exact tie case; the
checkers against the mutants they must refuse; what the arguments are held to; and the surface: exports, header, Python mirror."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

import ctc_beam_ref as BR
import ctc_lexicon_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host(case, B, nbest):
    rc, out = BR.call(_lib.load().rt_debug_ctc_beam_host, None, *case, B, nbest)
    assert rc == 0, _lib.load().rt_last_error(None)
    return out


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs and the fp64 rule per (N, beam), computed once"""
    g = {}
    for N in LR.GRID_N:
        case = BR.grid_case(N)
        g[N] = (case, {B: BR.reference(*case, B) for B, _ in BR.GRID_BEAMS})
    return g


# ---------------------------------------------------------------- the rule
def test_host_rule_on_the_grid_against_fp64(grid):
    """every check of the GPU test on the host rule; the figures its tolerances are four times of are measured here again; the
    condition on the ranks left out of the string comparison holds for the fp64 rule's own gaps on the chosen seeds; and the host
    rule run once more on logits a few ulp away meets every check as well"""
    stats = []
    for N in LR.GRID_N:
        case, refs = grid[N]
        z, W, b, tpl = case
        assert sorted(set(tpl)) == sorted(BR.GRID_T + (BR.GRID_LONG,)) and len(tpl) == 13
        for B, n in BR.GRID_BEAMS:
            st = BR.check(run_host(case, B, n), refs[B], tpl, N, B, n, BR.tol_of, what=("host", N, B, n))
            BR.check(run_host((z, BR.perturbed(W), b, tpl), B, n), refs[B], tpl, N, B, n, BR.tol_of, what=("host, perturbed", N, B, n))
            print("host fp32 against fp64, N = %d, beam %d / %d: %.3e up to 40 steps, %.3e on the long line; %d of %d ranks left out"
                  % ((N, B, n) + BR.worst_short_long(st) + (st["skipped"], st["ranks"])))
            stats.append(st)
    st = BR.merge_stats(stats)
    short, long_ = BR.worst_short_long(st)
    assert short <= BR.MEASURED_HOST_SHORT * 1.001 and long_ <= BR.MEASURED_HOST_LONG * 1.001, (short, long_)
    assert BR.TOL == 4 * BR.MEASURED_HOST_SHORT and BR.TOL_LONG == 4 * BR.MEASURED_HOST_LONG
    assert BR.condition_holds(st), st
    assert st["ranks"] > 600 and st["lines"] == 3 * 4 * 13


def test_exhaustive_case_returns_full_likelihoods():
    """classes = 3, T = 4, beam 32: the beam holds every string that has an alignment, so each logprob is the string's full CTC
    forward log-likelihood and the N-best are the true top N.  A merge that is forgotten, or folded into the wrong member, fails
    here."""
    case = BR.exhaustive_case(BR.EXHAUSTIVE_SEED)
    z, W, b, tpl = case
    lp = LR.logp64(LR.logits64(z, W, b))
    strings = BR.all_strings(2, 4)
    assert len(strings) == 31 <= BR.MAX_BEAM
    ll = {s: BR.loglik64(lp, s) for s in strings}
    order = sorted((s for s in strings if ll[s] > -np.inf), key=lambda s: -ll[s])
    gaps = [ll[order[k]] - ll[order[k + 1]] for k in range(BR.MAX_NBEST)]
    assert min(gaps) > 100 * BR.TOL, gaps
    out = run_host(case, 32, 8)
    H = BR.hyps_of(out, tpl, 8)[0]
    assert [s for s, _ in H] == order[:8], (H, order[:8])
    for s, v in H:
        assert abs(float(v) - ll[s]) <= BR.TOL, (s, float(v), ll[s])
    assert any(len(s) >= 2 and s[-1] != s[-2] for s, _ in H)
    BR.check(out, BR.reference(*case, 32), tpl, 3, 32, 8, BR.tol_of)
    # the fp64 restatement itself, against the definition
    R = dict(BR.beam64(LR.logits64(z, W, b), 32))
    assert set(R) == {s for s in strings if ll[s] > -np.inf}
    assert max(abs(R[s] - ll[s]) for s in R) < 1e-9


def check_ties(out, ref, tpl, nbest):
    """the exact tie rule: every string is the fp64 rule's with the same tie order"""
    H = BR.hyps_of(out, tpl, nbest)
    assert [[s for s, _ in h] for h in H] == [[s for s, _ in r[1][:nbest]] for r in ref]


@pytest.mark.parametrize("B", [2, 4])
def test_exact_ties_take_the_lower_id(B):
    case = BR.tie_case()
    z, W, b, tpl = case
    for c, c2 in BR.TIE_PAIRS:
        assert W[:, c].tobytes() == W[:, c2].tobytes() and b[c].tobytes() == b[c2].tobytes()
    ref = BR.reference(*case, B)
    out = run_host(case, B, B)
    check_ties(out, ref, tpl, B)
    H = BR.hyps_of(out, tpl, B)
    low, high = {c for c, _ in BR.TIE_PAIRS}, {c2 for _, c2 in BR.TIE_PAIRS}
    assert all(set(h[0][0]) & (low | high) for h in H)        # (every line's best string holds a class of a pair)
    n_ties = 0
    for h in H:
        for k in range(len(h) - 1):
            if h[k][1].tobytes() == h[k + 1][1].tobytes():    # (bit-equal totals: the lower id first)
                assert h[k][0] < h[k + 1][0], h
                n_ties += 1
    assert n_ties >= 2


def test_planted_strings_win_in_the_fp64_rule_and_on_the_host():
    for N in (65, 6625):
        z, W, b, tpl, entries, paths = BR.planted_case(N)
        for B, n in ((16, 4), (4, 4)):
            ref = BR.reference(z, W, b, tpl, B)
            H = BR.hyps_of(run_host((z, W, b, tpl), B, n), tpl, n)
            for i, (e, path) in enumerate(zip(entries, paths)):
                lp, R = ref[i]
                assert R[0][0] == tuple(e) == H[i][0][0], (N, B, i)
                assert R[0][1] - R[1][1] > 2 * BR.tol_of(tpl[i])
                path_lp = float(lp[np.arange(len(path)), path].sum())
                assert path_lp - BR.TOL_LONG <= float(H[i][0][1]) <= BR.loglik64(lp, tuple(e)) + BR.TOL_LONG


def test_stand_in_is_the_rule_and_every_mutant_is_caught(grid):
    ex = BR.exhaustive_case(BR.EXHAUSTIVE_SEED)
    tie = BR.tie_case()
    small, small_refs = grid[5]
    cases = [(lambda o: BR.check(o, BR.reference(*ex, 32), ex[3], 3, 32, 8, BR.tol_of), (ex, 32, 8)),
             (lambda o: check_ties(o, BR.reference(*tie, 4), tie[3], 4), (tie, 4, 4)),
             (lambda o: BR.check(o, small_refs[16], small[3], 5, 16, 8, BR.tol_of), (small, 16, 8))]
    for chk, (case, B, n) in cases:
        chk(BR.stand_in(*case, B, n))
    for m in BR.MUTANTS:
        caught = 0
        for chk, (case, B, n) in cases:
            try:
                chk(BR.stand_in(*case, B, n, mutant=m))
            except AssertionError:
                caught += 1
        assert caught >= 1, m
    # ... and by the cases meant for them
    for m, k in (("merge_forgotten", 0), ("repeat_takes_total", 0), ("ties_to_higher_index", 1), ("blank_in_top_c", 0)):
        chk, (case, B, n) = cases[k]
        with pytest.raises(AssertionError):
            chk(BR.stand_in(*case, B, n, mutant=m))


def test_checker_refuses_a_wrong_logprob_a_wrong_string_and_a_written_canary(grid):
    case, refs = grid[65]
    z, W, b, tpl = case
    good = run_host(case, 4, 4)
    i = tpl.index(40)
    o = sum(tpl[:i]) * 4
    for key, at, val in (("beams", (i, 0), (np.float32(good["beams"][i][0]["logprob"] + 0.05), good["beams"][i][0]["n_tokens"])),
                         ("tokens", o, 0), ("tokens", o + 39, 1), ("n", i, 3)):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][at] = val
        with pytest.raises(AssertionError):
            BR.check(bad, refs[4], tpl, 65, 4, 4, BR.tol_of)


# ---------------------------------------------------------------- arguments
def test_host_entry_rejects_bad_arguments_and_off_writes_nothing():
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f = lib.rt_debug_ctc_beam_host
    for tpl, B, n, msg in (([4], 33, 1, b"beam = 33 is outside [0, RT_MAX_BEAM]"), ([4], 4, 0, b"nbest = 0 is outside [1, min(beam, RT_MAX_NBEST)]"),
                           ([4], 4, 5, b"nbest = 5 is outside"), ([4], 32, 9, b"nbest = 9 is outside"), ([4], -1, 1, b"beam = -1"),
                           ([-4], 4, 1, b"line 0 has a negative number of time steps")):
        rc, out = BR.call(f, None, z, W, b, tpl, B, n)
        assert rc == 8 and msg in lib.rt_last_error(None), lib.rt_last_error(None)
        assert (out["n"] == BR.CANARY_N).all() and (out["tokens"] == BR.CANARY_TOK).all()
    rc, out = BR.call(f, None, z, W, b, [4], 0, 3)      # beam = 0: off
    assert rc == 0 and (out["n"] == BR.CANARY_N).all() and (out["beams"]["n_tokens"] == BR.CANARY_N).all() and (out["tokens"] == BR.CANARY_TOK).all()
    rc, out = BR.call(f, None, z, W, b, [], 4, 2)       # no line
    assert rc == 0 and (out["n"] == BR.CANARY_N).all() and (out["tokens"] == BR.CANARY_TOK).all()
    rc, out = BR.call(f, None, z, W, b, [0, 4, 0], 4, 2)   # lines without a time step report no hypothesis
    assert rc == 0 and out["n"].tolist() == [0, 2, 0]
    BR.hyps_of(out, [0, 4, 0], 2)
    # the setter and the getter without a session
    assert lib.rt_set_rec_beam(None, 4, 2) == 8 and b"rt_set_rec_beam: null session" in lib.rt_last_error(None)
    assert lib.rt_rec_beam(None, None, None) == 8
    assert lib.rt_results_rec_beams(None, 0, 0, None) == 0 and lib.rt_results_rec_beam_tokens(None, 0, 0, 0, None) == 0
    assert lib.rt_results_rec_beam_text(None, 0, 0, 0) is None


def test_all_zero_features_give_the_bias_distribution():
    """every step has the same distribution: with classes 1 and 2 far ahead, beam 1 reads the likelier of the two once"""
    z, W, b = LR.zero_feature_case(5, [-3.0, 2.0, 1.0, -9.0, -9.0], 6)
    out = run_host((z, W, b, [6]), 1, 1)
    H = BR.hyps_of(out, [6], 1)[0]
    assert H[0][0] == (1,)
    lp = LR.logp64(LR.logits64(z, W, b))
    assert float(H[0][1]) <= BR.loglik64(lp, (1,)) + BR.TOL


# ---------------------------------------------------------------- surface
def test_exports_header_and_python_mirror():
    names = ["rt_set_rec_beam", "rt_rec_beam", "rt_results_rec_beams", "rt_results_rec_beam_tokens", "rt_results_rec_beam_text",
             "rt_debug_ctc_beam", "rt_debug_ctc_beam_host"]
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n) and ("RT_API" in header and n + "(" in header), n
    assert "#define RT_MAX_BEAM 32" in header and "#define RT_MAX_NBEST 8" in header
    assert "typedef struct rt_beam { float logprob; int32_t n_tokens; } rt_beam;" in header
    assert (_lib.MAX_BEAM, _lib.MAX_NBEST) == (32, 8) == (BR.MAX_BEAM, BR.MAX_NBEST)
    assert C.sizeof(_lib.Beam) == BR.BEAM.itemsize == 8 and [f[0] for f in _lib.Beam._fields_] == list(BR.BEAM.names)
    S = retto_amd.RettoSession
    assert callable(S.set_rec_beam) and callable(S.rec_beam)
    assert inspect.signature(S.set_rec_beam).parameters["nbest"].default == 1
    assert retto_amd.RecProcessorSingleResult("", 0.0).beams is None
    h = retto_amd.BeamHypothesis(np.zeros(0, np.int32), "", -1.5)
    assert (h.text, h.logprob) == ("", -1.5)

"""numpy fp64 restatement of the lexicon snap rule (retto_amd/csrc/ctc_lexicon_align.h): a CTC Viterbi alignment with its
second-best path value, the checker the snap tests share, and a float32 numpy stand-in of the whole hook whose mutants the
checker must refuse (test_lexicon_align_cpu.py).  Nothing here decides what the library computes; call() only marshals the
arguments of rt_debug_ctc_lexicon_align / rt_debug_ctc_lexicon_align_host.  The lexicon half of a call (table, matches, counts)
is ctc_lexicon_ref's business and is checked by its check_outputs."""
import ctypes as C

import numpy as np

import ctc_lexicon_ref as LR

CANARY_IDX = -7                      # what the tests put into idx / snapped before a call (no class id, no flag)
CANARY_F = LR.CANARY_F               # and into prob / vit
MUTANTS = ("ties_to_previous_state", "skip_across_equal", "end_always_last_blank", "prob_over_raw_logits",
           "written_below_threshold", "neighbour_rows_written", "pad_columns_in_lse")
# Worst deviations from the fp64 reference measured on the MI355X over the hook grid (LR.grid_case at N = 5, 65, 6625, both
# chunkings; test_gpu_lexicon_align.py's docstring has them per N): for the Viterbi value the larger of |vit_out - the fp64 score
# of the returned path| and (fp64 optimum - that score); for the probabilities |prob - fp64 softmax|.  Each tolerance is 4 x its
# own figure, the convention of ctc_lexicon_ref.HOOK_TOL.
MEASURED_WORST_VIT = 7.830e-5
MEASURED_WORST_PROB = 1.753e-6
VIT_TOL = 4 * MEASURED_WORST_VIT
PROB_TOL = 4 * MEASURED_WORST_PROB
# The same Viterbi figure on the long lines of test_gpu_lexicon_align.test_long_lines_send_their_backpointers_through_memory (256
# to 513 steps, |Viterbi value| up to 3024: the error grows with T and with the magnitude of the running sum, so the grid's figure
# does not carry over), and its tolerance; the probabilities there stay inside PROB_TOL (measured 8.60e-7)
MEASURED_WORST_VIT_LONG = 8.681e-4
VIT_TOL_LONG = 4 * MEASURED_WORST_VIT_LONG
# one threshold per lexicon of LR.grid_lexicons (1, 3, 4, 5, 257 entries): 1.0 is reached by the only entry of a one-entry lexicon
# (its posterior is expf(0)), 0 never snaps, 1e-6 snaps wherever the line has a match at all (noise-only lines included: winners
# without a planted margin), and noise-only lines of the 3- and 257-entry lexicons stay below theirs
GRID_MIN_POST = (1.0, 0.9999, 0.0, 1e-6, 0.5)


# ---- the rule in fp64 ------------------------------------------------------------------------------------------------------
def states_of(entry):
    """(cls [S], skip [S]) of the entry's extended sequence"""
    S = 2 * len(entry) + 1
    cls = [entry[(s - 1) // 2] if s & 1 else 0 for s in range(S)]
    skip = [bool(s & 1 and s >= 3 and cls[s] != cls[s - 2]) for s in range(S)]
    return cls, skip


def viterbi64(l, entry):
    """The best alignment of the entry to one line's logits l [T][N] (fp64), T >= need(entry), by the rule's own recursion and
    tie order (stay, then s-1, then s-2; a later one only when strictly greater; end S-1 unless S-2 is strictly greater).
    Returns (optimum, path idx [T], second): second is the best value of any OTHER state path -- the maximum over lattice nodes
    (t, s) off the best path of fwd[t][s] + bwd[t][s]: every other path visits such a node, so this is exact (-inf: no other)."""
    T = l.shape[0]
    cls, skip = states_of(entry)
    S = len(cls)
    e = l[:, cls]                                           # [T][S]: the step's logit of each state
    ninf = -np.inf
    fwd = np.full((T, S), ninf); bp = np.zeros((T, S), np.int64)
    fwd[0, :2] = e[0, :2]
    for t in range(1, T):
        for s in range(S):
            b, o = fwd[t - 1, s], 0
            if s >= 1 and fwd[t - 1, s - 1] > b:
                b, o = fwd[t - 1, s - 1], 1
            if skip[s] and fwd[t - 1, s - 2] > b:
                b, o = fwd[t - 1, s - 2], 2
            fwd[t, s] = b + e[t, s]; bp[t, s] = o
    bwd = np.full((T, S), ninf)
    bwd[T - 1, S - 1] = bwd[T - 1, S - 2] = 0.0
    for t in range(T - 2, -1, -1):
        for s in range(S):
            b = bwd[t + 1, s] + e[t + 1, s]
            if s + 1 < S:
                b = max(b, bwd[t + 1, s + 1] + e[t + 1, s + 1])
            if s + 2 < S and skip[s + 2]:
                b = max(b, bwd[t + 1, s + 2] + e[t + 1, s + 2])
            bwd[t, s] = b
    s = S - 2 if fwd[T - 1, S - 2] > fwd[T - 1, S - 1] else S - 1
    opt = fwd[T - 1, s]
    on = np.zeros((T, S), bool); path = [0] * T
    for t in range(T - 1, -1, -1):
        on[t, s] = True; path[t] = cls[s]
        s -= bp[t, s]
    with np.errstate(invalid="ignore"):
        through = np.where(on, ninf, fwd + bwd)
    return float(opt), path, float(np.nanmax(np.where(np.isnan(through), ninf, through)))


def collapse(idx):
    """the greedy CTC decode of a class path: repeats merged, blanks dropped"""
    return [int(c) for t, c in enumerate(idx) if c != 0 and (t == 0 or c != idx[t - 1])]


def path_states(idx, entry):
    """the state sequence a class path implies (it is unique: from a token state the three successors have three different
    classes, from a blank the two have two), or None when some step is not a legal move of the entry's lattice"""
    cls, skip = states_of(entry)
    S = len(cls)
    out = []
    for t, c in enumerate(idx):
        if t == 0:
            cand = [s for s in (0, 1) if cls[s] == c]
        else:
            p = out[-1]
            cand = [s for s in (p, p + 1, p + 2) if s < S and cls[s] == c and (s - p < 2 or skip[s])]
        if not cand:
            return None
        out.append(cand[0])
    return out if out[-1] >= S - 2 else None


def fmt_tol(T, big):
    """What plain fp32 arithmetic may differ from fp64 by, from the number formats, for a line of T steps whose Viterbi value has
    magnitude up to `big`: each logit carries an error of about 3e-5 (120 products, ctc_lexicon_ref / test_lexicon_cpu.host_tol)
    and each of the T adds rounds at half an ulp of the running sum: (vit_tol, prob_tol).  A probability p = exp(l - lse) moves by
    at most p <= 1 times the error of (l - lse): two logit errors, an ulp of |l - lse| <= 64 and a few ulp of expf / logf."""
    return T * (3e-5 + 0.5 * float(np.spacing(np.float32(max(big, 1.0))))), 6e-5 + 4.0 * float(np.spacing(np.float32(64.0)))


# ---- marshalling -----------------------------------------------------------------------------------------------------------
def new_outputs(tpl, line_lex, lexicons):
    out = LR.new_outputs(tpl, line_lex, lexicons)
    rows = max(sum(tpl), 1)
    out.update(idx=np.full(rows, CANARY_IDX, np.int32), prob=np.full(rows, CANARY_F, np.float32),
               snapped=np.full(len(tpl), CANARY_IDX, np.int32), vit=np.full(len(tpl), CANARY_F, np.float32))
    return out


def call(fn, handle, z, W, b, tpl, line_lex, lexicons, min_post, chunk=None, want_table=True):
    """rt_debug_ctc_lexicon_align (handle, chunk given) or rt_debug_ctc_lexicon_align_host (handle None); returns (rc, outputs)"""
    N = W.shape[1]
    out = new_outputs(tpl, line_lex, lexicons)
    ids, lens, first = LR.flat_lexicons(lexicons)
    keep = [np.ascontiguousarray(a, t) for a, t in ((z, np.float32), (W, np.float32), (b, np.float32), (tpl, np.int32),
                                                     (line_lex, np.int32), (min_post, np.float32))]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(keep[0]), p(keep[1]), p(keep[2]), N, p(keep[3]), len(tpl), p(keep[4]), p(ids), p(lens), p(first), len(lexicons),
            p(keep[5])]
    if handle is not None:
        args = [handle] + args + [0 if chunk is None else chunk]
    args += [p(out["idx"]), p(out["prob"]), p(out["snapped"]), p(out["vit"]),
             p(out["table"]) if want_table else None, p(out["matches"]), p(out["n"])]
    return fn(*args), out


# ---- the checker -----------------------------------------------------------------------------------------------------------
def should_snap(out, i, k, min_post):
    """the snap condition, on the very fp32 values the call returned (margin-free: the rule is stated on them)"""
    if k == 0:
        return False
    mp = np.float32(min_post[k - 1])
    return bool(mp > 0 and out["n"][i] >= 1 and out["matches"][i][0]["posterior"] >= mp)


def check_align(out, l64, tpl, line_lex, lexicons, min_post, vit_tol, prob_tol, exact_logits=False, what=""):
    """Everything the snap half of a call must have produced, margin-free, no line left out; l64 [rows][N]: the fp64 logits of the
    same features.  A line snaps exactly where should_snap says.  Per snapped line: every idx[t] is 0 or a class of the entry (match
    0's); the greedy collapse of idx is the entry; the state sequence the path implies is monotone with legal steps, from state
    0 or 1 to S-2 or S-1; the path's fp64 score is at least the fp64 optimum - vit_tol; vit_out is within vit_tol of that
    score; prob[t] within prob_tol of the fp64 softmax; and where the fp64 gap between the best and the second-best path is at
    least 10 vit_tol -- or the caller vouches that the logits are exact in fp32 and their sums in fp64 (exact_logits: all-zero
    features), so that the fp64 recursion with the rule's tie order IS the rule -- the path equals the fp64 path.  Per unsnapped
    line of a lexicon: snapped == 0 and its rows and its vit slot still hold the canaries bit for bit; a line of lexicon 0 keeps
    its snapped canary too.  Returns (worst Viterbi deviation, worst |prob - fp64|, number of snapped lines, number of lines
    held to the exact path)."""
    lp64 = LR.logp64(l64) if sum(tpl) else l64
    worst_v = worst_p = 0.0
    n_snapped = n_exact = 0
    o = 0
    for i, (T, k) in enumerate(zip(tpl, line_lex)):
        w = (what, "line", i, "T", T, "lexicon", k)
        idx, prob = out["idx"][o:o + T], out["prob"][o:o + T]
        fire = should_snap(out, i, k, min_post)
        if not fire:
            assert int(out["snapped"][i]) == (0 if k > 0 else CANARY_IDX), (w, "snapped flag", int(out["snapped"][i]))
            assert (idx == CANARY_IDX).all() and prob.tobytes() == np.full(T, CANARY_F, np.float32).tobytes(), (w, "rows of an unsnapped line written")
            assert out["vit"][i].tobytes() == CANARY_F.tobytes(), (w, "vit of an unsnapped line written")
            o += T
            continue
        n_snapped += 1
        assert int(out["snapped"][i]) == 1, (w, "snapped flag", int(out["snapped"][i]))
        entry = lexicons[k - 1][int(out["matches"][i][0]["entry"])]
        assert T >= LR.need(entry), (w, "an infeasible entry was aligned")
        assert set(int(c) for c in idx) <= set(entry) | {0}, (w, "classes outside the entry", idx.tolist())
        assert collapse(idx) == list(entry), (w, "collapse", collapse(idx), entry)
        assert path_states(idx.tolist(), entry) is not None, (w, "illegal state sequence", idx.tolist())
        l = l64[o:o + T]
        opt, path, second = viterbi64(l, entry)
        score = float(sum(l[t, idx[t]] for t in range(T)))
        dv = max(opt - score, abs(float(out["vit"][i]) - score))
        worst_v = max(worst_v, dv)
        assert score >= opt - vit_tol, (w, "path score below the optimum", score, opt, vit_tol)
        assert abs(float(out["vit"][i]) - score) <= vit_tol, (w, "vit_out", float(out["vit"][i]), score, vit_tol)
        dp = float(np.abs(prob.astype(np.float64) - np.exp(lp64[o + np.arange(T), idx])).max())
        worst_p = max(worst_p, dp)
        assert dp <= prob_tol, (w, "prob", dp, prob_tol)
        if exact_logits or opt - second >= 10 * vit_tol:
            n_exact += 1
            assert idx.tolist() == path, (w, "path", idx.tolist(), path, opt - second)
        o += T
    return worst_v, worst_p, n_snapped, n_exact


def figures(out, l64, tpl, line_lex, lexicons, min_post):
    """(worst Viterbi deviation, worst |prob - fp64|) over the lines that should have snapped, without asserting anything: what a
    test prints before it checks, and what the MEASURED_* constants above were read from"""
    lp64 = LR.logp64(l64) if sum(tpl) else l64
    wv = wp = 0.0
    o = 0
    for i, (T, k) in enumerate(zip(tpl, line_lex)):
        idx = out["idx"][o:o + T]
        if should_snap(out, i, k, min_post) and ((idx >= 0) & (idx < l64.shape[1])).all():
            entry = lexicons[k - 1][int(out["matches"][i][0]["entry"])]
            opt = viterbi64(l64[o:o + T], entry)[0]
            score = float(sum(l64[o + t, idx[t]] for t in range(T)))
            wv = max(wv, opt - score, abs(float(out["vit"][i]) - score))
            wp = max(wp, float(np.abs(out["prob"][o:o + T].astype(np.float64) - np.exp(lp64[o + np.arange(T), idx])).max()))
        o += T
    return wv, wp


# ---- a float32 stand-in of the whole hook, and its mutants --------------------------------------------------------------
def stand_in(z, W, b, tpl, line_lex, lexicons, min_post, mutant=None):
    """What a correct implementation returns (LR.stand_in for the lexicon half, the alignment in fp32 numpy), or -- mutant -- one
    of the wrong ones."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    N = W.shape[1]
    out = new_outputs(tpl, line_lex, lexicons)
    out.update(LR.stand_in(z, W, b, tpl, line_lex, lexicons))
    l = (np.asarray(z, f) @ np.asarray(W, f) + np.asarray(b, f)).astype(f)
    lcols = np.concatenate([l, np.zeros((len(l), -N % 4), f)], axis=1) if mutant == "pad_columns_in_lse" else l
    mx = lcols.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(lcols - mx).sum(axis=1, keepdims=True, dtype=f))).astype(f)[:, 0]
    ninf = f(-np.inf)
    o = 0
    for i, (T, k) in enumerate(zip(tpl, line_lex)):
        if k == 0:
            o += T
            continue
        fire = should_snap(out, i, k, min_post)
        out["snapped"][i] = 1 if fire else 0
        if not fire and not (mutant == "written_below_threshold" and out["n"][i] >= 1):
            o += T
            continue
        entry = lexicons[k - 1][int(out["matches"][i][0]["entry"])]
        cls, skip = states_of(entry)
        if mutant == "skip_across_equal":
            skip = [bool(s & 1 and s >= 3) for s in range(len(cls))]
        S = len(cls)
        v = [l[o][cls[s]] if s < 2 else ninf for s in range(S)]
        bp = np.zeros((T, S), np.int64)
        for t in range(1, T):
            nx = []
            for s in range(S):
                b0, off = v[s], 0
                if s >= 1 and (v[s - 1] >= b0 if mutant == "ties_to_previous_state" else v[s - 1] > b0):
                    b0, off = v[s - 1], 1
                if skip[s] and v[s - 2] > b0:
                    b0, off = v[s - 2], 2
                nx.append(f(b0 + l[o + t][cls[s]])); bp[t, s] = off
            v = nx
        s = S - 1 if mutant == "end_always_last_blank" or not v[S - 2] > v[S - 1] else S - 2
        out["vit"][i] = v[s]
        shift = T if mutant == "neighbour_rows_written" and o + 2 * T <= len(out["idx"]) else 0
        for t in range(T - 1, -1, -1):
            c = cls[s]
            out["idx"][o + shift + t] = c
            out["prob"][o + shift + t] = f(np.exp(l[o + t][c])) if mutant == "prob_over_raw_logits" else f(np.exp(f(l[o + t][c] - lse[o + t])))
            s = max(s - bp[t, s], 0)
        o += T
    return out

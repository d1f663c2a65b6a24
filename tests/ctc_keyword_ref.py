"""numpy fp64 restatement of the rec keyword rule (retto_amd/csrc/ctc_keyword.h), a brute-force check of it over every class
path, hand-built tie cases, and the checkers the keyword tests share, with a float32 numpy stand-in of the whole hook whose
mutants the exact checker must refuse (test_keyword_cpu.py).  Nothing here decides what the library computes; call() only
marshals the arguments of rt_debug_ctc_keywords / rt_debug_ctc_keywords_host."""
import ctypes as C
import itertools

import numpy as np

import ctc_align_ref as AR
import ctc_lexicon_ref as LR

D = LR.D                     # SvtrCore::D: width of the CTC head's input features
HITS = 8                     # RT_KEYWORD_HITS
HIT = np.dtype([("entry", np.int32), ("score", np.float32), ("first_col", np.int32), ("last_col", np.int32),
                ("quad", np.float32, (8,))])   # rt_keyword_hit
CANARY_ENTRY = -7777         # what the tests put into the outputs before a call
CANARY_COL = -4242
CANARY_F = np.float32(-123.5)
MUTANTS = ("restart_on_tie", "skip_across_equal", "leading_blank", "latest_end", "threshold_ignored", "lse_for_rmax",
           "pad_columns_in_rmax", "ties_to_higher_entry")
# Worst deviation measured on the MI355X over the grid of test_gpu_keywords.py, both figures of check_grid() in one: |score_out
# - the fp64 value of the best alignment inside the returned span| and the fp64 optimum minus that value (that file's docstring
# has them per N), on the lines of up to 40 steps and on the line of 301 steps.
MEASURED_WORST = 1.297e-4
MEASURED_WORST_LONG = 7.050e-5
# The tolerances start as the project's own, ctc_align_ref.VIT_TOL (3.13e-4) up to 40 steps and VIT_TOL_LONG (3.47e-3) beyond.
# On the short lines the device's worst passes a quarter of VIT_TOL (7.83e-5): the scores there are sums of up to 40 costs that
# reach several hundred in magnitude, where one fp32 rounding is 3e-5.  So that tolerance is not taken over and not widened by
# eye: the plain fp32 loops of rt_debug_ctc_keywords_host were measured against fp64 on the same grid (1.087e-4 at N = 5,
# 1.092e-4 at N = 65, 1.094e-4 at N = 6625; test_keyword_cpu.test_host_rule_on_the_grid_against_fp64 measures them again), and
# the tolerance is 4 x that figure, the project's margin.  The long line's worst is below a quarter of VIT_TOL_LONG, which stands.
HOST_WORST = 1.094e-4
TOL = 4 * HOST_WORST
TOL_LONG = AR.VIT_TOL_LONG


def tol_of(T):
    return TOL if T <= 40 else TOL_LONG


# ---- the rule in fp64 ------------------------------------------------------------------------------------------------------
def cost64(z, W, b):
    """d[t][c] = l[t][c] - max_c l[t][c] of the fp64 logits, per row"""
    l = LR.logits64(z, W, b)
    return l - l.max(axis=1, keepdims=True)


def _tables(entries):
    E, S = len(entries), 2 * max(len(e) for e in entries) - 1
    cls = np.zeros((E, S), np.int64); valid = np.zeros((E, S), bool); skip = np.zeros((E, S), bool)
    for i, e in enumerate(entries):
        valid[i, :2 * len(e) - 1] = True
        for s in range(0, 2 * len(e) - 1, 2):
            cls[i, s] = e[s // 2]
            skip[i, s] = s >= 2 and e[s // 2] != e[s // 2 - 1]
    return cls, valid, skip, np.array([2 * len(e) - 2 for e in entries])


def spot64(d, entries, windows=None):
    """The rule over one line's costs d [T][N] (fp64), all entries advancing together: (score [E], first_col [E], last_col [E]);
    -inf and (-1, -1) where infeasible.  windows = (a [E], b [E]): instead, per entry the value of the best alignment that starts
    in state 0 at frame a and ends in state 2 L - 2 at frame b, every frame outside at cost 0 (no restart, one end); -inf where
    the window is (-1, -1) or too short."""
    T, E = d.shape[0], len(entries)
    score = np.full(E, -np.inf); first = np.full(E, -1, np.int64); last = np.full(E, -1, np.int64)
    if T == 0:
        return score, first, last
    cls, valid, skip, end = _tables(entries)
    S = cls.shape[1]
    rows = np.arange(E)
    ninf = np.full((E, 1), -np.inf); neg1 = np.full((E, 1), -1, np.int64)
    v = np.full((E, S), -np.inf); a = np.full((E, S), -1, np.int64)
    wa, wb = (np.asarray(windows[0]), np.asarray(windows[1])) if windows is not None else (None, None)
    for t in range(T):
        dt = d[t][cls]
        bv, ba = v.copy(), a.copy()
        if windows is None and t > 0:
            r = ~(bv[:, 0] >= 0.0)
            bv[r, 0] = 0.0; ba[r, 0] = t
        p1v = np.concatenate([ninf, v[:, :-1]], axis=1); p1a = np.concatenate([neg1, a[:, :-1]], axis=1)
        take = p1v > bv
        take[:, 0] = False
        bv = np.where(take, p1v, bv); ba = np.where(take, p1a, ba)
        p2v = np.concatenate([ninf, ninf, v[:, :-2]], axis=1) if S >= 2 else ninf
        p2a = np.concatenate([neg1, neg1, a[:, :-2]], axis=1) if S >= 2 else neg1
        take = skip & (p2v > bv)
        bv = np.where(take, p2v, bv); ba = np.where(take, p2a, ba)
        nv, na = dt + bv, ba
        start = np.full(E, t == 0) if windows is None else wa == t
        nv[start] = -np.inf; na[start] = -1
        nv[start, 0] = dt[start, 0]; na[start, 0] = t
        nv[~valid] = -np.inf; na[~valid] = -1
        v, a = nv, na
        ev = v[rows, end]
        better = ev > score if windows is None else wb == t
        score = np.where(better, ev, score); first = np.where(better, a[rows, end], first); last = np.where(better, t, last)
    feas = np.array([T >= LR.need(e) for e in entries])
    if windows is not None:
        feas &= wa >= 0
    score[~feas] = -np.inf; first[~feas] = -1; last[~feas] = -1
    return score, first, last


_PATHS = {}


def brute(d, entry):
    """the definition: the largest sum of per-step costs over every class path of length T whose collapsed string (repeats
    merged, blanks dropped) contains the entry as a substring; -inf when there is none"""
    T, N = d.shape
    if (N, T) not in _PATHS:
        paths = np.array(list(itertools.product(range(N), repeat=T)), np.int64).reshape(-1, T)
        col = [tuple(c for t, c in enumerate(p) if c != 0 and (t == 0 or c != p[t - 1])) for p in paths]
        _PATHS[(N, T)] = (paths, col)
    paths, col = _PATHS[(N, T)]
    e, L = tuple(entry), len(entry)
    has = np.array([any(c[i:i + L] == e for i in range(len(c) - L + 1)) for c in col], bool)
    if not has.any():
        return -np.inf
    return float(d[np.arange(T), paths].sum(axis=1)[has].max())


def top_hits(score, min_score, flip=False):
    """the entries of a score row that pass min_score, best first: by score descending, then entry index ascending"""
    ok = [e for e in range(len(score)) if score[e] > -np.inf and score[e] >= min_score]
    return sorted(ok, key=lambda e: (-float(score[e]), -e if flip else e))[:HITS]


# ---- marshalling -----------------------------------------------------------------------------------------------------------
def new_outputs(tpl, line_kw, lists):
    table = sum(len(lists[k - 1]) for k in line_kw if 0 < k <= len(lists))
    h = np.zeros((len(tpl), HITS), HIT)
    h["entry"] = CANARY_ENTRY; h["score"] = CANARY_F; h["first_col"] = CANARY_COL; h["last_col"] = CANARY_COL; h["quad"] = CANARY_F
    return {"score": np.full(max(table, 1), CANARY_F, np.float32), "span": np.full((max(table, 1), 2), CANARY_COL, np.int32),
            "hits": h, "n": np.full(len(tpl), -1, np.int32)}


def split_rows(out, line_kw, lists):
    """the flat tables as (score row, span rows) per line (None for a line of list 0)"""
    rows, o = [], 0
    for k in line_kw:
        n = len(lists[k - 1]) if k > 0 else 0
        rows.append((out["score"][o:o + n], out["span"][o:o + n]) if k > 0 else None)
        o += n
    return rows


def call(fn, handle, z, W, b, tpl, line_kw, lists, mins, chunk=None):
    """rt_debug_ctc_keywords (handle, chunk given) or rt_debug_ctc_keywords_host (handle None); returns (rc, outputs)"""
    N = W.shape[1]
    out = new_outputs(tpl, line_kw, lists)
    ids, lens, first = LR.flat_lexicons(lists)
    keep = [np.ascontiguousarray(a, t) for a, t in ((z, np.float32), (W, np.float32), (b, np.float32), (tpl, np.int32),
                                                     (line_kw, np.int32), (mins, np.float32))]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(keep[0]), p(keep[1]), p(keep[2]), N, p(keep[3]), len(tpl), p(keep[4]), p(ids), p(lens), p(first), len(lists), p(keep[5])]
    if handle is not None:
        args = [handle] + args + [0 if chunk is None else chunk]
    args += [p(out["score"]), p(out["span"]), p(out["hits"]), p(out["n"])]
    return fn(*args), out


# ---- the checkers ----------------------------------------------------------------------------------------------------------
def check_hits(out, tpl, line_kw, lists, mins, what=""):
    """The hits are the top HITS of the RETURNED table under the rule, exactly: entries, order, the table's very bits, the table's
    spans; canaries in the slots past the count, in every quad, and in everything of a line of list 0."""
    for i, (k, row) in enumerate(zip(line_kw, split_rows(out, line_kw, lists))):
        h, n = out["hits"][i], int(out["n"][i])
        w = (what, "line", i, "T", tpl[i])
        assert (h["quad"] == CANARY_F).all(), (w, "a quad was written")
        if k == 0:
            assert n == 0 and (h["entry"] == CANARY_ENTRY).all() and (h["score"] == CANARY_F).all() and \
                (h["first_col"] == CANARY_COL).all() and (h["last_col"] == CANARY_COL).all(), (w, "list 0 touched")
            continue
        score, span = row
        want = top_hits(score, mins[k - 1])
        assert n == len(want) and [int(e) for e in h["entry"][:n]] == want, (w, "hits", n, h["entry"][:n], want)
        for j, e in enumerate(want):
            assert h["score"][j].tobytes() == score[e].tobytes(), (w, "hit", j, "is not the table's score")
            assert (int(h["first_col"][j]), int(h["last_col"][j])) == tuple(int(x) for x in span[e]), (w, "hit", j, "span")
        assert (h["entry"][n:] == CANARY_ENTRY).all() and (h["score"][n:] == CANARY_F).all() and \
            (h["first_col"][n:] == CANARY_COL).all() and (h["last_col"][n:] == CANARY_COL).all(), (w, "slots past the count")


def check_grid(out, z, W, b, tpl, line_kw, lists, mins, tol_of, what=""):
    """Margin-free against fp64, no line and no entry left out.  For every (line, entry): an infeasible entry gives -inf and
    (-1, -1); otherwise the span is ordered and inside the line, the fp64 value of the best alignment confined to the returned
    span is within tol of score_out, and the fp64 optimum minus that value is <= tol (tol = tol_of(T)).  Then check_hits().
    Returns {T: (worst |score - confined|, worst optimum - confined)}."""
    d = cost64(z, W, b) if sum(tpl) else np.zeros((0, W.shape[1]))
    worst, o = {}, 0
    for i, (T, k, row) in enumerate(zip(tpl, line_kw, split_rows(out, line_kw, lists))):
        if k > 0:
            lst, (score, span), tol = lists[k - 1], row, tol_of(T)
            w = (what, "line", i, "T", T)
            feas = np.array([T >= LR.need(e) for e in lst])
            assert not np.isnan(score).any(), (w, "NaN in the table")
            assert np.array_equal(np.isneginf(score), ~feas), (w, "-inf exactly where infeasible")
            assert (span[~feas] == -1).all(), (w, "an infeasible entry has a span")
            f, l = span[:, 0].astype(np.int64), span[:, 1].astype(np.int64)
            assert ((0 <= f[feas]) & (f[feas] <= l[feas]) & (l[feas] < T)).all(), (w, "a span outside the line")
            if feas.any():
                opt, _, _ = spot64(d[o:o + T], lst)
                conf, _, _ = spot64(d[o:o + T], lst, windows=(np.where(feas, f, -1), np.where(feas, l, -1)))
                assert np.isfinite(conf[feas]).all(), (w, "no alignment fits the returned span", np.flatnonzero(feas & ~np.isfinite(conf))[:8])
                e1 = np.abs(score[feas].astype(np.float64) - conf[feas]); e2 = opt[feas] - conf[feas]
                assert e1.max() <= tol, (w, "score against its span", int(np.flatnonzero(feas)[e1.argmax()]), float(e1.max()), tol)
                assert e2.max() <= tol, (w, "span against the optimum", int(np.flatnonzero(feas)[e2.argmax()]), float(e2.max()), tol)
                pw = worst.get(T, (0.0, 0.0))
                worst[T] = (max(pw[0], float(e1.max())), max(pw[1], float(e2.max())))
        o += T
    check_hits(out, tpl, line_kw, lists, mins, what)
    return worst


def same(a, b):
    """two outputs agree bit for bit: tables, spans, hits (quads included), counts"""
    return all(a[k].tobytes() == b[k].tobytes() for k in ("score", "span", "hits", "n"))


# ---- a float32 stand-in of the whole hook, and its mutants ----------------------------------------------------------------
def stand_in(z, W, b, tpl, line_kw, lists, mins, mutant=None):
    """What a correct implementation returns (fp32 logits, the recursion in fp32 scalars), or -- mutant -- one of the wrong ones."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    N = W.shape[1]
    out = new_outputs(tpl, line_kw, lists)
    l = (np.asarray(z, f) @ np.asarray(W, f) + np.asarray(b, f)).astype(f)
    lcols = np.concatenate([l, np.zeros((len(l), -N % 4), f)], axis=1) if mutant == "pad_columns_in_rmax" else l
    mx = lcols.max(axis=1, keepdims=True)
    if mutant == "lse_for_rmax":
        mx = (mx + np.log(np.exp(lcols - mx).sum(axis=1, keepdims=True, dtype=f))).astype(f)
    d = (l - mx).astype(f)
    NINF = (f(-np.inf), -1)
    o = oo = 0
    for i, (T, k) in enumerate(zip(tpl, line_kw)):
        if k == 0:
            out["n"][i] = 0
            o += T
            continue
        lst = lists[k - 1]
        for ei, e in enumerate(lst):
            res = (f(-np.inf), -1, -1)
            ext = [e[s // 2] if s % 2 == 0 else 0 for s in range(2 * len(e) - 1)]
            if mutant == "leading_blank":
                ext = [0] + ext
            S = len(ext)
            tok = lambda s: ext[s] != 0
            if T >= LR.need(e):
                st = []
                for t in range(T):
                    nx = []
                    for s in range(S):
                        dd = d[o + t][ext[s]]
                        if t == 0:
                            nx.append((dd, 0) if s == 0 else NINF)
                            continue
                        best = st[s]
                        if s == 0:
                            if not (best[0] > 0 if mutant == "restart_on_tie" else best[0] >= 0):
                                best = (f(0.0), t)
                        else:
                            if st[s - 1][0] > best[0]:
                                best = st[s - 1]
                            sk = tok(s) and s >= 2 and tok(s - 2) and (mutant == "skip_across_equal" or ext[s] != ext[s - 2])
                            if sk and st[s - 2][0] > best[0]:
                                best = st[s - 2]
                        nx.append((f(dd + best[0]), best[1]))
                    st = nx
                    if st[S - 1][0] > res[0] or (mutant == "latest_end" and st[S - 1][0] == res[0] and res[0] > -np.inf):
                        res = (st[S - 1][0], st[S - 1][1], t)
            out["score"][oo + ei] = res[0]; out["span"][oo + ei] = res[1:]
        row = out["score"][oo:oo + len(lst)]
        want = top_hits(row, -np.inf if mutant == "threshold_ignored" else mins[k - 1], flip=mutant == "ties_to_higher_entry")
        for j, e in enumerate(want):
            h = out["hits"][i][j]
            h["entry"] = e; h["score"] = row[e]; h["first_col"], h["last_col"] = out["span"][oo + e]
        out["n"][i] = len(want)
        o += T; oo += len(lst)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def exact_inputs(rows, N):
    """(z, W, b) whose fp32 logits are the given integer rows [.][N], bit for bit, whatever the summation order: feature c of a
    row IS its logit of class c, W picks it out, the bias is zero"""
    rows = np.asarray(rows, np.float32).reshape(-1, N)
    z = np.zeros((max(len(rows), 1), D), np.float32); z[:len(rows), :N] = rows
    W = np.zeros((D, N), np.float32); W[np.arange(N), np.arange(N)] = 1.0
    return z, W, np.zeros(N, np.float32)


def case(lines, N, lists, mins):
    """one exact case: lines = [(integer logit rows [T][N], list id)], as the arguments of call()"""
    z, W, b = exact_inputs(np.concatenate([np.asarray(r, np.float32).reshape(-1, N) for r, _ in lines] + [np.zeros((0, N), np.float32)]), N)
    return z, W, b, [len(np.asarray(r).reshape(-1, N)) for r, _ in lines], [k for _, k in lines], lists, list(mins)


def expected(z, W, b, tpl, line_kw, lists, mins):
    """what the rule gives for an exact case, from the fp64 restatement (integers: every fp32 sum is exact, so bit for bit)"""
    out = new_outputs(tpl, line_kw, lists)
    d = cost64(z, W, b)
    o = oo = 0
    for i, (T, k) in enumerate(zip(tpl, line_kw)):
        if k == 0:
            out["n"][i] = 0
        else:
            lst = lists[k - 1]
            sc, fi, la = spot64(d[o:o + T], lst)
            out["score"][oo:oo + len(lst)] = sc; out["span"][oo:oo + len(lst), 0] = fi; out["span"][oo:oo + len(lst), 1] = la
            want = top_hits(out["score"][oo:oo + len(lst)], mins[k - 1])
            for j, e in enumerate(want):
                h = out["hits"][i][j]
                h["entry"] = e; h["score"] = sc[e]; h["first_col"] = fi[e]; h["last_col"] = la[e]
            out["n"][i] = len(want)
            oo += len(lst)
        o += T
    return out


# Hand-built tie cases: (name, logit rows [T][N] as integers, entry, (score, first_col, last_col)).  Column 0 is the blank; the
# last column is a filler class that holds the row maximum 0 wherever no class of the entry does, so a row IS its costs.
_F = 0
KNOWN = (
    # L = 1: the best frame wins, and among equal ones the first (t = 2 restarts to the same -1, not strictly greater)
    ("L1", [[-9, -9, -3, _F], [-9, -9, -1, _F], [-9, -9, -1, _F]], [2], (-1.0, 1, 1)),
    # start tie: state 0 sits at 0 since frame 0; restarting at frame 1 would tie, the earlier start stays
    ("start_tie", [[-9, 0, -9, _F], [-9, 0, -5, _F], [-9, -9, 0, _F]], [1, 2], (0.0, 0, 2)),
    # end tie: frames 0 and 2 both end the entry at 0; the earliest end stays
    ("end_tie", [[-9, 0, -9, _F], [-9, -4, 0, _F], [-9, 0, -9, _F]], [1], (0.0, 0, 0)),
    # stay vs enter: at frame 2 state 2 holds (-1, start 0) and state 0 offers (-1, start 1): the tie stays, the start is 0
    ("stay_vs_enter", [[-9, -1, -9, -9, _F], [-9, -1, 0, -9, _F], [-9, -9, 0, -9, _F], [-9, -9, -9, 0, _F]], [1, 2, 3], (-1.0, 0, 3)),
    # equal neighbours need the blank between them: 1 1 1 reads as ONE token, the second needs frame 1 to be the blank at -2
    ("equal_neighbours", [[-2, 0, _F], [-2, 0, _F], [-2, 0, _F]], [1, 1], (-2.0, 0, 2)),
    # ... and two frames cannot hold them at all
    ("equal_neighbours_infeasible", [[-2, 0, _F], [-2, 0, _F]], [1, 1], (-np.inf, -1, -1)),
    # a skip is taken where the neighbours differ: no blank frame needed
    ("skip", [[-7, 0, -9, _F], [-7, -9, 0, _F]], [1, 2], (0.0, 0, 1)),
)


def known_case(rows, entry):
    return case([(rows, 1)], len(rows[0]), [[list(entry)]], [-np.inf])


def small_cases(n, seed=77):
    """n random exact cases for the brute force: N <= 4 classes, T <= 6 steps, lists of 1..4 entries of L <= 3 (equal neighbours
    included), every logit a negative integer (so a pad column of 0 would be the row maximum)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        N = int(rng.integers(2, 5))
        lst = []
        for _ in range(int(rng.integers(1, 5))):
            e = [int(rng.integers(1, N))]
            for _ in range(int(rng.integers(0, 3))):
                e.append(e[-1] if rng.random() < 0.3 else int(rng.integers(1, N)))
            lst.append(e)
        lines = [(rng.integers(-4, 0, (int(rng.integers(0, 7)), N)), 1) for _ in range(int(rng.integers(1, 3)))]
        out.append(case(lines, N, [lst], [[-np.inf, -np.inf, -3.0, 0.0][int(rng.integers(0, 4))]]))
    return out


def planted_rows(rng, W, T, path, at, gain=4.0, noise=1.5):
    """features of one line of T steps of noise with the class path `path` planted from step `at` on, by
    ctc_lexicon_ref.planted_features' formula"""
    z = rng.normal(0.0, noise, (T, D))
    for j, c in enumerate(path):
        z[at + j] += gain * W[:, c] / np.linalg.norm(W[:, c]) * np.sqrt(D) / 4.0
    return np.clip(z, -20.0, 20.0).astype(np.float32)


def grid_case(N):
    """inputs of the N-grid of test_gpu_keywords.py: (z, W, b, tokens_per_line, line_kw, lists, mins).  The lists are
    ctc_lexicon_ref.grid_lexicons (entry lengths GRID_LENS, sizes GRID_COUNTS); per list, lines of T = 1, need - 1, need and 40
    for its longest entry, planted (ctc_lexicon_ref.grid_case's gain) where it fits; a line without a list after every third
    line; one line of 301 steps at the end."""
    rng = np.random.default_rng(9300 + N)
    W = (rng.normal(0.0, 1.0, (D, N)) * np.sqrt(2.0 / D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    lists = LR.grid_lexicons(rng, N)
    mins = [-np.inf, -30.0, -np.inf, -2.0, -np.inf]
    W64 = W.astype(np.float64)
    tpl, line_kw, rows = [], [], []

    def add(T, k, path=None):
        tpl.append(T); line_kw.append(k)
        rows.append(planted_rows(rng, W64, T, path or [], 0))
        if len(tpl) % 4 == 3:
            tpl.append(9); line_kw.append(0); rows.append(planted_rows(rng, W64, 9, [], 0))

    for k, lst in enumerate(lists):
        e = max(lst, key=len)
        nd = LR.need(e)
        for T in (1, nd - 1, nd, 40):
            add(T, k + 1, LR.alignment(e, T) if T >= nd else None)
    add(301, len(lists), None)
    return np.concatenate(rows), W, b, tpl, line_kw, lists, mins

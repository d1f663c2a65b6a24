"""numpy fp64 restatement of the rec lexicon rule (retto_amd/csrc/ctc_lexicon.h), a brute-force check of it, and the checker the
lexicon tests share, with a float32 numpy stand-in of the whole hook whose mutants the checker must refuse (test_lexicon_cpu.py).
Nothing here decides what the library computes; call() only marshals the arguments of rt_debug_ctc_lexicon /
rt_debug_ctc_lexicon_host."""
import ctypes as C
import itertools

import numpy as np

D = 120                      # SvtrCore::D: width of the CTC head's input features
MATCHES = 4                  # RT_LEXICON_MATCHES
MAX_LEN = 31                 # RT_LEXICON_MAX_LEN
MATCH = np.dtype([("entry", np.int32), ("loglik", np.float32), ("posterior", np.float32)])   # rt_lexicon_match
CANARY_ENTRY = -7777         # what the tests put into the outputs before a call
CANARY_F = np.float32(-123.5)
MUTANTS = ("skip_across_equal", "final_blank_forgotten", "lse_dropped", "pad_columns_in_lse", "infeasible_reported",
           "ties_to_higher_index")
# Worst |loglik - fp64| and |posterior - fp64| measured on the MI355X over the grid of test_gpu_lexicon.py (that file's docstring
# has the figures per N).  Each tolerance is 4 x its own figure, the convention of test_gpu_candidates.py / test_gpu_charset.py.
MEASURED_WORST_LL = 1.851e-4
MEASURED_WORST_POST = 1.185e-5
HOOK_TOL = 4 * MEASURED_WORST_LL
HOOK_PTOL = 4 * MEASURED_WORST_POST
GRID_N = (5, 65, 6625)
GRID_LENS = (1, 7, 8, 15, 16, 31)      # the bucket edges: 16 lanes up to 7, 32 up to 15, 64 up to 31
GRID_COUNTS = (1, 3, 4, 5, 257)        # one entry, a partial wave, exactly 4 per wave, one past it, many waves of every bucket


# ---- the rule in fp64 ------------------------------------------------------------------------------------------------------
def logits64(z, W, b):
    l = np.asarray(z, np.float64) @ np.asarray(W, np.float64)
    return l if b is None else l + np.asarray(b, np.float64)


def logp64(l):
    """log-softmax over every class, per row"""
    m = l.max(axis=1, keepdims=True)
    return l - (m + np.log(np.exp(l - m).sum(axis=1, keepdims=True)))


def need(entry):
    """the fewest time steps an entry fits into: its length plus its number of equal neighbours"""
    return len(entry) + sum(1 for a, b in zip(entry[1:], entry[:-1]) if a == b)


def _lse(x, axis=None):
    x = np.asarray(x, np.float64)
    m = np.max(x, axis=axis, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(np.isneginf(m), -np.inf, m + np.log(np.exp(x - np.where(np.isneginf(m), 0.0, m)).sum(axis=axis, keepdims=True)))
    return r.reshape(()) if axis is None else np.squeeze(r, axis=axis)


def loglik64(lp, entries):
    """CTC forward log-likelihood of every entry over one line's log-probabilities lp [T][N] (fp64); -inf where infeasible.
    All entries advance together: alpha [E][S_max], states past an entry's S = 2 L + 1 stay -inf."""
    T, E = lp.shape[0], len(entries)
    out = np.full(E, -np.inf)
    if T == 0:
        return out
    S_max = 2 * max(len(e) for e in entries) + 1
    cls = np.zeros((E, S_max), np.int64); valid = np.zeros((E, S_max), bool); skip = np.zeros((E, S_max), bool)
    for i, e in enumerate(entries):
        S = 2 * len(e) + 1
        valid[i, :S] = True
        for s in range(1, S, 2):
            cls[i, s] = e[(s - 1) // 2]
            skip[i, s] = s >= 3 and e[(s - 1) // 2] != e[(s - 3) // 2]
    ninf = np.full((E, 1), -np.inf)
    a = np.full((E, S_max), -np.inf)
    a[:, :2] = lp[0][cls[:, :2]]
    a[~valid] = -np.inf
    for t in range(1, T):
        a1 = np.concatenate([ninf, a[:, :-1]], axis=1)
        a2 = np.where(skip, np.concatenate([ninf, ninf, a[:, :-2]], axis=1), -np.inf)
        a = np.logaddexp(np.logaddexp(a, a1), a2) + lp[t][cls]
        a[~valid] = -np.inf
    for i, e in enumerate(entries):
        S = 2 * len(e) + 1
        out[i] = np.logaddexp(a[i, S - 1], a[i, S - 2]) if T >= need(e) else -np.inf
    return out


def brute64(lp, entry):
    """the definition: log of the sum, over every class path of length T that collapses to the entry (repeats merged, blanks
    dropped), of the product of its per-step probabilities"""
    T, N = lp.shape
    terms = []
    for path in itertools.product(range(N), repeat=T):
        col = [c for t, c in enumerate(path) if c != 0 and (t == 0 or c != path[t - 1])]
        if col == list(entry):
            terms.append(sum(lp[t, c] for t, c in enumerate(path)))
    return float(_lse(terms)) if terms else -np.inf


def reference(z, W, b, tpl, line_lex, lexicons):
    """per line None (lexicon 0) or (loglik64 [n], posterior64 [n]) of its lexicon's entries, from the fp64 logits of the same
    features; posterior 0 where infeasible"""
    lp = logp64(logits64(z, W, b)) if sum(tpl) else np.zeros((0, W.shape[1]))
    ref, o = [], 0
    for T, k in zip(tpl, line_lex):
        if k > 0:
            ll = loglik64(lp[o:o + T], lexicons[k - 1])
            with np.errstate(invalid="ignore"):
                post = np.where(np.isneginf(ll), 0.0, np.exp(ll - _lse(ll))) if np.isfinite(ll).any() else np.zeros(len(ll))
            ref.append((ll, post))
        else:
            ref.append(None)
        o += T
    return ref


def top2_gap(ll):
    """fp64 gap between the two best entries of a line (inf with fewer than two feasible ones)"""
    f = np.sort(ll[np.isfinite(ll)])
    return float(f[-1] - f[-2]) if len(f) >= 2 else np.inf


# ---- marshalling -----------------------------------------------------------------------------------------------------------
def flat_lexicons(lexicons):
    ids = [c for lex in lexicons for e in lex for c in e]
    lens = [len(e) for lex in lexicons for e in lex]
    first = np.concatenate([[0], np.cumsum([len(lex) for lex in lexicons])])
    return np.array(ids, np.int32), np.array(lens, np.int32), first.astype(np.int32)


def new_outputs(tpl, line_lex, lexicons):
    table = sum(len(lexicons[k - 1]) for k in line_lex if 0 < k <= len(lexicons))
    m = np.empty((len(tpl), MATCHES), MATCH)
    m["entry"] = CANARY_ENTRY; m["loglik"] = CANARY_F; m["posterior"] = CANARY_F
    return {"table": np.full(max(table, 1), CANARY_F, np.float32), "matches": m, "n": np.full(len(tpl), -1, np.int32)}


def split_table(table, line_lex, lexicons):
    """the flat loglik table as one array per line (None for a line of lexicon 0)"""
    rows, o = [], 0
    for k in line_lex:
        n = len(lexicons[k - 1]) if k > 0 else 0
        rows.append(table[o:o + n] if k > 0 else None)
        o += n
    return rows


def call(fn, handle, z, W, b, tpl, line_lex, lexicons, chunk=None, want_table=True):
    """rt_debug_ctc_lexicon (handle, chunk given) or rt_debug_ctc_lexicon_host (handle None); returns (rc, outputs)"""
    N = W.shape[1]
    out = new_outputs(tpl, line_lex, lexicons)
    ids, lens, first = flat_lexicons(lexicons)
    keep = [np.ascontiguousarray(a, t) for a, t in ((z, np.float32), (W, np.float32), (b, np.float32), (tpl, np.int32),
                                                     (line_lex, np.int32))]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(keep[0]), p(keep[1]), p(keep[2]), N, p(keep[3]), len(tpl), p(keep[4]), p(ids), p(lens), p(first), len(lexicons)]
    if handle is not None:
        args = [handle] + args + [0 if chunk is None else chunk]
    args += [p(out["table"]) if want_table else None, p(out["matches"]), p(out["n"])]
    return fn(*args), out


# ---- the checker -----------------------------------------------------------------------------------------------------------
def check_outputs(out, ref, tpl, line_lex, lexicons, tol, ptol, what=""):
    """Everything a call must have produced, margin-free, no line and no entry left out.  Per line of a lexicon: every finite
    table entry within tol of fp64; -inf exactly where the entry is infeasible; the count min(MATCHES, feasible); each match's
    loglik within tol of its entry's fp64 value and, bit for bit, the table's value of that entry; logliks non-increasing, equal
    ones by ascending entry index; no entry twice; every unreported feasible entry has fp64 loglik <= the last reported + tol and,
    where the table gives it the last reported's very bits, a higher index; posteriors within ptol of fp64; canaries past the
    count.  A line of lexicon 0: count 0 and every match slot untouched.  Without a table (out["table"] None: the pipeline returns
    the matches only) the checks against the table fall away, the others stay.  Returns (worst |loglik - fp64|, worst |posterior
    - fp64|)."""
    rows = split_table(out["table"], line_lex, lexicons) if out["table"] is not None else [None] * len(tpl)
    worst_l = worst_p = 0.0
    for i, (T, k) in enumerate(zip(tpl, line_lex)):
        m, n = out["matches"][i], int(out["n"][i])
        w = (what, "line", i, "T", T)
        if k == 0:
            assert n == 0 and (m["entry"] == CANARY_ENTRY).all() and (m["loglik"] == CANARY_F).all(), (w, "lexicon 0 touched")
            continue
        lex, (ll, post), row = lexicons[k - 1], ref[i], rows[i]
        feas = np.array([T >= need(e) for e in lex])
        assert np.array_equal(np.isfinite(ll), feas), (w, "reference feasibility")
        if row is not None:
            assert np.array_equal(np.isneginf(row), ~feas), (w, "-inf exactly where infeasible", np.flatnonzero(np.isneginf(row) != ~feas)[:8])
            assert not np.isnan(row).any(), (w, "NaN in the table")
        if row is not None and feas.any():
            err = np.abs(row[feas].astype(np.float64) - ll[feas])
            worst_l = max(worst_l, float(err.max()))
            assert err.max() <= tol, (w, "table", int(np.flatnonzero(feas)[err.argmax()]), float(err.max()), tol)
        assert n == min(MATCHES, int(feas.sum())), (w, "count", n, int(feas.sum()))
        ent = [int(e) for e in m["entry"][:n]]
        assert len(set(ent)) == n and all(0 <= e < len(lex) and feas[e] for e in ent), (w, "entries", ent)
        for j in range(n):
            e = ent[j]
            assert row is None or m["loglik"][j].tobytes() == row[e].tobytes(), (w, "match", j, "is not the table's value")
            worst_l = max(worst_l, abs(float(m["loglik"][j]) - ll[e]))
            assert abs(float(m["loglik"][j]) - ll[e]) <= tol, (w, "match loglik", j, float(m["loglik"][j]), ll[e], tol)
            dp = abs(float(m["posterior"][j]) - post[e])
            worst_p = max(worst_p, dp)
            assert dp <= ptol, (w, "posterior", j, float(m["posterior"][j]), post[e], ptol)
            if j > 0:
                a, c = float(m["loglik"][j - 1]), float(m["loglik"][j])
                assert a > c or (a == c and ent[j - 1] < e), (w, "order", ent, m["loglik"][:n])
        assert (m["entry"][n:] == CANARY_ENTRY).all() and (m["loglik"][n:] == CANARY_F).all(), (w, "slots past the count")
        if n:
            last_e, last = ent[n - 1], m["loglik"][n - 1]
            for e in np.flatnonzero(feas):
                if int(e) in ent:
                    continue
                assert ll[e] <= float(last) + tol, (w, "left out", int(e), ll[e], float(last))
                assert row is None or not (row[e] > last or (row[e] == last and e < last_e)), (w, "left out against the table", int(e))
    return worst_l, worst_p


# ---- a float32 stand-in of the whole hook, and its mutants --------------------------------------------------------------
def stand_in(z, W, b, tpl, line_lex, lexicons, mutant=None):
    """What a correct implementation returns (fp32 logits, the recursion in fp32 numpy), or -- mutant -- one of the wrong ones."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    N = W.shape[1]
    out = new_outputs(tpl, line_lex, lexicons)
    l = (np.asarray(z, f) @ np.asarray(W, f) + np.asarray(b, f)).astype(f)
    lcols = np.concatenate([l, np.zeros((len(l), -N % 4), f)], axis=1) if mutant == "pad_columns_in_lse" else l
    mx = lcols.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(lcols - mx).sum(axis=1, keepdims=True, dtype=f))).astype(f)
    lp = l if mutant == "lse_dropped" else (l - lse).astype(f)

    def lae(*x):
        m = max(x)
        if m == -np.inf:
            return f(-np.inf)
        return f(m + np.log(f(sum(np.exp(f(v - m)) for v in x))))

    o = oo = 0
    for i, (T, k) in enumerate(zip(tpl, line_lex)):
        if k == 0:
            out["n"][i] = 0
            o += T
            continue
        lex = lexicons[k - 1]
        row = np.full(len(lex), -np.inf, f)
        for ei, e in enumerate(lex):
            S = 2 * len(e) + 1
            if T < need(e):
                if mutant == "infeasible_reported":
                    row[ei] = f(-60.0 - ei)
                continue
            cls = [e[(s - 1) // 2] if s & 1 else 0 for s in range(S)]
            a = [lp[o][cls[s]] if s < 2 else f(-np.inf) for s in range(S)]
            for t in range(1, T):
                nx = []
                for s in range(S):
                    skip = s & 1 and s >= 3 and (mutant == "skip_across_equal" or cls[s] != cls[s - 2])
                    nx.append(f(lae(a[s], a[s - 1] if s >= 1 else f(-np.inf), a[s - 2] if skip else f(-np.inf)) + lp[o + t][cls[s]]))
                a = nx
            row[ei] = a[S - 2] if mutant == "final_blank_forgotten" else lae(a[S - 1], a[S - 2], f(-np.inf))
        out["table"][oo:oo + len(lex)] = row
        fin = [ei for ei in range(len(lex)) if row[ei] > -np.inf]
        order = sorted(fin, key=lambda ei: (-row[ei], -ei if mutant == "ties_to_higher_index" else ei))[:MATCHES]
        if fin:
            m = max(row[ei] for ei in fin)
            tot = f(m + np.log(f(sum(np.exp(f(row[ei] - m)) for ei in fin))))
        for j, ei in enumerate(order):
            out["matches"][i][j] = (ei, row[ei], f(np.exp(f(row[ei] - tot))))
        out["n"][i] = len(order)
        o += T; oo += len(lex)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def random_entry(rng, N, L, max_need=40):
    """L class ids of [1, N); about one neighbour in five repeats; redrawn until the entry fits into max_need steps"""
    while True:
        e = [int(rng.integers(1, N))]
        for _ in range(L - 1):
            e.append(e[-1] if rng.random() < 0.2 else int(rng.integers(1, N)))
        if need(e) <= max_need:
            return e


def alignment(entry, T):
    """one class path of length T >= need(entry) that collapses to the entry: its tokens, a blank between equal neighbours, the
    last state repeated to the end"""
    path = []
    for j, c in enumerate(entry):
        if j > 0 and entry[j - 1] == c:
            path.append(0)
        path.append(c)
    assert len(path) <= T
    return path + [path[-1]] * (T - len(path))


def planted_features(rng, W, paths, gain=4.0, noise=1.5):
    """features of the lines whose class paths are given (None: noise only): each step leans toward its class's weight column,
    so that the fp64 likelihood of the planted entry stands clear of every other entry's"""
    rows = []
    for T, path in paths:
        z = rng.normal(0.0, noise, (T, D))
        if path is not None:
            for t, c in enumerate(path):
                z[t] += gain * W[:, c] / np.linalg.norm(W[:, c]) * np.sqrt(D) / 4.0
        rows.append(z)
    z = np.concatenate(rows) if rows else np.zeros((0, D))
    return np.clip(z, -20.0, 20.0).astype(np.float32) if len(z) else np.zeros((1, D), np.float32)


def grid_lexicons(rng, N):
    """one lexicon per count of GRID_COUNTS; between them their entry lengths are exactly GRID_LENS.  No entry twice in a lexicon
    (ties have their own test), so at most one one-token entry each: N = 5 has only four of them"""
    lens_of = {1: [7], 3: [1, 8, 31], 4: [7, 7, 1, 7], 5: [1, 7, 15, 16, 7],
               257: list(GRID_LENS) + [GRID_LENS[1 + i % 5] for i in range(251)]}
    lexicons = []
    for n in GRID_COUNTS:
        lex = []
        for L in lens_of[n]:
            e = random_entry(rng, N, L)
            while e in lex:
                e = random_entry(rng, N, L)
            lex.append(e)
        assert len(lex) == n
        lexicons.append(lex)
    assert sorted({len(e) for lex in lexicons for e in lex}) == list(GRID_LENS)
    return lexicons


def grid_case(N):
    """inputs of the N-grid of test_gpu_lexicon.py: (z, W, b, tokens_per_line, line_lex, lexicons).  Per lexicon its longest
    entry is planted on five lines of T = 1, L, L + pairs - 1 (infeasible), L + pairs, 40 steps (noise only where it does not fit)"""
    rng = np.random.default_rng(9100 + N)
    W = (rng.normal(0.0, 1.0, (D, N)) * np.sqrt(2.0 / D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    lexicons = grid_lexicons(rng, N)
    tpl, line_lex, paths = [], [], []
    for k, lex in enumerate(lexicons):
        e = max(lex, key=len)
        L, nd = len(e), need(e)
        for T in (1, L, nd - 1, nd, 40):
            tpl.append(T); line_lex.append(k + 1)
            paths.append((T, alignment(e, T) if T >= nd else None))
    z = planted_features(rng, W.astype(np.float64), paths)
    return z, W, b, tpl, line_lex, lexicons


def zero_feature_case(N, bias, T):
    """all-zero features: every logit is its bias, bit for bit"""
    rng = np.random.default_rng(N)
    W = (rng.normal(0.0, 1.0, (D, N)) * np.sqrt(2.0 / D)).astype(np.float32)
    return np.zeros((T, D), np.float32), W, np.asarray(bias, np.float32)

"""numpy fp64 restatement of the rec charset rule (retto_amd/csrc/ctc_charset.h) and the checker the charset tests share, with a
float32 numpy stand-in of the whole hook whose mutants the checker must refuse (test_charset_cpu.py).  Nothing here decides what
the library computes; call() only marshals the arguments of rt_debug_ctc_charset / rt_debug_ctc_charset_host."""
import ctypes as C

import numpy as np

import ctc_candidates_ref as R

CANARY_TOK = -4242          # what the tests put into tokens_out before a call
GRID_TPL = [40, 1, 80, 7, 33, 120]
GRID_LINE_SET = [1, 3, 2, 0, 0, 3]   # {blank, N - 1}, half the classes, 11 classes, none, none, half the classes
MUTANTS = ("mask_ignored", "blank_not_forced", "sum_over_all", "ties_to_higher_id", "pad_columns_admitted")


def mask_words(n_classes):
    return (n_classes + 31) // 32


def mask_of(ids, n_classes):
    """the mask words of a set of class ids (bit 0 is NOT forced here: the rule forces the blank, not the mask)"""
    m = np.zeros(mask_words(n_classes), np.uint32)
    for c in ids:
        m[int(c) >> 5] |= np.uint32(1) << np.uint32(int(c) & 31)
    return m


def members(mask, n_classes):
    """class ids of the set: the mask's bits below n_classes, and the blank"""
    return [c for c in range(n_classes) if c == 0 or (int(mask[c >> 5]) >> (c & 31)) & 1]


def logits64(z, W, b):
    l = np.asarray(z, np.float64) @ np.asarray(W, np.float64)
    return l if b is None else l + np.asarray(b, np.float64)


def masked_softmax64(l, S):
    """fp64 softmax of one row's logits over the classes S; 0 outside S"""
    q = np.zeros(len(l), np.float64)
    e = np.exp(l[S] - l[S].max())
    q[S] = e / e.sum()
    return q


def grid_sets(rng, N):
    """the three sets of the grid: {blank, N - 1}, 11 classes (all of them when N < 11), about half the classes"""
    s2 = sorted(rng.choice(N, min(11, N), replace=False).tolist())
    s3 = sorted(np.flatnonzero(rng.random(N) < 0.5).tolist())
    return np.stack([mask_of([N - 1], N), mask_of(s2, N), mask_of(s3, N)])


def grid_case(N):
    """inputs of the N-grid of test_gpu_charset.py: (z, W, b, idx, prob, tokens_per_line, line_set, masks)"""
    rng = np.random.default_rng(7000 + N)
    z, W, b, idx, prob = R.make_case(rng, N, GRID_TPL)
    return z, W, b, idx, prob, GRID_TPL, GRID_LINE_SET, grid_sets(rng, N)


def min_top2_gap(z, W, b, tpl, line_set, masks):
    """smallest fp64 gap between the two largest allowed logits over the restricted rows (inf when a set has one class)"""
    l = logits64(z, W, b)
    N, gap, o = l.shape[1], np.inf, 0
    for T, s in zip(tpl, line_set):
        if s > 0:
            S = members(masks[s - 1], N)
            if len(S) > 1:
                top = np.sort(l[o:o + T][:, S], axis=1)
                gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
        o += T
    return gap


def decode(idx, prob):
    """k_ctc_decode on one line: tokens, and the score as the fp32 sum in step order over the count (NaN without tokens)"""
    cols = R.kept_cols(idx)
    acc = np.float32(0.0)
    for t in cols:
        acc = np.float32(acc + np.float32(prob[t]))
    with np.errstate(invalid="ignore", divide="ignore"):
        score = np.float32(acc) / np.float32(len(cols))
    return [int(idx[t]) for t in cols], cols, np.float32(score)


def new_outputs(idx, prob, tpl, K):
    rows = max(int(sum(tpl)), 1)
    out = {"idx": np.array(idx, np.int32, copy=True), "prob": np.array(prob, np.float32, copy=True),
           "tokens": np.full(rows, CANARY_TOK, np.int32), "ntok": np.full(len(tpl), -1, np.int32),
           "scores": np.full(len(tpl), -5.0, np.float32)}
    out["cands"], out["cols"] = R.new_outputs(rows, max(K, 1))
    return out


def call(fn, handle, z, W, b, idx, prob, tpl, line_set, masks, K, chunk=None):
    """rt_debug_ctc_charset (handle, chunk given) or rt_debug_ctc_charset_host (handle None); returns (rc, outputs)"""
    N = W.shape[1]
    out = new_outputs(idx, prob, tpl, K)
    keep = [np.ascontiguousarray(a, t) for a, t in ((z, np.float32), (W, np.float32), (b, np.float32), (tpl, np.int32),
                                                     (line_set, np.int32), (np.asarray(masks).reshape(-1), np.uint32))]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(keep[0]), p(keep[1]), p(keep[2]), N, p(out["idx"]), p(out["prob"]), p(keep[3]), len(tpl), p(keep[4]), p(keep[5]),
            len(masks), K]
    if handle is not None:
        args = [handle] + args + [0 if chunk is None else chunk]
    args += [p(out["tokens"]), p(out["ntok"]), p(out["scores"]), p(out["cands"]) if K > 0 else None, p(out["cols"]) if K > 0 else None]
    return fn(*args), out


def stand_in(z, W, b, idx, prob, tpl, line_set, masks, K, mutant=None):
    """The whole hook in float32 numpy: what a correct implementation returns, or -- mutant -- one of the wrong ones in MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    N = W.shape[1]
    out = new_outputs(idx, prob, tpl, K)
    l = (np.asarray(z, np.float32) @ np.asarray(W, np.float32) + np.asarray(b, np.float32)).astype(np.float32)
    if mutant == "pad_columns_admitted":   # the GEMM's pad columns hold the logit 0
        l = np.concatenate([l, np.zeros((len(l), -N % 4), np.float32)], axis=1)
    ncol = l.shape[1]

    def allowed(s):
        if mutant == "mask_ignored":
            return list(range(N))
        S = [c for c in range(N) if (int(masks[s - 1][c >> 5]) >> (c & 31)) & 1]
        if mutant != "blank_not_forced" and 0 not in S:
            S = [0] + S
        return (S or [0]) + list(range(N, ncol))

    def best_first(row, S):   # ids of S by logit descending, ties by id (ascending; the mutant: descending)
        return sorted(S, key=lambda c: (-float(row[c]), -c if mutant == "ties_to_higher_id" else c))

    def softmax(row, S):
        over = list(range(ncol)) if mutant == "sum_over_all" else S
        e = np.exp((row - row[S].max()).astype(np.float32))
        return e / e[over].sum(dtype=np.float32)

    o = 0
    for li, (T, s) in enumerate(zip(tpl, line_set)):
        S = allowed(s) if s > 0 else None
        for t in range(T if S else 0):
            out["idx"][o + t] = best_first(l[o + t], S)[0]
            out["prob"][o + t] = softmax(l[o + t], S)[out["idx"][o + t]]
        toks, cols, score = decode(out["idx"][o:o + T], out["prob"][o:o + T])
        out["tokens"][o:o + len(toks)] = toks
        out["ntok"][li] = len(toks); out["scores"][li] = score
        for j, t in enumerate(cols if K > 0 else []):
            out["cols"][o + j] = t
            out["cands"][o + j][0] = (out["idx"][o + t], out["prob"][o + t])
            Sj = S if S else list(range(N))
            p = softmax(l[o + t], Sj)
            rest = [c for c in best_first(l[o + t], Sj) if c != out["idx"][o + t]][:K - 1]
            for r in range(1, K):
                out["cands"][o + j][r] = (rest[r - 1], p[rest[r - 1]]) if r - 1 < len(rest) else (-1, 0.0)
        o += T
    return out


def check_token_masked(tok, ids, ps, qS, S, tol, what=""):
    """ranks 1..K-1 of a token of a restricted row: every named class is in S, and -- with S renumbered 0 .. |S| - 1 -- the
    complete check of ctc_candidates_ref.check_token (fill from |S| - 1 entries on, distinct, |p - q|, nothing better left out)"""
    pos = {c: k for k, c in enumerate(S)}
    assert all(int(i) == -1 or int(i) in pos for i in ids), (what, "a class outside the set", list(ids))
    return R.check_token(pos[tok], [pos.get(int(i), -1) for i in ids], ps, qS[S], tol, what)


def check_outputs(out, z, W, b, idx0, prob0, tpl, line_set, masks, K, tol, what=""):
    """Everything a call must have produced, margin-free and with no row excluded.  Restricted rows: idx in S, its fp64 masked
    probability within 2 tol of the best allowed class's, the lowest id among the classes whose fp64 logit equals its own,
    |prob - q_S[idx]| <= tol.  Rows of set-0 lines: idx / prob untouched bit
    for bit.  Every line: tokens, count and score exactly the greedy decode of the RETURNED idx / prob, the canary past the count.
    K > 0: kept columns, rank 0 bit for bit, ranks >= 1 by check_token (masked on restricted lines).  Returns the worst |p - q|."""
    idx0 = np.asarray(idx0, np.int32); prob0 = np.asarray(prob0, np.float32)
    N = W.shape[1]
    l = logits64(z, W, b)
    worst, o = 0.0, 0
    for li, (T, s) in enumerate(zip(tpl, line_set)):
        gi, gp = out["idx"][o:o + T], out["prob"][o:o + T]
        S = members(masks[s - 1], N) if s > 0 else None
        qrows = {}
        if S is None:
            assert gi.tobytes() == idx0[o:o + T].tobytes() and gp.tobytes() == prob0[o:o + T].tobytes(), (what, li, "set-0 rows touched")
        else:
            for t in range(T):
                q = qrows[t] = masked_softmax64(l[o + t], S)
                assert int(gi[t]) in S, (what, li, t, "idx outside the set", int(gi[t]))
                assert q[gi[t]] >= q.max() - 2 * tol, (what, li, t, "not the best allowed class", float(q[gi[t]]), float(q.max()))
                tied = [c for c in S if l[o + t][c] == l[o + t][gi[t]]]   # (exact ties: all-zero features, where logits are biases)
                assert int(gi[t]) == tied[0], (what, li, t, "a tie must go to the lower id", int(gi[t]), tied)
                assert np.isfinite(gp[t]), (what, li, t)
                d = abs(float(gp[t]) - q[gi[t]])
                worst = max(worst, d)
                assert d <= tol, (what, li, t, "|prob - q_S|", d, tol)
        toks, cols, score = decode(gi, gp)
        assert out["ntok"][li] == len(toks), (what, li, "count", int(out["ntok"][li]), len(toks))
        assert list(out["tokens"][o:o + len(toks)]) == toks, (what, li, "tokens")
        assert np.all(out["tokens"][o + len(toks):o + T] == CANARY_TOK), (what, li, "tokens canary")
        assert np.float32(out["scores"][li]).tobytes() == score.tobytes() or (np.isnan(score) and np.isnan(out["scores"][li])), \
            (what, li, "score", float(out["scores"][li]), float(score))
        if K > 0:
            cands, ccols = out["cands"], out["cols"]
            assert list(ccols[o:o + len(cols)]) == cols, (what, li, "cols")
            for j, t in enumerate(cols):
                c = cands[o + j]
                assert c["id"][0] == gi[t] and c["prob"][0].tobytes() == gp[t].tobytes(), (what, li, j, "rank 0")
                if K > 1 and S is not None:
                    worst = max(worst, check_token_masked(int(gi[t]), c["id"][1:], c["prob"][1:], qrows[t], S, tol, (what, li, j)))
                elif K > 1:
                    q = masked_softmax64(l[o + t], list(range(N)))
                    worst = max(worst, R.check_token(int(gi[t]), c["id"][1:], c["prob"][1:], q, tol, (what, li, j)))
            assert np.all(ccols[o + len(cols):o + T] == R.CANARY_ID), (what, li, "cols canary")
            assert np.all(cands["id"][o + len(cols):o + T] == R.CANARY_ID), (what, li, "cands canary")
            assert np.all(cands["prob"][o + len(cols):o + T] == R.CANARY_PROB), (what, li, "cands canary")
        o += T
    return worst


def zero_feature_case(N, bias, T):
    """all-zero features: every logit is exactly its bias"""
    z = np.zeros((T, R.D), np.float32)
    W = np.random.default_rng(N).normal(0, 1, (R.D, N)).astype(np.float32)
    return z, W, np.asarray(bias, np.float32)

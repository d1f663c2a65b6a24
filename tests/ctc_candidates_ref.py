"""numpy fp64 restatement of the token-candidate rule (retto_amd/csrc/ctc_candidates.h, rt_config.rec_return_candidates) and the
checker the candidate tests share.  Nothing here calls the library."""
import ctypes as C

import numpy as np

D = 120                  # SvtrCore::D: width of the CTC head's input features
CANARY_ID = -7777        # what the tests put into the outputs before a call
CANARY_PROB = np.float32(-123.5)
CAND = np.dtype([("id", np.int32), ("prob", np.float32)])   # rt_candidate


def kept_cols(idx):
    """Time steps the greedy CTC decode keeps: argmax not the blank 0 and different from the previous step's argmax."""
    idx = np.asarray(idx)
    return [t for t in range(len(idx)) if idx[t] != 0 and (t == 0 or idx[t] != idx[t - 1])]


def softmax64(z, W, b):
    """fp64 logits z @ W + b and their softmax over every class, per row."""
    l = np.asarray(z, np.float64) @ np.asarray(W, np.float64)
    if b is not None:
        l = l + np.asarray(b, np.float64)
    l = l - l.max(axis=1, keepdims=True)
    e = np.exp(l)
    return e / e.sum(axis=1, keepdims=True)


def check_token(tok, ids, ps, q, tol, what=""):
    """The complete, margin-free check of ranks 1..K-1 of one token.  ids / ps: the returned entries after rank 0; q: the
    reference probabilities of every class.  Returns the worst |p - q| over the entries."""
    classes = len(q)
    n_real = min(len(ids), classes - 1)
    ids = [int(i) for i in ids]; ps = [float(p) for p in ps]
    for i, p in zip(ids[n_real:], ps[n_real:]):   # fill when the model has fewer than K classes
        assert i == -1 and p == 0.0, (what, "fill", ids, ps)
    ids, ps = ids[:n_real], ps[:n_real]
    assert len(set(ids)) == len(ids), (what, "distinct", ids)
    assert all(0 <= i < classes and i != tok for i in ids), (what, "range", ids, tok)
    worst = 0.0
    for k, (i, p) in enumerate(zip(ids, ps)):
        assert np.isfinite(p), (what, "finite", ps)
        if k > 0:
            assert p <= ps[k - 1] + tol, (what, "non-increasing", ps)
        worst = max(worst, abs(p - q[i]))
    assert worst <= tol, (what, "|p - q|", worst, tol)
    if ids:
        rest = np.array(q, np.float64, copy=True)
        rest[ids] = -1.0; rest[tok] = -1.0
        assert rest.max() <= min(ps) + 2 * tol, (what, "a better class was left out", float(rest.max()), min(ps))
    return worst


def new_outputs(rows, K):
    """(cands [rows, K], cols [rows]) filled with the canary."""
    cands = np.empty((max(rows, 1), K), CAND)
    cands["id"] = CANARY_ID; cands["prob"] = CANARY_PROB
    return cands, np.full(max(rows, 1), CANARY_ID, np.int32)


def call_args(z, W, b, idx, prob, tokens_per_line):
    """Contiguous arrays of the debug entry points' input arguments (kept alive by the caller) and their pointers."""
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in
            ((z, np.float32), (W, np.float32), (b, np.float32), (idx, np.int32), (prob, np.float32), (tokens_per_line, np.int32))]
    return keep, [None if a is None else a.ctypes.data_as(C.c_void_p) for a in keep]


def check_outputs(cands, cols, ntok, z, W, b, idx, prob, tokens_per_line, K, tol, what=""):
    """Everything a call must have produced: the kept columns, rank 0 copied bit for bit, ranks >= 1 per check_token against
    the fp64 softmax of the same features, and the canary in every slot past a line's token count.  Returns the worst |p - q|."""
    idx = np.asarray(idx, np.int32); prob = np.asarray(prob, np.float32)
    q = softmax64(z, W, b) if K > 1 else None
    worst, o = 0.0, 0
    for li, T in enumerate(tokens_per_line):
        kc = kept_cols(idx[o:o + T])
        assert ntok[li] == len(kc), (what, li, ntok[li], len(kc))
        assert list(cols[o:o + len(kc)]) == kc, (what, li)
        for j, t in enumerate(kc):
            c = cands[o + j]
            assert c["id"][0] == idx[o + t], (what, li, j)
            assert c["prob"][0].tobytes() == prob[o + t].tobytes(), (what, li, j)
            if K > 1:
                worst = max(worst, check_token(int(idx[o + t]), c["id"][1:], c["prob"][1:], q[o + t], tol, (what, li, j)))
        assert np.all(cols[o + len(kc):o + T] == CANARY_ID), (what, li, "cols canary")
        assert np.all(cands["id"][o + len(kc):o + T] == CANARY_ID), (what, li, "cands canary")
        assert np.all(cands["prob"][o + len(kc):o + T] == CANARY_PROB), (what, li, "cands canary")
        o += T
    return worst


def make_case(rng, n_classes, tokens_per_line, blank_share=0.3, repeat_share=0.3):
    """Features of the real scale (|z| up to about 20, He-scaled W) and the head's (argmax, probability) per time step for lines
    of tokens_per_line steps.  A share of the steps repeats the previous step's features (so its argmax: dropped by the keep
    rule) and a share is declared blank (idx 0), so that about a third of the steps are kept."""
    rows = int(sum(tokens_per_line))
    z = np.clip(rng.normal(0.0, 6.0, (max(rows, 1), D)), -20.0, 20.0).astype(np.float32)
    for r in range(1, rows):
        if rng.random() < repeat_share:
            z[r] = z[r - 1]
    W = (rng.normal(0.0, 1.0, (D, n_classes)) * np.sqrt(2.0 / D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, n_classes).astype(np.float32)
    q = softmax64(z, W, b)
    idx = q.argmax(axis=1).astype(np.int32)
    idx[rng.random(len(idx)) < blank_share] = 0
    prob = q[np.arange(len(idx)), idx].astype(np.float32)
    return z, W, b, idx[:max(rows, 1)], prob[:max(rows, 1)]

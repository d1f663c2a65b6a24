"""numpy fp64 restatement of the rec beam rule (retto_amd/csrc/ctc_beam.h), the checkers the beam tests share, and a float32
stand-in of the whole hook whose mutants the checkers must refuse (test_beam_cpu.py).  Nothing here decides what the library
computes; call() only marshals the arguments of rt_debug_ctc_beam / rt_debug_ctc_beam_host."""
import ctypes as C

import numpy as np

import ctc_lexicon_ref as LR

D = LR.D                     # SvtrCore::D: width of the CTC head's input features
MAX_BEAM = 32                # RT_MAX_BEAM
MAX_NBEST = 8                # RT_MAX_NBEST
TOP_C = 8                    # bm::TOP_C
BEAM = np.dtype([("logprob", np.float32), ("n_tokens", np.int32)])   # rt_beam
CANARY_N = -7777             # what the tests put into the outputs before a call
CANARY_TOK = -4242
CANARY_F = np.float32(-123.5)
MUTANTS = ("merge_forgotten", "repeat_takes_total", "stay_uses_blank", "ties_to_higher_index", "pad_columns_in_lse",
           "blank_in_top_c")
GRID_T = (1, 2, 7, 40)                           # per (T, repeat) one line; every third line of the grid is pure noise
GRID_LONG = 301
GRID_BEAMS = ((1, 1), (4, 4), (16, 8), (32, 8))  # (beam, nbest)
# Worst |logprob - fp64 rule| of the plain fp32 host loops (rt_debug_ctc_beam_host) over the grid, every (beam, nbest) of
# GRID_BEAMS and every N of ctc_lexicon_ref.GRID_N, at every rank: on the lines of up to 40 steps and on the line of 301 steps
# (test_beam_cpu.test_host_rule_on_the_grid_against_fp64 measures them again).  Both figures come from N = 6625, where
# lx::row_lse adds 6625 fp32 terms one after the other and a line's logprob carries one such lse per step (N = 5: 7.7e-6 and
# 3.3e-5, N = 65: 1.1e-5 and 4.0e-5).  The tolerances are 4 x these, the factor ctc_keyword_ref.TOL and ctc_lexicon_ref.HOOK_TOL
# take over their measurements.
MEASURED_HOST_SHORT = 4.951e-4
MEASURED_HOST_LONG = 7.667e-4
TOL = 4 * MEASURED_HOST_SHORT
TOL_LONG = 4 * MEASURED_HOST_LONG


def tol_of(T):
    return TOL if T <= 40 else TOL_LONG


# ---- the rule in fp64 ------------------------------------------------------------------------------------------------------
def _lae(a, b):
    return float(np.logaddexp(a, b))


def top_c(row, with_blank=False):
    """K_t of one row of logits: the up to TOP_C non-blank classes, by logit descending, then id ascending"""
    ids = np.arange(0 if with_blank else 1, len(row))
    order = ids[np.lexsort((ids, -row[ids]))]
    return [int(c) for c in order[:TOP_C]]


def beam64(l, B):
    """The rule over one line's fp64 logits l [T][N]: the WHOLE final beam in its own order as [(string tuple, logprob)]"""
    T = l.shape[0]
    if T == 0:
        return []
    lp = LR.logp64(l)
    beam = [((), 0.0, -np.inf)]
    for t in range(T):
        K = top_c(l[t])
        where = {h[0]: j for j, h in enumerate(beam)}
        tot = [_lae(pb, pnb) for _s, pb, pnb in beam]
        spb = [tot[j] + lp[t][0] for j in range(len(beam))]
        spnb = [pnb + lp[t][s[-1]] if s else -np.inf for s, _pb, pnb in beam]
        cands = []
        for j, (s, pb, pnb) in enumerate(beam):
            for r, c in enumerate(K):
                v = (pb if s and s[-1] == c else tot[j]) + lp[t][c]
                q = where.get(s + (c,))
                if q is not None:
                    spnb[q] = _lae(spnb[q], v)
                else:
                    cands.append((v, MAX_BEAM + j * TOP_C + r, s + (c,), -np.inf, v))
        for j, (s, _pb, _pnb) in enumerate(beam):
            cands.append((_lae(spb[j], spnb[j]), j, s, spb[j], spnb[j]))
        cands = [x for x in cands if x[0] > -np.inf]
        cands.sort(key=lambda x: (-x[0], x[1]))
        beam = [(s, pb, pnb) for _t, _i, s, pb, pnb in cands[:B]]
    return [(s, _lae(pb, pnb)) for s, pb, pnb in beam]


def loglik64(lp, s):
    """the full CTC forward log-likelihood of a string over one line's log-probabilities (the empty string: all blanks)"""
    if len(s) == 0:
        return float(lp[:, 0].sum())
    return float(LR.loglik64(lp, [list(s)])[0])


def reference(z, W, b, tpl, B):
    """per line (lp64 [T][N], the fp64 rule's whole final beam)"""
    l = LR.logits64(z, W, b) if sum(tpl) else np.zeros((0, W.shape[1]))
    out, o = [], 0
    for T in tpl:
        out.append((LR.logp64(l[o:o + T]) if T else np.zeros((0, W.shape[1])), beam64(l[o:o + T], B)))
        o += T
    return out


# ---- marshalling -----------------------------------------------------------------------------------------------------------
def new_outputs(tpl, nbest):
    beams = np.empty((max(len(tpl), 1), max(nbest, 1)), BEAM)
    beams["logprob"] = CANARY_F; beams["n_tokens"] = CANARY_N
    return {"n": np.full(max(len(tpl), 1), CANARY_N, np.int32), "beams": beams,
            "tokens": np.full(max(sum(max(T, 0) for T in tpl) * max(nbest, 1), 1), CANARY_TOK, np.int32)}


def call(fn, handle, z, W, b, tpl, beam, nbest, chunk=None):
    """rt_debug_ctc_beam (handle, chunk given) or rt_debug_ctc_beam_host (handle None); returns (rc, outputs)"""
    N = W.shape[1]
    out = new_outputs(tpl, nbest)
    keep = [np.ascontiguousarray(a, t) for a, t in ((z, np.float32), (W, np.float32), (b, np.float32), (tpl, np.int32))]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(keep[0]), p(keep[1]), p(keep[2]), N, p(keep[3]), len(tpl), beam, nbest]
    if handle is not None:
        args = [handle] + args + [0 if chunk is None else chunk]
    args += [p(out["n"]), p(out["beams"]), p(out["tokens"])]
    return fn(*args), out


def hyps_of(out, tpl, nbest):
    """per line [(string tuple, logprob float32)] of its reported hypotheses, with the canaries checked: record slots past the
    count, token slots past every length and everything of the hypotheses a line does not have"""
    res, o = [], 0
    for i, T in enumerate(tpl):
        n = int(out["n"][i])
        assert 0 <= n <= nbest, ("count", i, n)
        rec = out["beams"][i]
        assert (rec["n_tokens"][n:] == CANARY_N).all() and (rec["logprob"][n:] == CANARY_F).all(), ("record slots past the count", i)
        tok = out["tokens"][o * nbest:(o + T) * nbest].reshape(nbest, T) if T else np.zeros((nbest, 0), np.int32)
        hyps = []
        for k in range(n):
            L = int(rec["n_tokens"][k])
            assert 0 <= L <= T, ("length", i, k, L, T)
            assert (tok[k, L:] == CANARY_TOK).all(), ("token slots past the length", i, k)
            hyps.append((tuple(int(c) for c in tok[k, :L]), rec["logprob"][k]))
        assert (tok[n:] == CANARY_TOK).all(), ("token slots of a hypothesis the line does not have", i)
        res.append(hyps)
        o += T
    assert (out["n"][len(tpl):] == CANARY_N).all() and (out["tokens"][o * nbest:] == CANARY_TOK).all()
    return res


# ---- the checker -----------------------------------------------------------------------------------------------------------
def check(out, ref, tpl, N, B, nbest, tol_of, what=""):
    """Margin-free on every line and every hypothesis: the count is min(nbest, the fp64 rule's beam size); strings are distinct,
    hold no blank and no class outside the head; logprobs do not increase; canaries elsewhere; logprob <= the string's full CTC
    likelihood + tol.  Against the fp64 rule R: at every rank |logprob - R's| <= tol; the string at rank k is R's unless R's own gap
    to rank k - 1 or k + 1 (of its first nbest + 1) is <= 2 tol.  Returns {"worst": {T: worst |logprob - R's| over every
    rank}, "ranks": all, "skipped": ranks left out of the string comparison, "lines": lines with time steps,
    "rank0_skipped": lines whose rank 0 was left out}."""
    hyps = hyps_of(out, tpl, nbest)
    st = {"worst": {}, "ranks": 0, "skipped": 0, "lines": 0, "rank0_skipped": 0}
    for i, (T, (lp, R)) in enumerate(zip(tpl, ref)):
        w, tol, H = (what, "line", i, "T", T), tol_of(T), hyps[i]
        assert len(H) == min(nbest, len(R)), (w, "count", len(H), len(R))
        if T == 0:
            continue
        st["lines"] += 1
        assert len({s for s, _ in H}) == len(H), (w, "a string twice", H)
        for k, (s, v) in enumerate(H):
            assert all(1 <= c < N for c in s), (w, "a blank or a foreign class", k, s)
            assert np.isfinite(v), (w, "logprob", k, v)
            assert k == 0 or float(H[k - 1][1]) >= float(v), (w, "order", k, H[k - 1][1], v)
            full = loglik64(lp, s)
            assert float(v) <= full + tol, (w, "above the full likelihood", k, float(v), full, tol)
        Rv = [r[1] for r in R[:nbest + 1]]
        for k, (s, v) in enumerate(H):
            st["worst"][T] = max(st["worst"].get(T, 0.0), abs(float(v) - Rv[k]))
            assert abs(float(v) - Rv[k]) <= tol, (w, "logprob at rank", k, float(v), Rv[k], tol)
            near = (k > 0 and Rv[k - 1] - Rv[k] <= 2 * tol) or (k + 1 < len(Rv) and Rv[k] - Rv[k + 1] <= 2 * tol)
            st["ranks"] += 1
            if near:
                st["skipped"] += 1
                st["rank0_skipped"] += 1 if k == 0 else 0
                continue
            assert s == R[k][0], (w, "string at rank", k, s, R[k][0], Rv[max(k - 1, 0):k + 2])
    return st


def merge_stats(stats):
    out = {"worst": {}, "ranks": 0, "skipped": 0, "lines": 0, "rank0_skipped": 0}
    for s in stats:
        for k in ("ranks", "skipped", "lines", "rank0_skipped"):
            out[k] += s[k]
        for T, v in s["worst"].items():
            out["worst"][T] = max(out["worst"].get(T, 0.0), v)
    return out


def worst_short_long(st):
    return (max([v for T, v in st["worst"].items() if T <= 40] + [0.0]), max([v for T, v in st["worst"].items() if T > 40] + [0.0]))


def condition_holds(st):
    """the ranks left out of the string comparison are at most 10 % of all ranks, and rank 0 is left out on at most 5 % of the lines"""
    return st["skipped"] <= 0.10 * st["ranks"] and st["rank0_skipped"] <= 0.05 * st["lines"]


def same_strings(a, b, tpl, nbest):
    ha, hb = hyps_of(a, tpl, nbest), hyps_of(b, tpl, nbest)
    return [[s for s, _ in h] for h in ha] == [[s for s, _ in h] for h in hb]


# ---- a float32 stand-in of the whole hook, and its mutants ----------------------------------------------------------------
def stand_in(z, W, b, tpl, B, nbest, mutant=None):
    """What a correct implementation returns (fp32 logits, the rule in fp32 scalars), or -- mutant -- one of the wrong ones."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    N = W.shape[1]
    out = new_outputs(tpl, nbest)
    l = (np.asarray(z, f) @ np.asarray(W, f) + np.asarray(b, f)).astype(f)
    lcols = np.concatenate([l, np.zeros((len(l), -N % 4), f)], axis=1) if mutant == "pad_columns_in_lse" else l
    mx = lcols.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(lcols - mx).sum(axis=1, keepdims=True, dtype=f))).astype(f)
    lp = (l - lse).astype(f)
    NINF = f(-np.inf)

    def lae(a, c):
        m = max(a, c)
        if m == -np.inf:
            return NINF
        with np.errstate(invalid="ignore"):
            return f(m + np.log(f(f(np.exp(f(a - m))) + f(np.exp(f(c - m))))))

    o = 0
    for i, T in enumerate(tpl):
        beam = [((), f(0.0), NINF)] if T else []
        for t in range(T):
            row = lp[o + t]
            K = top_c(l[o + t].astype(np.float64), with_blank=mutant == "blank_in_top_c")
            where = {h[0]: j for j, h in enumerate(beam)}
            tot = [lae(pb, pnb) for _s, pb, pnb in beam]
            spb = [f(tot[j] + row[0]) for j in range(len(beam))]
            spnb = [f(pnb + row[0 if mutant == "stay_uses_blank" else s[-1]]) if s else NINF for s, _pb, pnb in beam]
            cands = []
            for j, (s, pb, pnb) in enumerate(beam):
                for r, c in enumerate(K):
                    v = f((pb if s and s[-1] == c and mutant != "repeat_takes_total" else tot[j]) + row[c])
                    q = where.get(s + (c,)) if mutant != "merge_forgotten" else None
                    if q is not None:
                        spnb[q] = lae(spnb[q], v)
                    else:
                        cands.append((v, MAX_BEAM + j * TOP_C + r, s + (c,), NINF, v))
            for j, (s, _pb, _pnb) in enumerate(beam):
                cands.append((lae(spb[j], spnb[j]), j, s, spb[j], spnb[j]))
            cands = [x for x in cands if x[0] > -np.inf]
            cands.sort(key=lambda x: (-float(x[0]), -x[1] if mutant == "ties_to_higher_index" else x[1]))
            beam = [(s, pb, pnb) for _t, _i, s, pb, pnb in cands[:B]]
        n = min(nbest, len(beam))
        out["n"][i] = n
        for k in range(n):
            s, pb, pnb = beam[k]
            out["beams"][i][k] = (lae(pb, pnb), len(s))
            out["tokens"][o * nbest + k * T:o * nbest + k * T + len(s)] = s
        o += T
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def weights(rng, N):
    W = (rng.normal(0.0, 1.0, (D, N)) * np.sqrt(2.0 / D)).astype(np.float32)
    return W, rng.normal(0.0, 0.5, N).astype(np.float32)


GRID_SEED = 9500


def grid_case(N, seed=GRID_SEED):
    """inputs of the N-grid of test_gpu_beam.py: (z, W, b, tokens_per_line).  Three lines of each T of GRID_T and one of GRID_LONG
    steps; every third line is pure noise, the others carry a random string planted by ctc_lexicon_ref.planted_features' formula
    (gain 4.0, noise 1.5) along ctc_lexicon_ref.alignment."""
    rng = np.random.default_rng(seed + N)
    W, b = weights(rng, N)
    tpl = [T for _ in range(3) for T in GRID_T] + [GRID_LONG]
    paths = []
    for i, T in enumerate(tpl):
        if i % 3 == 2:
            paths.append((T, None))
            continue
        e = LR.random_entry(rng, N, max(1, min(T // 2, 24)), T)
        paths.append((T, LR.alignment(e, T)))
    z = LR.planted_features(rng, W.astype(np.float64), paths, gain=4.0, noise=1.5)
    return z, W, b, tpl


def perturbed(W, seed=1):
    """W with every column scaled by 1 + k 2^-23, k in -2 .. 2: the logits move by a few ulp"""
    k = np.random.default_rng(seed).integers(-2, 3, W.shape[1]).astype(np.float64)
    return (W.astype(np.float64) * (1.0 + k * 2.0 ** -23)).astype(np.float32)


EXHAUSTIVE_SEED = 0


def exhaustive_case(seed):
    """classes = 3 (two symbols), T = 4: there are 31 strings of up to 4 tokens, so a beam of 32 never overflows"""
    rng = np.random.default_rng(7000 + seed)
    W, b = weights(rng, 3)
    z = np.clip(rng.normal(0.0, 1.5, (4, D)), -20.0, 20.0).astype(np.float32)
    return z, W, b, [4]


def all_strings(n_sym, max_len):
    out = [()]
    for L in range(1, max_len + 1):
        out += [tuple(int(c) + 1 for c in np.unravel_index(i, (n_sym,) * L)) for i in range(n_sym ** L)]
    return out


TIE_PAIRS = ((1, 5), (2, 6), (3, 8))
TIE_SEED = 1


def tie_case(seed=TIE_SEED):
    """N = 9: classes c and c' > c of TIE_PAIRS are identical bit for bit (W's columns and the bias), so the two extensions carry
    bit-equal totals on any device.  Lines of 3, 6 and 12 steps, one of them planted with classes of the pairs."""
    rng = np.random.default_rng(8100 + seed)
    W, b = weights(rng, 9)
    for c, c2 in TIE_PAIRS:
        W[:, c2] = W[:, c]; b[c2] = b[c]
    tpl = [3, 6, 12, 12]
    paths = [(3, None), (6, LR.alignment([1, 4, 2], 6)), (12, LR.alignment([3, 3, 1, 7, 2], 12)), (12, None)]
    z = LR.planted_features(rng, W.astype(np.float64), paths, gain=2.0, noise=1.5)
    return z, W, b, tpl


PLANTED_LENS = (1, 7, 15, 31)
PLANTED_T = 48


def planted_case(N):
    """one line of PLANTED_T steps per length of PLANTED_LENS, a random string planted (gain 4.0) into noise along its alignment;
    returns (z, W, b, tpl, entries, paths)"""
    rng = np.random.default_rng(8300 + N)
    W, b = weights(rng, N)
    entries = [LR.random_entry(rng, N, L, PLANTED_T) for L in PLANTED_LENS]
    paths = [LR.alignment(e, PLANTED_T) for e in entries]
    z = LR.planted_features(rng, W.astype(np.float64), [(PLANTED_T, p) for p in paths], gain=4.0, noise=1.5)
    return z, W, b, [PLANTED_T] * len(entries), entries, paths

"""numpy fp64 restatement of the rec vocabulary and its fusion into the beam (retto_amd/csrc/ctc_vocab.h): the count of words that
are no entries by its DIRECT DEFINITION (no trie: the string split into maximal runs of word classes), the fused beam rule on top
of ctc_lm_ref / ctc_beam_ref, the checker the beam-vocabulary tests share, the marshalling, and a float32 stand-in of the whole
hook whose mutants the checker must refuse (test_beam_vocab_cpu.py).  Nothing here decides what the library computes; call()
only marshals the arguments of rt_debug_ctc_beam_vocab / rt_debug_ctc_beam_vocab_host."""
import ctypes as C

import numpy as np

import ctc_beam_ref as BR
import ctc_lexicon_ref as LR
import ctc_lm_ref as MR

MAX_LEN = 63                 # RT_VOCAB_MAX_LEN
MAX_WORDS = 1 << 20          # RT_VOCAB_MAX_WORDS
MAX_VOCABS = 4               # RT_MAX_VOCABS
CASE_VARIANTS = 1            # RT_VOCAB_CASE_VARIANTS
OFF = -1
BEAM_VOCAB = np.dtype([("oov_words", np.int32), ("score", np.float32)])   # rt_beam_vocab
CANARY_OOV = -5151
CANARY_SCORE = np.float32(-654.75)
GAMMA = 1.5                  # the weight of the grid
ORDER = 3                    # the grid's model, where it has one: ctc_lm_ref.grid_model(N, 3, case), with ctc_lm_ref.ALPHA / BETA
MUTANTS = ("open_word_counted", "closing_forgotten", "count_again_on_merge", "separator_keeps_state", "terminal_ignored",
           "prefix_taken_as_word", "ranked_by_total", "gamma_on_lm_score")
# Worst |closing score - fp64 rule| of the plain fp32 host loops (rt_debug_ctc_beam_vocab_host) over ctc_beam_ref.grid_case, every
# (beam, nbest) of ctc_beam_ref.GRID_BEAMS and every N of ctc_lexicon_ref.GRID_N, alone and with the order-3 model, at every rank,
# with GAMMA: on the lines of up to 40 steps and on the line of 301 steps (test_beam_vocab_cpu.test_host_rule_on_the_grid_against_fp64
# measures them again).  gamma times a small integer is exact in fp32, so the figures stay close to the plain and the fused
# beam's: both come from N = 6625, the serial 6625-term lse of the host loops and, with the model, its sum.  On the fp64 rule's own
# gaps 34 of the grid's 1602 ranks are left out of the string comparison, rank 0 on none of the 312 lines.  The tolerances are 4 x
# these, the project's factor; the device is held to the same ones, never measured against itself.
MEASURED_HOST_SHORT = 4.992e-4
MEASURED_HOST_LONG = 7.917e-4
TOL = 4 * MEASURED_HOST_SHORT
TOL_LONG = 4 * MEASURED_HOST_LONG


def tol_of(T):
    return TOL if T <= 40 else TOL_LONG


# ---- the vocabulary --------------------------------------------------------------------------------------------------------
class Vocab:
    """classes: the head's (the blank included).  words: sequences of class ids of [1, classes), in id-form order; one given
    twice is one word."""

    def __init__(self, classes, words):
        self.classes = classes
        self.words = [tuple(int(c) for c in w) for w in words]
        self.entries = set(self.words)
        self.word_classes = {c for w in self.entries for c in w}
        self.prefixes = {w[:k] for w in self.entries for k in range(1, len(w) + 1)}
        self.node = {(): 0}                    # prefix -> the trie node's number: order of first creation, word by word, id by id
        for w in self.words:
            for k in range(1, len(w) + 1):
                self.node.setdefault(w[:k], len(self.node))

    def id_form(self):
        return np.array([c for w in self.words for c in w], np.int32), np.array([len(w) for w in self.words], np.int32)

    def runs(self, s):
        """the maximal runs of word classes of a string, and whether the last one reaches the string's end"""
        out, cur = [], []
        for c in s:
            if int(c) in self.word_classes:
                cur.append(int(c))
            elif cur:
                out.append(tuple(cur)); cur = []
        if cur:
            out.append(tuple(cur))
        return out, bool(cur)

    def count(self, s, closed=True):
        """the definition: the runs that are no entries; the last run, while open, counts only if it is no prefix of an entry"""
        runs, open_ = self.runs(s)
        n = sum(1 for r in runs if r not in self.entries)
        if not closed and open_ and runs[-1] not in self.entries and runs[-1] in self.prefixes:
            n -= 1
        return n

    def final_state(self, s):
        runs, open_ = self.runs(s)
        return self.node.get(runs[-1], OFF) if open_ else 0


def score64(fused, oov, gamma):
    return fused - float(np.float32(gamma)) * oov


# ---- the fused rule in fp64 ------------------------------------------------------------------------------------------------
def beam_vocab64(l, B, vocab, gamma, model=None, alpha=0.0, beta=0.0):
    """ctc_lm_ref.beam_lm64 with the selection by fused - gamma * (open count) and the final beam ranked by fused - gamma *
    (closed count), then beam order: the WHOLE final beam as [(string, logprob, lm, fused, closed count, closing score)]; without
    a model lm = 0 and fused = logprob"""
    T = l.shape[0]
    if T == 0:
        return []
    lp = LR.logp64(l)
    _lae = lambda a, b: float(np.logaddexp(a, b))
    beam = [((), 0.0, -np.inf)]
    lm_of, open_of = {(): 0.0}, {(): 0}
    fused = lambda tot, s: MR.fused64(tot, lm_of[s], len(s), alpha, beta) if model is not None else tot
    for t in range(T):
        K = BR.top_c(l[t])
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
                    cands.append((v, BR.MAX_BEAM + j * BR.TOP_C + r, s + (c,), -np.inf, v))
        for j, (s, _pb, _pnb) in enumerate(beam):
            cands.append((_lae(spb[j], spnb[j]), j, s, spb[j], spnb[j]))
        cands = [x for x in cands if x[0] > -np.inf]
        for x in cands:
            if x[2] not in open_of:
                open_of[x[2]] = vocab.count(x[2], closed=False)
                lm_of[x[2]] = model.lm64(x[2]) if model is not None else 0.0
        cands.sort(key=lambda x: (-score64(fused(x[0], x[2]), open_of[x[2]], gamma), x[1]))
        beam = [(s, pb, pnb) for _t, _i, s, pb, pnb in cands[:B]]
    out = []
    for s, pb, pnb in beam:
        tot, closed = _lae(pb, pnb), vocab.count(s)
        out.append((s, tot, lm_of[s], fused(tot, s), closed, score64(fused(tot, s), closed, gamma)))
    out.sort(key=lambda x: -x[5])     # (stable: ties keep the beam's order)
    return out


def reference(z, W, b, tpl, B, vocab, gamma, model=None, alpha=0.0, beta=0.0):
    """per line (lp64 [T][N], the fp64 rule's whole final beam in closing order)"""
    l = LR.logits64(z, W, b) if sum(tpl) else np.zeros((0, W.shape[1]))
    out, o = [], 0
    for T in tpl:
        out.append((LR.logp64(l[o:o + T]) if T else np.zeros((0, W.shape[1])), beam_vocab64(l[o:o + T], B, vocab, gamma, model, alpha, beta)))
        o += T
    return out


# ---- marshalling -----------------------------------------------------------------------------------------------------------
def new_outputs(tpl, nbest):
    out = MR.new_outputs(tpl, nbest)
    out["vocab"] = np.empty((max(len(tpl), 1), max(nbest, 1)), BEAM_VOCAB)
    out["vocab"]["oov_words"] = CANARY_OOV; out["vocab"]["score"] = CANARY_SCORE
    return out


def call(fn, handle, z, W, b, tpl, beam, nbest, vocab, gamma, model=None, alpha=0.0, beta=0.0, chunk=None, word_form=None,
         id_form=None, oov=None, lm_null=False):
    """rt_debug_ctc_beam_vocab (handle, chunk given) or rt_debug_ctc_beam_vocab_host (handle None); returns (rc, outputs).
    model None: no n-gram and the weights as given (0 and 0 mean no model).  word_form / id_form / oov: in place of the
    vocabulary's and the model's own.  lm_null: NULL in place of lm_out"""
    N = W.shape[1]
    out = new_outputs(tpl, nbest)
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    ids, lens, logp, bo = (none if model is None else model.id_form()) if id_form is None else id_form
    wids, wlens = vocab.id_form() if word_form is None else word_form
    keep = [np.ascontiguousarray(a, t) for a, t in ((z, np.float32), (W, np.float32), (b, np.float32), (tpl, np.int32),
                                                     (ids, np.int32), (lens, np.int32), (logp, np.float32), (bo, np.float32),
                                                     (wids, np.int32), (wlens, np.int32))]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(keep[0]), p(keep[1]), p(keep[2]), N, p(keep[3]), len(tpl), beam, nbest]
    if handle is not None:
        args = [handle] + args + [0 if chunk is None else chunk]
    args += [p(keep[4]), p(keep[5]), p(keep[6]), p(keep[7]), len(keep[5]),
             float((0.0 if model is None else model.oov) if oov is None else oov), float(alpha), float(beta)]
    args += [p(keep[8]), p(keep[9]), len(keep[9]), float(gamma)]
    args += [p(out["n"]), p(out["beams"]), p(out["tokens"]), None if lm_null else p(out["lm"]), p(out["vocab"])]
    return fn(*args), out


def walk_call(lib, vocab, strings, word_form=None, classes=None):
    """rt_debug_vocab_walk over strings; returns (rc, open [n], closed [n], state [n], message)"""
    wids, wlens = vocab.id_form() if word_form is None else word_form
    keep = [np.ascontiguousarray(a, np.int32) for a in (wids, wlens, [c for s in strings for c in s], [len(s) for s in strings])]
    res = [np.full(max(len(strings), 1), CANARY_OOV, np.int32) for _ in range(3)]
    err = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.rt_debug_vocab_walk(vocab.classes if classes is None else classes, p(keep[0]), p(keep[1]), len(keep[1]), p(keep[2]), p(keep[3]),
                                 len(strings), p(res[0]), p(res[1]), p(res[2]), err, 512)
    return rc, res[0], res[1], res[2], err.value.decode()


def compile_call(lib, dictionary_bytes, text, flags=0, cap=1 << 12):
    """rt_debug_vocab_compile; returns (rc, {ids, lens, words (tuples), n_words, nodes, word_classes, variants_dropped, classes,
    n, n_ids}, message)"""
    raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    ids = np.zeros(cap * 8, np.int32); lens = np.zeros(cap, np.int32)
    n_ids, n, words, nodes, wc, dropped, classes = (C.c_int() for _ in range(7))
    err = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.rt_debug_vocab_compile(dictionary_bytes, len(dictionary_bytes), raw, len(raw), flags, p(ids), len(ids), p(lens), cap,
                                    C.byref(n_ids), C.byref(n), C.byref(words), C.byref(nodes), C.byref(wc), C.byref(dropped),
                                    C.byref(classes), err, 512)
    got_ids, got_lens = ids[:n_ids.value if rc == 0 else 0], lens[:n.value if rc == 0 else 0]
    off = np.concatenate([[0], np.cumsum(got_lens)])
    return rc, {"ids": got_ids, "lens": got_lens, "words": [tuple(int(c) for c in got_ids[off[i]:off[i + 1]]) for i in range(len(got_lens))],
                "n_words": words.value, "nodes": nodes.value, "word_classes": wc.value, "variants_dropped": dropped.value,
                "classes": classes.value, "n": n.value, "n_ids": n_ids.value}, err.value.decode()


def hyps_of(out, tpl, nbest, fused):
    """per line [(string, logprob, lm, lm score, oov_words, score)] of its hypotheses (float32 / int32 scalars; lm and lm score
    None without a model, whose records must then be untouched), with ctc_beam_ref.hyps_of's canary checks and the records' own"""
    plain = BR.hyps_of(out, tpl, nbest)
    res = []
    for i, H in enumerate(plain):
        rec, lm = out["vocab"][i], out["lm"][i]
        assert (rec["oov_words"][len(H):] == CANARY_OOV).all() and (rec["score"][len(H):] == CANARY_SCORE).all(), ("vocab slots past the count", i)
        n_lm = len(H) if fused else 0
        assert (lm["lm"][n_lm:] == MR.CANARY_LM).all() and (lm["score"][n_lm:] == MR.CANARY_LM).all(), ("lm slots past the count", i)
        res.append([(s, v, lm["lm"][k] if fused else None, lm["score"][k] if fused else None, rec["oov_words"][k], rec["score"][k])
                    for k, (s, v) in enumerate(H)])
    assert (out["vocab"]["oov_words"][len(tpl):] == CANARY_OOV).all() and (out["lm"]["lm"][len(tpl):] == MR.CANARY_LM).all()
    return res


# ---- the checker -----------------------------------------------------------------------------------------------------------
def check(out, ref, tpl, N, B, nbest, tol_of, vocab, gamma, model=None, alpha=0.0, beta=0.0, what=""):
    """ctc_lm_ref.check with the comparisons made on the closing score.  Margin-free on every line and every hypothesis: the
    count; strings distinct, without a blank or a foreign class; closing scores do not increase; canaries elsewhere; logprob <=
    the string's full CTC likelihood + tol; with a model lm within tol of the definition's sum and the lm score = logprob +
    (alpha lm + beta len) to float32 rounding (no gamma in it); oov_words = the definition's closed count EXACTLY; score = fused
    - gamma * oov_words to float32 rounding.  Against the fp64 rule R: at every rank |score - R's| <= tol; the string at rank k
    is R's unless R's own gap to rank k - 1 or k + 1 (of its first nbest + 1) is <= 2 tol, and then its logprob is R's within
    tol.  Returns ctc_beam_ref.check's statistics, `worst` over |score - R's|."""
    fused = model is not None
    hyps = hyps_of(out, tpl, nbest, fused)
    a32, b32, g32 = float(np.float32(alpha)), float(np.float32(beta)), float(np.float32(gamma))
    st = {"worst": {}, "ranks": 0, "skipped": 0, "lines": 0, "rank0_skipped": 0}
    for i, (T, (lp, R)) in enumerate(zip(tpl, ref)):
        w, tol, H = (what, "line", i, "T", T), tol_of(T), hyps[i]
        assert len(H) == min(nbest, len(R)), (w, "count", len(H), len(R))
        if T == 0:
            continue
        st["lines"] += 1
        assert len({h[0] for h in H}) == len(H), (w, "a string twice", H)
        for k, (s, v, lm, lsc, oov, sc) in enumerate(H):
            assert all(1 <= c < N for c in s), (w, "a blank or a foreign class", k, s)
            assert np.isfinite(v) and np.isfinite(sc), (w, "a value", k, v, sc)
            assert k == 0 or float(H[k - 1][5]) >= float(sc), (w, "order", k, H[k - 1][5], sc)
            full = BR.loglik64(lp, s)
            assert float(v) <= full + tol, (w, "above the full likelihood", k, float(v), full, tol)
            base = float(v)
            if fused:
                want = model.lm64(s)
                assert abs(float(lm) - want) <= tol, (w, "lm", k, s, float(lm), want)
                mine = float(v) + (a32 * float(lm) + b32 * len(s))
                assert abs(float(lsc) - mine) <= 4e-7 * (abs(float(v)) + abs(a32 * float(lm)) + abs(b32 * len(s)) + 1.0), (w, "lm score", k, float(lsc), mine)
                base = float(lsc)
            assert int(oov) == vocab.count(s), (w, "oov_words", k, s, int(oov), vocab.count(s))
            mine = base - g32 * int(oov)
            assert abs(float(sc) - mine) <= 4e-7 * (abs(base) + abs(g32 * int(oov)) + 1.0), (w, "score", k, float(sc), mine)
        Rv = [r[5] for r in R[:nbest + 1]]
        for k, (s, v, lm, lsc, oov, sc) in enumerate(H):
            st["worst"][T] = max(st["worst"].get(T, 0.0), abs(float(sc) - Rv[k]))
            assert abs(float(sc) - Rv[k]) <= tol, (w, "score at rank", k, float(sc), Rv[k], tol)
            near = (k > 0 and Rv[k - 1] - Rv[k] <= 2 * tol) or (k + 1 < len(Rv) and Rv[k] - Rv[k + 1] <= 2 * tol)
            st["ranks"] += 1
            if near:
                st["skipped"] += 1
                st["rank0_skipped"] += 1 if k == 0 else 0
                continue
            assert s == R[k][0], (w, "string at rank", k, s, R[k][0], Rv[max(k - 1, 0):k + 2])
            assert abs(float(v) - R[k][1]) <= tol, (w, "logprob at rank", k, float(v), R[k][1])
    return st


# ---- a float32 stand-in of the whole hook, and its mutants ----------------------------------------------------------------
def stand_in(z, W, b, tpl, B, nbest, vocab, gamma, model=None, alpha=0.0, beta=0.0, mutant=None):
    """What a correct implementation returns (fp32 logits, the rule in fp32 scalars, a member carrying its trie state as the open
    run's prefix and its count; the model's sum in fp32 over the definition's per-token scores), or -- mutant -- one of the wrong
    ones."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    out = new_outputs(tpl, nbest)
    l = (np.asarray(z, f) @ np.asarray(W, f) + np.asarray(b, f)).astype(f)
    mx = l.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(l - mx).sum(axis=1, keepdims=True, dtype=f))).astype(f)
    lp = (l - lse).astype(f)
    NINF = f(-np.inf)
    a32, b32, g32 = f(alpha), f(beta), f(gamma)
    OFFS = "off"   # a state is the open run's prefix (a tuple on the trie, () the root) or OFFS

    def lae(a, c):
        m = max(a, c)
        if m == -np.inf:
            return NINF
        with np.errstate(invalid="ignore"):
            return f(m + np.log(f(f(np.exp(f(a - m))) + f(np.exp(f(c - m))))))

    def close(state):
        if state == OFFS or state == ():
            return 0
        if mutant == "prefix_taken_as_word":
            return 0
        if mutant == "terminal_ignored":
            return 1
        return 0 if state in vocab.entries else 1

    def step(state, c):
        if c not in vocab.word_classes:
            return (state if mutant == "separator_keeps_state" else ()), close(state)
        if state == OFFS:
            return OFFS, 0
        nx = state + (c,)
        return (nx, 0) if nx in vocab.prefixes else (OFFS, 1)

    def fused_of(total, lm, n):
        return f(total + f(f(a32 * lm) + f(b32 * f(n)))) if model is not None else total

    def key(total, lm, n, oov, state):
        if mutant == "ranked_by_total":
            return float(total)
        if mutant == "open_word_counted":
            oov = oov + (1 if state not in (OFFS, ()) and state not in vocab.entries else 0)
        return float(f(fused_of(total, lm, n) - f(g32 * f(oov))))

    o = 0
    for i, T in enumerate(tpl):
        # a member: (string, pb, pnb, lm, state, oov)
        beam = [((), f(0.0), NINF, f(0.0), (), 0)] if T else []
        for t in range(T):
            row = lp[o + t]
            K = BR.top_c(l[o + t].astype(np.float64))
            where = {h[0]: j for j, h in enumerate(beam)}
            tot = [lae(h[1], h[2]) for h in beam]
            spb = [f(tot[j] + row[0]) for j in range(len(beam))]
            spnb = [f(h[2] + row[h[0][-1]]) if h[0] else NINF for h in beam]
            soov = [h[5] for h in beam]
            cands = []
            for j, (s, pb, pnb, lm, state, oov) in enumerate(beam):
                for r, c in enumerate(K):
                    v = f((pb if s and s[-1] == c else tot[j]) + row[c])
                    q = where.get(s + (c,))
                    nx, add = step(state, c)
                    if q is not None:
                        spnb[q] = lae(spnb[q], v)
                        if mutant == "count_again_on_merge":
                            soov[q] += add
                    else:
                        nlm = f(lm + f(model.score64((model.bos,) + s, c))) if model is not None else f(0.0)
                        cands.append((v, BR.MAX_BEAM + j * BR.TOP_C + r, s + (c,), NINF, v, nlm, nx, oov + add))
            for j, (s, _pb, _pnb, lm, state, _oov) in enumerate(beam):
                cands.append((lae(spb[j], spnb[j]), j, s, spb[j], spnb[j], lm, state, soov[j]))
            cands = [x for x in cands if x[0] > -np.inf]
            cands.sort(key=lambda x: (-key(x[0], x[5], len(x[2]), x[7], x[6]), x[1]))
            beam = [(s, pb, pnb, lm, state, oov) for _t, _i, s, pb, pnb, lm, state, oov in cands[:B]]
        final = []
        for s, pb, pnb, lm, state, oov in beam:
            total = lae(pb, pnb)
            closed = oov + (0 if mutant == "closing_forgotten" else close(state))
            fu = fused_of(total, lm, len(s))
            final.append((s, total, lm, fu, closed, f(fu - f(g32 * f(closed)))))
        if mutant not in ("closing_forgotten", "ranked_by_total"):
            final.sort(key=lambda x: -float(x[5]))
        n = min(nbest, len(final))
        out["n"][i] = n
        for k in range(n):
            s, total, lm, fu, closed, sc = final[k]
            out["beams"][i][k] = (total, len(s))
            if model is not None:
                out["lm"][i][k] = (lm, sc if mutant == "gamma_on_lm_score" else fu)
            out["vocab"][i][k] = (closed, sc)
            out["tokens"][o * nbest + k * T:o * nbest + k * T + len(s)] = s
        o += T
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
VOCAB_SEED = 5300


def is_grid_separator(c):
    return c % 4 == 0


def grid_vocab(N, case):
    """the grid's vocabulary of one N: the classes divisible by 4 never occur in a word (class 4 at N = 5: the separators the
    lines are sure to hold); 60 % of the word runs of the plain fp64 beam's (width 4) best readings of the grid's lines, so that
    hypotheses hold entries, prefixes of entries and words that are none, plus as many random words of 1 to 5 ids"""
    z, W, b, tpl = case
    rng = np.random.default_rng(VOCAB_SEED + N)
    runs = []
    for _lp, R in BR.reference(z, W, b, tpl, 4):
        cur = []
        for c in (R[0][0] if R else ()) + (0,):
            if c and not is_grid_separator(c):
                cur.append(c)
            elif cur:
                runs.append(tuple(cur[:MAX_LEN])); cur = []
    runs = sorted(set(runs))
    words = [r for r in runs if rng.random() < 0.6]
    real = [c for c in range(1, N) if not is_grid_separator(c)]
    for _ in range(max(len(words), 1)):
        words.append(tuple(int(real[int(rng.integers(len(real)))]) for _ in range(int(rng.integers(1, 6)))))
    return Vocab(N, words)


RESCUE_N = 6
RESCUE_WORD = (1, 2, 3)
RESCUE_WRONG = (1, 4, 3)


def rescue_case():
    """ctc_lm_ref.rescue_case's line over seeded noise: it spells RESCUE_WORD along 1 _ 2 _ 3 _, each step's class 6 above the
    rest, but at the step of the 2 class 4 stands 1.0 above it -- the evidence alone reads RESCUE_WRONG, a non-word one class
    away from the entry.  (The noise, within +-0.5, keeps the weak hypotheses from tying exactly: which of them a beam holds is
    then no matter of rounding.)  The vocabulary holds the entry and one word with class 4, so that 4 is a word class and
    (1, 4, 3) one run that is no entry."""
    path = [1, 0, 2, 0, 3, 0]
    logits = np.random.default_rng(8400).uniform(-0.5, 0.5, (6, RESCUE_N))
    for t, c in enumerate(path):
        logits[t, c] = 6.0
    logits[2, 4] = 7.0
    return MR.logits_case(logits), Vocab(RESCUE_N, [RESCUE_WORD, (4, 5)])


def prefix_case():
    """One line of 2 steps for beam 1: step 0 puts class 1 -- the first id of the only entry (1, 2), an OPEN word on the trie --
    0.5 above the separator 3; step 1 reads class 2.  The rule does not count the open word, keeps (1) and ends in the entry
    (1, 2) with no word charged; a rule that counts an open word keeps (3) and ends in (3, 2), whose word (2) is no entry."""
    logits = np.zeros((2, 5))
    logits[0, 1] = 6.0; logits[0, 3] = 5.5; logits[1, 2] = 6.0
    return MR.logits_case(logits, seed=3), Vocab(5, [(1, 2)])


def tie_vocab():
    """a vocabulary in which the classes of ctc_beam_ref.TIE_PAIRS are interchangeable: every word comes with each of its
    spellings over the pairs, so that two strings that differ by a pair's classes carry the same counts"""
    rng = np.random.default_rng(8300)
    twin = {}
    for lo, hi in BR.TIE_PAIRS:
        twin[lo] = (lo, hi); twin[hi] = (lo, hi)
    words = set()
    for _ in range(12):
        w = tuple(int(rng.integers(1, 9)) for _ in range(int(rng.integers(1, 4))))
        if any(c == 4 for c in w):      # (class 4 stays a separator)
            continue
        forms = [()]
        for c in w:
            forms = [g + (x,) for g in forms for x in twin.get(c, (c,))]
        words.update(forms)
    return Vocab(9, sorted(words))

"""numpy fp64 restatement of the rec pattern rule (retto_amd/csrc/ctc_pattern.h), independent of the C++ tables: its own parser
for the pattern language, Python's re.fullmatch over a class -> character map as the acceptance oracle, an fp64 Viterbi over the
product of the CTC frame labels and its own DFA with the rule's tie order, a brute force over every labelling for short lines,
the checker the pattern tests share, and a float32 stand-in of the hook whose mutants the checker must refuse
(test_pattern_cpu.py).  Nothing here decides what the library computes; call() only marshals the arguments of
rt_debug_ctc_pattern / rt_debug_ctc_pattern_host."""
import ctypes as C
import itertools
import re

import numpy as np

import ctc_align_ref as AR
import ctc_lexicon_ref as LR

CANARY_IDX = AR.CANARY_IDX
CANARY_F = LR.CANARY_F
BASE = 0xE000          # class c stands as chr(BASE + c) in the oracle's strings (a private-use block: no regex meaning)
META = "\\.[]()|?*+{}^-"
MUTANTS = ("exclusion_dropped", "enter_before_stay", "ties_to_highest_class", "val2_not_excluding", "end_over_all_states",
           "prob_restricted_softmax", "other_line_written")
NINF = -np.inf
# logprob and free_logprob are held to LR.HOOK_TOL on lines of up to 40 steps.  On the long lines of
# test_gpu_pattern.test_long_lines_on_both_sides_of_the_lds_boundary (up to 513 steps, sum of lse up to 2000) that constant is too
# tight for a reason that is no bug: both values are sums of T fp32 terms added in t order, each add rounding at half an ulp of
# a running sum in the thousands.  Measured on that case against the fp64 reference: the host fp32 entry
# (rt_debug_ctc_pattern_host) deviates by 1.341e-3, the device by MEASURED_DEVICE_LOGPROB_LONG; the tolerance is four times the
# host figure, the project's margin.
MEASURED_HOST_LOGPROB_LONG = 1.341e-3
MEASURED_DEVICE_LOGPROB_LONG = 1.463e-3
LOGPROB_TOL_LONG = 4 * MEASURED_HOST_LOGPROB_LONG


def entries_of(dict_bytes):
    """the dictionary as the recogniser numbers it: "blank", the file's trimmed lines, " " (plain lines: no odd whitespace here)"""
    text = dict_bytes.decode("utf-8")
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return ["blank"] + [ln.strip() for ln in lines] + [" "]


def synthetic_dictionary(N):
    """N classes: the blank, N - 2 one-code-point entries U+4E00 ..., the appended " "; (bytes, entries)"""
    data = "".join(chr(0x4E00 + i) + "\n" for i in range(N - 2)).encode("utf-8")
    return data, entries_of(data)


# ---- the parser ------------------------------------------------------------------------------------------------------------
def tokens_of(pattern, entries):
    """[("atom", frozenset of class ids) | ("op", one of | ( ) ? * +) | ("rep", m, n or None)]"""
    N = len(entries)
    single = {}
    for c in range(1, N):
        if len(entries[c]) == 1:
            single.setdefault(entries[c], []).append(c)

    def lit(ch):
        assert ch in single, ("no entry for", ch)
        return set(single[ch])

    def rng(a, z):
        assert a in single and z in single and a <= z
        return {c for ch, cs in single.items() if a <= ch <= z for c in cs}

    out, i, n = [], 0, len(pattern)

    def escape(i):
        """the set behind a backslash at pattern[i - 1]; returns (set, next i)"""
        ch = pattern[i]
        if ch == "d":
            return rng("0", "9"), i + 1
        if ch == "c":
            j = pattern.index("}", i)
            return {int(pattern[i + 2:j])}, j + 1
        assert ch in META
        return lit(ch), i + 1

    while i < n:
        ch = pattern[i]
        if ch in "|()?*+":
            out.append(("op", ch)); i += 1
        elif ch == "{":
            j = pattern.index("}", i)
            body = pattern[i + 1:j].split(",")
            m = int(body[0])
            out.append(("rep", m, m if len(body) == 1 else (None if body[1] == "" else int(body[1]))))
            i = j + 1
        elif ch == ".":
            out.append(("atom", frozenset(range(1, N)))); i += 1
        elif ch == "\\":
            s, i = escape(i + 1)
            out.append(("atom", frozenset(s)))
        elif ch == "[":
            i += 1
            neg = pattern[i] == "^"
            i += neg
            s = set()
            while pattern[i] != "]":
                if pattern[i] == "\\":
                    e, i = escape(i + 1)
                    s |= e
                elif pattern[i + 1] == "-" and pattern[i + 2] != "]":
                    s |= rng(pattern[i], pattern[i + 2]); i += 3
                else:
                    s |= lit(pattern[i]); i += 1
            i += 1
            out.append(("atom", frozenset(set(range(1, N)) - s if neg else s)))
        else:
            out.append(("atom", frozenset(lit(ch)))); i += 1
    return out


def python_regex(tokens):
    """the pattern for re.fullmatch over strings of chr(BASE + class)"""
    parts = []
    for tk in tokens:
        if tk[0] == "atom":
            parts.append("[" + "".join(chr(BASE + c) for c in sorted(tk[1])) + "]")
        elif tk[0] == "op":
            parts.append("(?:" if tk[1] == "(" else tk[1])
        else:
            parts.append("{%d%s}" % (tk[1], "" if tk[2] == tk[1] else "," + ("" if tk[2] is None else str(tk[2]))))
    return re.compile("".join(parts))


class _Nfa:
    def __init__(self):
        self.eps, self.arcs = [], []          # per state: epsilon targets; (class set, target)

    def state(self):
        self.eps.append([]); self.arcs.append([])
        return len(self.eps) - 1


def _build_nfa(tokens):
    """Thompson's construction by recursive descent; returns (nfa, start, end)"""
    nfa, pos = _Nfa(), [0]

    def peek():
        return tokens[pos[0]] if pos[0] < len(tokens) else None

    def alt():
        s, e = nfa.state(), nfa.state()
        while True:
            a, b = concat()
            nfa.eps[s].append(a); nfa.eps[b].append(e)
            if peek() == ("op", "|"):
                pos[0] += 1
            else:
                return s, e

    def concat():
        s = e = nfa.state()
        while peek() is not None and peek() not in (("op", "|"), ("op", ")")):
            a, b = repeat()
            nfa.eps[e].append(a); e = b
        return s, e

    def repeat():
        start = pos[0]

        def one():   # parses the atom or group at `start` (again): a fresh copy each time
            pos[0] = start
            tk = tokens[pos[0]]; pos[0] += 1
            if tk == ("op", "("):
                a, b = alt()
                assert peek() == ("op", ")")
                pos[0] += 1
                return a, b
            assert tk[0] == "atom", tk
            a, b = nfa.state(), nfa.state()
            nfa.arcs[a].append((tk[1], b))
            return a, b

        spare = [one()]
        tk = peek()
        if tk is None or not (tk[0] == "rep" or tk in (("op", "?"), ("op", "*"), ("op", "+"))):
            return spare[0]
        after = pos[0] + 1
        m, x = {("op", "?"): (0, 1), ("op", "*"): (0, None), ("op", "+"): (1, None)}.get(tk, tk[1:])
        copy = lambda: spare.pop() if spare else one()
        s = e = nfa.state()
        for _ in range(m):                # m mandatory copies
            a, b = copy()
            nfa.eps[e].append(a); e = b
        if x is None:                     # ... then any number more
            a, b = copy()
            loop = nfa.state()
            nfa.eps[e].append(loop); nfa.eps[loop].append(a); nfa.eps[b].append(loop); e = loop
        else:
            for _ in range(x - m):        # ... then x - m optional ones
                a, b = copy()
                nx = nfa.state()
                nfa.eps[e].append(a); nfa.eps[e].append(nx); nfa.eps[b].append(nx); e = nx
        pos[0] = after
        return s, e

    s, e = alt()
    assert pos[0] == len(tokens), "trailing tokens"
    return nfa, s, e


class Auto:
    """A DFA as flat arc arrays (src, cls, dst), start state 0, and what the Viterbi needs of it: the pairs (dst, cls) sorted,
    each pair's predecessor edges sorted by src"""

    def __init__(self, n_states, src, cls, dst, accept):
        self.S = n_states
        self.accept = np.asarray(accept, bool)
        src, cls, dst = (np.asarray(a, np.int64) for a in (src, cls, dst))
        self.src, self.cls, self.dst = src, cls, dst
        key = dst * (1 << 20) + cls
        ukey, inv = np.unique(key, return_inverse=True)
        self.pair_q, self.pair_c = ukey >> 20, ukey & ((1 << 20) - 1)
        self.P = len(ukey)
        order = np.lexsort((src, inv))
        self.e_pair, self.e_src = inv[order], src[order]
        self.seg = np.searchsorted(self.pair_q, np.arange(n_states + 1))
        self.e_start = np.searchsorted(self.e_pair, np.arange(self.P))
        self.start_pair = np.zeros(self.P, bool)
        self.start_pair[self.e_pair[self.e_src == 0]] = True

    def run(self, seq):
        """the state after consuming the class string, or None"""
        q = 0
        for c in seq:
            hit = np.nonzero((self.src == q) & (self.cls == c))[0]
            if len(hit) == 0:
                return None
            q = int(self.dst[hit[0]])
        return q

    def accepts(self, seq):
        q = self.run(seq)
        return q is not None and bool(self.accept[q])


class Pattern:
    """a pattern over a dictionary: .rx the oracle, .auto this file's own DFA (subset construction, dead states dropped)"""

    def __init__(self, pattern, entries):
        self.text, self.N = pattern, len(entries)
        tokens = tokens_of(pattern, entries)
        self.rx = python_regex(tokens)
        nfa, s0, end = _build_nfa(tokens)

        def closure(states):
            seen, todo = set(states), list(states)
            while todo:
                for v in nfa.eps[todo.pop()]:
                    if v not in seen:
                        seen.add(v); todo.append(v)
            return frozenset(seen)

        start = closure([s0])
        ids, order, arcs = {start: 0}, [start], []
        k = 0
        while k < len(order):
            cur = order[k]
            by_class = {}
            for u in cur:
                for cs, v in nfa.arcs[u]:
                    for c in cs:
                        by_class.setdefault(c, set()).add(v)
            memo = {}
            for c in sorted(by_class):
                tgt = frozenset(by_class[c])
                if tgt not in memo:
                    memo[tgt] = closure(tgt)
                nx = memo[tgt]
                if nx not in ids:
                    ids[nx] = len(order); order.append(nx)
                arcs.append((k, c, ids[nx]))
            k += 1
        accept = [end in st for st in order]
        # (every state of a Thompson NFA with non-empty atoms reaches the end state, so none is dead)
        self.auto = Auto(len(order), [a[0] for a in arcs], [a[1] for a in arcs], [a[2] for a in arcs], accept)

    def accepts(self, seq):
        return self.rx.fullmatch("".join(chr(BASE + c) for c in seq)) is not None


def collapse(idx):
    return AR.collapse(idx)


def differing(auto, s):
    """the product of `auto` with the DFA of "any string but s": the best path over it is the best path whose collapse differs"""
    L = len(s)
    D = L + 2                                   # d < L: s[:d] matched so far; L: all of s; L + 1: deviated
    s_arr = np.asarray(list(s) + [-1, -1], np.int64)
    d = np.arange(D)[None, :]
    c = auto.cls[:, None]
    d2 = np.where((d < L) & (s_arr[np.minimum(d, L)] == c), d + 1, L + 1)
    src = (auto.src[:, None] * D + d).ravel(); dst = (auto.dst[:, None] * D + d2).ravel(); cls = np.broadcast_to(c, d2.shape).ravel()
    accept = (auto.accept[:, None] & (np.arange(D)[None, :] != L)).ravel()
    # only the states reachable from (0, 0) matter; the unreachable ones stay at -inf by themselves
    return Auto(auto.S * D, src, cls, dst, accept)


# ---- the rule in fp64 ------------------------------------------------------------------------------------------------------
def _top2(A, Cv):
    S, P = A.S, A.P
    v1 = np.full(S, NINF); v2 = np.full(S, NINF); a1 = np.full(S, -1, np.int64); a2 = np.full(S, -1, np.int64)
    if P == 0:
        return v1, a1, v2, a2
    ne = A.seg[1:] > A.seg[:-1]
    starts = A.seg[:-1][ne]
    ar = np.arange(P)

    def best(vals):
        v = np.maximum.reduceat(vals, starts)
        full = np.full(S, NINF); full[ne] = v
        hit = (vals == full[A.pair_q]) & (vals > NINF)
        first = np.minimum.reduceat(np.where(hit, ar, P), starts)
        a = np.full(S, -1, np.int64); a[ne] = np.where(first < P, first, -1)
        return full, a

    v1, a1 = best(Cv)
    rest = Cv.copy(); rest[a1[a1 >= 0]] = NINF
    v2, a2 = best(rest)
    return v1, a1, v2, a2


def viterbi64(l, A, want_path=True):
    """(value, path or None): the rule of ctc_pattern.h in fp64 over the automaton A; value -inf: infeasible.  Codes: -1 stay,
    -(q + 2) from the blank of q, >= 0 a pair"""
    T = l.shape[0]
    if T < 1:
        return NINF, None
    S, P = A.S, A.P
    B = np.full(S, NINF); B[0] = l[0, 0]
    Cv = np.where(A.start_pair, l[0, A.pair_c], NINF) if P else np.zeros(0)
    bpC, bpB = [None], [None]
    E = len(A.e_pair)
    ar = np.arange(E)
    for t in range(1, T):
        v1, a1, v2, a2 = _top2(A, Cv)
        k1 = np.where(a1 >= 0, A.pair_c[np.maximum(a1, 0)], 0) if P else np.zeros(S, np.int64)
        if P:
            q = A.e_src; c = A.pair_c[A.e_pair]
            other = k1[q] != c
            cand = np.where(other, v1[q], v2[q]); ca = np.where(other, a1[q], a2[q])
            use = cand > B[q]
            into = np.where(use, cand, B[q]); code = np.where(use, ca, -(q + 2))
            m = np.maximum.reduceat(into, A.e_start)
            first = np.minimum.reduceat(np.where(into == m[A.e_pair], ar, E), A.e_start)
            take = m > Cv
            newC = l[t, A.pair_c] + np.where(take, m, Cv)
            bpC.append(np.where(take, code[np.minimum(first, E - 1)], -1))
        else:
            newC = Cv; bpC.append(np.zeros(0, np.int64))
        takeB = v1 > B
        bpB.append(np.where(takeB, a1, -1))
        B = l[t, 0] + np.where(takeB, v1, B)
        Cv = newC
    v1, a1, _, _ = _top2(A, Cv)
    best, node = NINF, None
    for q in np.nonzero(A.accept)[0]:
        if B[q] > best:
            best, node = B[q], -(int(q) + 2)
        if v1[q] > best:
            best, node = v1[q], int(a1[q])
    if node is None or not want_path:
        return float(best), None
    path = [0] * T
    for t in range(T - 1, -1, -1):
        path[t] = 0 if node < 0 else int(A.pair_c[node])
        if t > 0:
            k = int(bpB[t][-node - 2]) if node < 0 else int(bpC[t][node])
            if k != -1:
                node = k
    return float(best), path


def brute64(l, pat):
    """the best labelling of a short line whose collapse the oracle accepts: (value, collapse) or (-inf, None)"""
    T, N = l.shape
    best, arg = NINF, None
    for lab in itertools.product(range(N), repeat=T):
        if pat.accepts(collapse(lab)):
            v = float(sum(l[t, lab[t]] for t in range(T)))
            if v > best:
                best, arg = v, lab
    return best, (collapse(arg) if arg is not None else None)


def min_steps64(pat, limit=140):
    """the least T at which some labelling is accepted, by the boolean recurrence (all-zero logits)"""
    for T in range(1, limit):
        if viterbi64(np.zeros((T, pat.N)), pat.auto, want_path=False)[0] > NINF:
            return T
    return None


# ---- marshalling -----------------------------------------------------------------------------------------------------------
def flat_tables(compiled):
    """a list of retto_amd.debug_pattern_compile results as rt_debug_ctc_pattern's flat tables"""
    S = np.asarray([c["S"] for c in compiled], np.int32); G = np.asarray([c["G"] for c in compiled], np.int32)
    group_of = np.ascontiguousarray(np.stack([c["group_of"] for c in compiled]), np.int32)
    delta = np.ascontiguousarray(np.concatenate([c["delta"].ravel() for c in compiled]), np.int32)
    accept = np.ascontiguousarray(np.concatenate([c["accept"] for c in compiled]), np.int32)
    return S, G, group_of, delta, accept


def new_outputs(tpl, idx0=None, prob0=None):
    rows = max(sum(tpl), 1)
    return dict(idx=np.full(rows, CANARY_IDX, np.int32) if idx0 is None else np.array(idx0, np.int32),
                prob=np.full(rows, CANARY_F, np.float32) if prob0 is None else np.array(prob0, np.float32),
                matched=np.full(len(tpl), CANARY_IDX, np.int32), vit=np.full(len(tpl), CANARY_F, np.float32),
                logprob=np.full(len(tpl), CANARY_F, np.float32), free=np.full(len(tpl), CANARY_F, np.float32))


def call(fn, handle, z, W, b, tpl, line_pat, compiled, chunk=None, idx0=None, prob0=None):
    """rt_debug_ctc_pattern (handle, chunk given) or rt_debug_ctc_pattern_host (handle None); returns (rc, outputs)"""
    N = W.shape[1]
    out = new_outputs(tpl, idx0, prob0)
    tabs = flat_tables(compiled)
    keep = [np.ascontiguousarray(a, t) for a, t in ((z, np.float32), (W, np.float32), (b, np.float32), (tpl, np.int32),
                                                     (line_pat, np.int32))]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(keep[0]), p(keep[1]), p(keep[2]), N, p(keep[3]), len(tpl), p(keep[4])] + [p(a) for a in tabs] + [len(compiled)]
    if handle is not None:
        args = [handle] + args + [0 if chunk is None else chunk]
    args += [p(out[k]) for k in ("idx", "prob", "matched", "vit", "logprob", "free")]
    return fn(*args), out


# ---- exact inputs and known answers ----------------------------------------------------------------------------------------
DICT5 = "a\nb\nc\n".encode()                              # N = 5, no duplicate: a = 1, b = 2, c = 3, " " = 4


def crafted(lines):
    """features and weights whose logits are exactly the given rows (one-hot features, the rows as weights; at most 120 rows):
    (z, W, b, tokens_per_line, fp64 logits)"""
    rows = np.concatenate([np.asarray(l, np.float64) for l in lines])
    assert len(rows) <= LR.D
    W = np.zeros((LR.D, rows.shape[1]), np.float32); W[:len(rows)] = rows
    z = np.zeros((len(rows), LR.D), np.float32); z[np.arange(len(rows)), np.arange(len(rows))] = 1.0
    assert (W[:len(rows)].astype(np.float64) == rows).all()
    return z, W, np.zeros(rows.shape[1], np.float32), [len(l) for l in lines], rows


def flat(T, N, v=-1.0):
    return np.full((T, N), v)


KNOWN = [  # (what the tie rule decides, pattern, logits rows, idx, matched)
    ("the path packs to the left and ends in the blank", "ab", flat(5, 5), [1, 2, 0, 0, 0], 1),
    ("the lowest class of a set wins", "[ab]", flat(2, 5), [1, 0], 1),
    ("the lowest class of a set wins, on the last frame too", "[bc]", flat(1, 5), [2], 1),
    ("the lowest predecessor wins", "(a|c)b", flat(2, 5), [1, 2], 1),
    ("stay before enter", "ab", [[-8, 0, -8, -8, -8], [-8, 0, 0, -8, -8], [-8, -8, 0, -8, -8]], [1, 2, 2], 1),
    ("within a predecessor the blank comes before a class", "ab", [[-8, 0, -8, -8, -8], [0, 0, -8, -8, -8], [-8, -8, 0, -8, -8]], [1, 0, 2], 1),
    ("bb needs its blank: two steps do not match", "bb", flat(2, 5), None, 0),
    ("... and three do", "bb", flat(3, 5), [2, 0, 2], 1),
    ("a* matches the all-blank path", "a*", flat(3, 5), [0, 0, 0], 1),
    ("a top-1 class equal to the entering class takes val2", "[ab]b", [[-8, -1, 0, -8, -8], [-8, -8, 0, -8, -8]], [1, 2], 1),
    ("the empty pattern matches blanks only", "", [[0, 1, 1, 1, 1], [0, 1, 1, 1, 1]], [0, 0], 1),
]


def known_case(compile_fn):
    """the KNOWN lines as one call: (z, W, b, tokens_per_line, line_pat, compiled, patterns, fp64 logits); compile_fn:
    retto_amd.debug_pattern_compile"""
    entries = entries_of(DICT5)
    texts = [k[1] for k in KNOWN]
    z, W, b, tpl, l64 = crafted([np.asarray(k[2], np.float64) for k in KNOWN])
    return z, W, b, tpl, list(range(1, len(KNOWN) + 1)), [compile_fn(DICT5, t) for t in texts], \
        [Pattern(t, entries) for t in texts], l64


# ---- the checker -----------------------------------------------------------------------------------------------------------
def check_pattern(out, l64, tpl, line_pat, pats, vit_tol, prob_tol, lp_tol, idx0=None, prob0=None, exact_logits=False, what=""):
    """Everything a call must have produced, margin-free, no line left out; l64 [rows][N]: the fp64 logits of the same features;
    pats: the Pattern of each pattern id; idx0 / prob0: the rows the call was given (None: the canaries).  Per pattern line:
    matched equals fp64 feasibility; a matched line's collapse is accepted by the oracle; the fp64 score of the returned path is
    within vit_tol of the fp64 optimum and vit_out within vit_tol of that score; prob within prob_tol of the fp64 softmax;
    logprob and free_logprob within lp_tol; where the optimum stands more than 10 vit_tol above the best path with a different
    collapse -- or the caller vouches that the logits are exact in fp32 and their sums in fp64 (exact_logits), so that the fp64
    recursion with the rule's tie order IS the rule -- idx is the fp64 path itself.  An unmatched pattern line reports 0, -inf, -inf and its free_logprob, and keeps its
    input rows bit for bit; a line of pattern 0 keeps its rows and its four canaries.  Returns (worst Viterbi deviation, worst
    |prob - fp64|, worst logprob deviation, matched lines, lines held to the exact path, unmatched pattern lines)."""
    ref = new_outputs(tpl, idx0, prob0)
    lp64 = LR.logp64(l64) if sum(tpl) else l64
    wv = wp = wl = 0.0
    n_matched = n_exact = n_unmatched = 0
    o = 0
    for i, (T, k) in enumerate(zip(tpl, line_pat)):
        w = (what, "line", i, "T", T, "pattern", k)
        idx, prob = out["idx"][o:o + T], out["prob"][o:o + T]
        keeps_rows = lambda: idx.tobytes() == ref["idx"][o:o + T].tobytes() and prob.tobytes() == ref["prob"][o:o + T].tobytes()
        if k == 0:
            assert keeps_rows(), (w, "rows of a line without a pattern written")
            for key in ("matched", "vit", "logprob", "free"):
                assert out[key][i].tobytes() == ref[key][i].tobytes(), (w, key, "of a line without a pattern written")
            o += T
            continue
        pat = pats[k - 1]
        l = l64[o:o + T]
        opt, path = viterbi64(l, pat.auto) if T else (NINF, None)
        free = float(np.sum(l.max(axis=1) - (l[np.arange(T), 0] - lp64[o:o + T, 0]))) if T else 0.0
        assert abs(float(out["free"][i]) - free) <= lp_tol, (w, "free_logprob", float(out["free"][i]), free)
        wl = max(wl, abs(float(out["free"][i]) - free))
        if path is None:
            n_unmatched += 1
            assert int(out["matched"][i]) == 0, (w, "an infeasible line is matched")
            assert out["vit"][i] == NINF and out["logprob"][i] == NINF, (w, "vit / logprob of an unmatched line")
            assert keeps_rows(), (w, "rows of an unmatched line written")
            o += T
            continue
        n_matched += 1
        assert int(out["matched"][i]) == 1, (w, "a feasible line is not matched", int(out["matched"][i]))
        assert ((idx >= 0) & (idx < l64.shape[1])).all(), (w, "classes outside [0, N)", idx.tolist())
        got = collapse(idx)
        assert pat.accepts(got), (w, "the collapse is not accepted", got)
        score = float(sum(l[t, idx[t]] for t in range(T)))
        dv = max(opt - score, abs(float(out["vit"][i]) - score))
        wv = max(wv, dv)
        assert score >= opt - vit_tol, (w, "path score below the optimum", score, opt, vit_tol)
        assert abs(float(out["vit"][i]) - score) <= vit_tol, (w, "vit_out", float(out["vit"][i]), score, vit_tol)
        dp = float(np.abs(prob.astype(np.float64) - np.exp(lp64[o + np.arange(T), idx])).max())
        wp = max(wp, dp)
        assert dp <= prob_tol, (w, "prob", dp, prob_tol)
        lse_sum = float(np.sum(l[np.arange(T), 0] - lp64[o:o + T, 0]))
        dl = abs(float(out["logprob"][i]) - (score - lse_sum))
        wl = max(wl, dl)
        assert dl <= lp_tol, (w, "logprob", float(out["logprob"][i]), score - lse_sum, lp_tol)
        second = viterbi64(l, differing(pat.auto, collapse(path)), want_path=False)[0]
        if exact_logits or opt - second > 10 * vit_tol:
            n_exact += 1
            assert idx.tolist() == path, (w, "path", idx.tolist(), path, opt - second)
        o += T
    return wv, wp, wl, n_matched, n_exact, n_unmatched


def figures(out, l64, tpl, line_pat, pats):
    """(worst Viterbi deviation, worst |prob - fp64|, worst logprob / free_logprob deviation) over the pattern lines, without
    asserting anything: what a test prints before it checks"""
    lp64 = LR.logp64(l64) if sum(tpl) else l64
    wv = wp = wl = 0.0
    o = 0
    for i, (T, k) in enumerate(zip(tpl, line_pat)):
        idx = out["idx"][o:o + T]
        if k and T:
            l = l64[o:o + T]
            lse = l[np.arange(T), 0] - lp64[o:o + T, 0]
            wl = max(wl, abs(float(out["free"][i]) - float(np.sum(l.max(axis=1) - lse))))
            if out["matched"][i] == 1 and ((idx >= 0) & (idx < l64.shape[1])).all():
                opt = viterbi64(l, pats[k - 1].auto, want_path=False)[0]
                score = float(sum(l[t, idx[t]] for t in range(T)))
                wv = max(wv, opt - score, abs(float(out["vit"][i]) - score))
                wp = max(wp, float(np.abs(out["prob"][o:o + T].astype(np.float64) - np.exp(lp64[o + np.arange(T), idx])).max()))
                wl = max(wl, abs(float(out["logprob"][i]) - (score - float(np.sum(lse)))))
        o += T
    return wv, wp, wl


# ---- a float32 stand-in of the hook, and its mutants -----------------------------------------------------------------------
def stand_in(z, W, b, tpl, line_pat, pats, mutant=None, idx0=None, prob0=None):
    """What a correct implementation returns (the rule in float32, plain loops over this file's own DFA), or -- mutant -- one of
    the wrong ones."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    out = new_outputs(tpl, idx0, prob0)
    l = (np.asarray(z, f) @ np.asarray(W, f) + np.asarray(b, f)).astype(f)
    mx = l.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(l - mx).sum(axis=1, keepdims=True, dtype=f))).astype(f)[:, 0]
    ninf = f(-np.inf)
    o = 0
    for i, (T, k) in enumerate(zip(tpl, line_pat)):
        if k == 0:
            if mutant == "other_line_written" and T:
                out["idx"][o] = 0
            o += T
            continue
        A = pats[k - 1].auto
        S, P = A.S, A.P
        pc, pq = A.pair_c, A.pair_q
        preds = [A.e_src[A.e_pair == p].tolist() for p in range(P)]
        out["free"][i] = f(sum((f(mx[o + t, 0] - lse[o + t]) for t in range(T)), f(0)))
        out["matched"][i] = 0; out["vit"][i] = ninf; out["logprob"][i] = ninf
        if T < 1:
            continue

        def tops(Cv):
            res = []
            for q in range(S):
                v1 = v2 = ninf; a1 = a2 = -1
                for p in range(int(A.seg[q]), int(A.seg[q + 1])):
                    v = Cv[p]
                    gt = (lambda x, y: x >= y) if mutant == "ties_to_highest_class" else (lambda x, y: x > y)
                    if v > ninf and gt(v, v1):
                        v2, a2, v1, a1 = v1, a1, v, p
                    elif v > ninf and gt(v, v2):
                        v2, a2 = v, p
                if mutant == "val2_not_excluding":
                    v2, a2 = v1, a1
                res.append((v1, a1, v2, a2))
            return res

        B = [l[o, 0] if q == 0 else ninf for q in range(S)]
        Cv = [l[o, pc[p]] if 0 in preds[p] else ninf for p in range(P)]
        bps = [None]
        for t in range(1, T):
            tp = tops(Cv)
            nC, nB, row = [], [], {}
            for p in range(P):
                c = pc[p]
                best, code = Cv[p], -1
                for q in preds[p]:
                    v1, a1, v2, a2 = tp[q]
                    other = mutant == "exclusion_dropped" or a1 < 0 or pc[a1] != c
                    cand, ca = (v1, a1) if other else (v2, a2)
                    v, kc = B[q], -(q + 2)
                    if cand > v:
                        v, kc = cand, ca
                    if v > best or (mutant == "enter_before_stay" and v == best and v > ninf):
                        best, code = v, kc
                nC.append(f(l[o + t, c] + best)); row[p] = code
            for q in range(S):
                best, code = B[q], -1
                if tp[q][0] > best:
                    best, code = tp[q][0], tp[q][1]
                nB.append(f(l[o + t, 0] + best)); row[-(q + 2)] = code
            B, Cv = nB, nC
            bps.append(row)
        tp = tops(Cv)
        best, node = ninf, None
        for q in range(S):
            if not (A.accept[q] or mutant == "end_over_all_states"):
                continue
            if B[q] > best:
                best, node = B[q], -(q + 2)
            if tp[q][0] > best:
                best, node = tp[q][0], tp[q][1]
        if node is None:
            o += T
            continue
        out["matched"][i] = 1; out["vit"][i] = best
        out["logprob"][i] = f(best - sum((lse[o + t] for t in range(T)), f(0)))
        for t in range(T - 1, -1, -1):
            c = 0 if node < 0 else int(pc[node])
            out["idx"][o + t] = c
            if mutant == "prob_restricted_softmax":
                allowed = sorted(set(pc.tolist()) | {0})
                out["prob"][o + t] = f(np.exp(l[o + t, c]) / np.exp(l[o + t, allowed]).sum())
            else:
                out["prob"][o + t] = f(np.exp(f(l[o + t, c] - lse[o + t])))
            if t > 0 and bps[t][node] != -1:
                node = bps[t][node]
        o += T
    return out

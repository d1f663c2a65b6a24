"""fp64 reference, float32 stand-in, numpy mutants, the cases and the check for the fused CTC head: nn::gemm with Epilogue::am_*
set (k_gemm<8, 1>, or k_gemm_wide<.., EPIM> behind argmax forms 1 and 2) followed by k_argmax_merge, driven one launch at a time
through rt_debug_gemm (tests/test_gpu_ctc_head.py on the GPU, tests/test_ctc_head_checks_cpu.py here).  Plain numpy, no device.

The head returns, per row of A [M][120], the class of the largest logit l = A W + bias (first maximum) and softmax(l)[that class]
= 1 / sum_c exp(l_c - max); the logits themselves never reach memory, so these two numbers are all a test can see.

How a row's classes map onto the kernels (nn_kernels.hip), which is what the planted ties below are placed against: a workgroup
takes a tile of 128 columns (form 0 and 2) or 240 columns (form 1); inside it a wave takes all 128 (form 0), 64 (form 2: two
waves) or 80 (form 1: three waves) consecutive columns in 16-column groups; inside a group lane quarter q = (col % 16) // 4 holds
columns 4 q .. 4 q + 3.  The maximum is folded in the lane over its groups in ascending order, then over the four quarters by two
__shfl_xor stages, then over the waves through LDS (forms 1 and 2), then over the tiles by k_argmax_merge.  Every stage must let
the lowest column win a tie.  Columns N .. round_up(N, 16) are pad: zero weights and zero bias, skipped by `col + j >= N`.

check() holds a launch's (idx, prob) to reference():
  * 0 <= idx < N;
  * idx = the fp64 argmax wherever the fp64 maximum beats the next distinct value by more than 2 B, B = the row's largest element
    bound 2^-24 (K + 8) (|a| . |w| + |bias|) (the bound of tests/test_gpu_ops.py); a maximum shared by bit-equal columns (a planted
    set) counts as one value and the lowest of them is the argmax; elsewhere idx is a class within 2 B of the maximum;
  * |prob / ref - 1| <= TOL_PROB per row; on the all-equal cases prob is float32(1 / N) within 4 ulp (every term is exp(0) = 1 and
    every partial sum an integer below 2^24, so the sum is N exactly and only the reciprocal rounds); on the large-logit case
    prob is finite and in (0, 1].

TOL_PROB = min(4 * MEASURED_STANDIN, 1.2e-5): standin() takes the fp64 logits rounded once to float32 and does max, exp, sum (class
by class, one float32 add each) and reciprocal in float32; its worst relative deviation from fp64 over the class-count cases is
MEASURED_STANDIN = 5.73e-6 (test_ctc_head_checks_cpu.py reproduces the figure).  The device sums in another order (lane, quarter,
wave, tile), accumulates the logits in fp32 and uses __expf; four is the margin the beam tolerances of this project give a plain
fp32 restatement, but 4 x 5.73e-6 is past the 1.2e-5 the tolerance may not exceed, so the cap binds: TOL_PROB = 1.2e-5, 2.1 times
the stand-in's own deviation.

Worst |prob / ref - 1| of the device per class count, M = 300, worst of the three forms (measured on an MI355X): N = 1: 0,
2: 3.9e-7, 3: 4.6e-7, 4: 4.2e-7, 5: 6.7e-7, 16: 1.1e-6, 17: 1.2e-6, 97: 1.6e-6, 127: 1.9e-6, 128: 2.0e-6, 129: 1.7e-6, 240: 2.1e-6,
241: 2.5e-6, 18385: 2.9e-6; row-count cases up to 2.5e-6, the tie case 1.7e-6, all-negative 1.3e-6; the large-logit case, which
is not held to TOL_PROB, 1.5e-5.  The device needed no term beyond TOL_PROB."""
import functools

import numpy as np

U = 2.0 ** -24
K = 120
TILE = 128
CLASS_COUNTS = (1, 2, 3, 4, 5, 16, 17, 97, 127, 128, 129, 240, 241, 18385)
ROW_COUNTS = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257)
ROW_COUNT_CLASSES = (97, 129)
EQUAL_COUNTS = (3, 97, 129, 6625)
NEGATIVE_COUNTS = (5, 97, 129)
TIE_N, TIE_M, TIE_ROWS_PER_SET = 400, 300, 8
TIE_SETS = ((8, 9), (40, 56), (64, 68), (80, 88), (28, 32), (20, 100), (70, 170), (110, 140), (230, 250), (300, 390), (150, 399),
            (0, 200), (5, 133, 261, 389))
MEASURED_STANDIN = 5.73e-6   # worst |standin prob / fp64 prob - 1| over CLASS_COUNTS at M = 300 (at N = 18385; 9.0e-7 at N = 240)
TOL_PROB = min(4 * MEASURED_STANDIN, 1.2e-5)   # (the cap binds)
MIN_DECISIVE = 0.98
NO_CLASS = 0x7fffffff   # what the kernels' running argmax starts as


def round_up(n, m):
    return (n + m - 1) // m * m


def operands(M, N, seed):
    """A [M][K] uniform(-1, 1), W [K][N] uniform(-1, 1) * 4 / sqrt(K), bias uniform(-1, 1): test_gpu_ops._operands with lda = K"""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = (rng.uniform(-1, 1, (K, N)) * (4.0 / np.sqrt(K))).astype(np.float32)
    bias = rng.uniform(-1, 1, N).astype(np.float32)
    return A, W, bias


def _product64(a, w):
    """a @ w in fp64, added up k by k: every column is treated alike, so bit-equal columns of w give bit-equal results (a BLAS
    product may take the columns of a partial block in another order)"""
    out = np.zeros((a.shape[0], w.shape[1]))
    for k in range(a.shape[1]):
        out += a[:, k:k + 1] * w[k]
    return out


def reference(A, W, bias):
    """(fp64 logits [M][N], the row's largest element bound [M], the fp64 argmax (first maximum) [M], 1 / sum exp(l - max) [M])"""
    a, w, b = A.astype(np.float64), W.astype(np.float64), bias.astype(np.float64)
    logits = _product64(a, w) + b
    bound = (U * (K + 8) * (np.abs(a) @ np.abs(w) + np.abs(b))).max(1)
    top = np.argmax(logits, 1)
    prob = 1.0 / np.exp(logits - logits.max(1, keepdims=True)).sum(1)
    return logits, bound, top, prob


def logits32(A, W, bias):
    """the fp64 logits rounded once to float32: bit-equal columns of W and bias give bit-equal logits"""
    return (_product64(A.astype(np.float64), W.astype(np.float64)) + bias.astype(np.float64)).astype(np.float32)


def _sum32(e):
    """row sums in column order, one float32 add per class, as a plain loop has them (np.sum would add pairwise)"""
    return np.cumsum(e, axis=1, dtype=np.float32)[:, -1]


def _head32(l):
    """first maximum and 1 / sum exp(l - max) of float32 logits, all in float32"""
    m = l.max(1, keepdims=True)
    return np.argmax(l, 1).astype(np.int32), (np.float32(1) / _sum32(np.exp(l - m))).astype(np.float32)


def standin(A, W, bias, l=None):
    """a correct head in float32: (idx, prob); l = logits32(A, W, bias) where the caller has them"""
    return _head32(logits32(A, W, bias) if l is None else l)


MUTANTS = ("tie_to_higher", "tie_by_quarter", "tiles_merged_with_ge", "pad_columns_take_part", "last_tile_dropped",
           "sum_of_winning_tile_only", "sum_not_rescaled")


def _tile_stats(l):
    """per 128-column tile: (max [M][T], first column of it [M][T], sum exp(l - tile max) [M][T]) in float32"""
    N = l.shape[1]
    ms, idxs, sums = [], [], []
    for t0 in range(0, N, TILE):
        part = l[:, t0:t0 + TILE]
        m = part.max(1)
        ms.append(m)
        idxs.append(np.argmax(part, 1) + t0)
        sums.append(_sum32(np.exp(part - m[:, None])))
    return np.stack(ms, 1), np.stack(idxs, 1), np.stack(sums, 1)


def mutant(name, A, W, bias, l=None):
    """the head restated wrongly in numpy: (idx, prob)"""
    l = logits32(A, W, bias) if l is None else l
    M, N = l.shape
    idx, prob = _head32(l)
    rows = np.arange(M)
    if name == "tie_to_higher":          # the last maximum wins
        return (N - 1 - np.argmax(l[:, ::-1], 1)).astype(np.int32), prob
    if name == "tie_by_quarter":         # lane-quarter order taken for column order
        col = np.arange(N)
        key = ((col % 16) // 4) * round_up(N, 16) + col
        tied = l == l.max(1, keepdims=True)
        return np.argmin(np.where(tied, key[None, :], np.iinfo(np.int64).max), 1).astype(np.int32), prob
    if name == "pad_columns_take_part":  # columns N .. round_up(N, 16) join with logit 0
        ext = np.concatenate([l, np.zeros((M, round_up(N, 16) - N), np.float32)], 1)
        return _head32(ext)
    if name == "last_tile_dropped":
        keep = (N - 1) // TILE * TILE
        if keep == 0:                    # nothing left: the running argmax is never set, the sum stays 0
            with np.errstate(divide="ignore"):
                return np.full(M, NO_CLASS, np.int32), np.float32(1) / np.zeros(M, np.float32)
        return _head32(l[:, :keep])
    tm, ti, ts = _tile_stats(l)
    if name == "tiles_merged_with_ge":   # first maximum within a tile, but a later tile wins a tie
        t = tm.shape[1] - 1 - np.argmax(tm[:, ::-1], 1)
        return ti[rows, t].astype(np.int32), prob
    if name == "sum_of_winning_tile_only":
        t = np.argmax(tm, 1)
        return idx, (np.float32(1) / ts[rows, t]).astype(np.float32)
    if name == "sum_not_rescaled":       # tile sums added without exp(m_t - m)
        return idx, (np.float32(1) / _sum32(ts)).astype(np.float32)
    raise KeyError(name)


# ----------------------------------------------------------------------------------------------------------------------------
class Case:
    """One launch: A [M][K] (lda = K), W [K][N], bias [N].  sets: groups of classes whose W columns and bias entries are
    bit-equal; planted: (set, rows) -- the rows built to make that set the clear joint maximum.  prob_rule: "rel" (TOL_PROB),
    "ulp" (float32(1 / N) within 4 ulp) or "finite"."""

    def __init__(self, name, A, W, bias, sets=(), planted=(), prob_rule="rel"):
        self.name, self.A, self.W, self.bias = name, A, W, bias
        self.M, self.N = A.shape[0], W.shape[1]
        self.sets, self.planted, self.prob_rule = tuple(sets), tuple(planted), prob_rule
        self._ref = None

    def ref(self):
        """reference() plus, per row: the margin of the maximum over the next distinct value (0 where the maximum is shared by
        columns that are not one bit-equal set) and the classes within 2 B of the maximum"""
        if self._ref is None:
            logits, bound, top, prob = reference(self.A, self.W, self.bias)
            mx = logits.max(1, keepdims=True)
            tied = logits == mx
            with np.errstate(invalid="ignore"):
                margin = mx[:, 0] - np.where(tied, -np.inf, logits).max(1)     # inf where every class holds the maximum
            gid = np.full(self.N, -1)
            for g, s in enumerate(self.sets):
                gid[list(s)] = g
            one_set = (gid[top] >= 0) & ((tied & (gid[None, :] == gid[top][:, None])).sum(1) == tied.sum(1))
            margin = np.where((tied.sum(1) == 1) | one_set, margin, 0.0)
            self._ref = dict(logits=logits, bound=bound, top=top, prob=prob, margin=margin, near=logits >= mx - 2 * bound[:, None])
        return self._ref

    def standin(self):
        return standin(self.A, self.W, self.bias, self.ref()["logits"].astype(np.float32))

    def mutant(self, name):
        return mutant(name, self.A, self.W, self.bias, self.ref()["logits"].astype(np.float32))

    def decisive(self):
        r = self.ref()
        return r["margin"] > 2 * r["bound"]


def violations(case, idx, prob):
    """what check() refuses, as {rule: rows}"""
    r = case.ref()
    idx, prob = np.asarray(idx).astype(np.int64), np.asarray(prob, np.float32)
    assert idx.shape == prob.shape == (case.M,)
    rows = np.arange(case.M)
    out = {}
    inside = (idx >= 0) & (idx < case.N)
    out["idx outside 0 .. N - 1"] = rows[~inside]
    safe = np.where(inside, idx, 0)
    dec = case.decisive()
    out["idx is not the fp64 argmax on a decisive row"] = rows[inside & dec & (idx != r["top"])]
    out["idx is no class within 2 B of the maximum"] = rows[inside & ~dec & ~r["near"][rows, safe]]
    tie = "idx is not the lowest class of the planted tie"
    for s, prows in case.planted:
        bad = np.asarray(prows)[idx[list(prows)] != min(s)]
        out[tie] = np.concatenate([out.get(tie, np.zeros(0, np.int64)), bad])
    p64 = prob.astype(np.float64)
    if case.prob_rule == "ulp":
        want = np.float32(1) / np.float32(case.N)
        bad = ~(np.abs(p64 - float(want)) <= 4 * float(np.spacing(want)))
        out["prob is not float32(1 / N) within 4 ulp"] = rows[bad]
    elif case.prob_rule == "finite":
        out["prob is not finite and in (0, 1]"] = rows[~(np.isfinite(p64) & (p64 > 0) & (p64 <= 1))]
    else:
        out["prob outside TOL_PROB"] = rows[~(np.abs(p64 / r["prob"] - 1) <= TOL_PROB)]
    return {k: np.unique(v) for k, v in out.items() if len(v)}


def deviation(case, prob):
    """worst |prob / ref - 1| over the rows"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return float(np.max(np.abs(np.asarray(prob, np.float64) / case.ref()["prob"] - 1)))


def check(case, idx, prob):
    assert case.decisive().mean() >= MIN_DECISIVE, "%s: decisive share %.3f" % (case.name, case.decisive().mean())
    bad = violations(case, idx, prob)
    assert not bad, "%s: %s" % (case.name, "; ".join("%s: %d rows (first %d, idx %d prob %.9g, fp64 argmax %d prob %.9g)" % (
        k, len(v), v[0], np.asarray(idx)[v[0]], np.asarray(prob)[v[0]], case.ref()["top"][v[0]], case.ref()["prob"][v[0]])
        for k, v in bad.items()))


def planted_sets_hit(case, rows):
    """the planted sets that own any of `rows`"""
    rows = set(int(r) for r in rows)
    return [s for s, prows in case.planted if rows & set(prows)]


# ----------------------------------------------------------------------------------------------------------------------------
def _class_count(N, M=300, scale=1.0):
    A, W, bias = operands(M, N, seed=1000 + N if M == 300 else 5000 + 1000 * N + M)
    return A * np.float32(scale), W, bias


def _ties():
    """N = 400: three full 128-column tiles plus a 16-column one (two 240-column tiles in form 1).  Every TIE_SETS entry gets
    bit-equal W columns and bias entries and eight rows s * W[:, a], s in [1, 2], which make it the joint maximum: the set's
    logit is s |W_a|^2 + b_a = 5.3 s + b_a against 0.49 s z + b_c (z about normal) for every other class."""
    A, W, bias = operands(TIE_M, TIE_N, seed=77)
    rng = np.random.default_rng(78)
    planted = []
    for k, s in enumerate(TIE_SETS):
        for c in s[1:]:
            W[:, c], bias[c] = W[:, s[0]], bias[s[0]]
        rows = [(11 + 37 * (TIE_ROWS_PER_SET * k + j)) % TIE_M for j in range(TIE_ROWS_PER_SET)]   # (37 and 300 are coprime)
        for r in rows:
            A[r] = np.float32(rng.uniform(1, 2)) * W[:, s[0]]
        planted.append((s, tuple(rows)))
    return Case("ties N400", A, W, bias, sets=TIE_SETS, planted=planted)


def _equal(N):
    A = np.zeros((64, K), np.float32)
    W = operands(1, N, seed=2000 + N)[1]
    every = tuple(range(N))
    return Case("all equal N%d" % N, A, W, np.full(N, 0.75, np.float32), sets=(every,), planted=((every, tuple(range(64))),),
                prob_rule="ulp")


def _negative(N):
    A, W, bias = operands(300, N, seed=3000 + N)
    return Case("all negative N%d" % N, A * np.float32(0.25), W, np.full(N, -20.0, np.float32))


_BUILDERS = {}
for _n in CLASS_COUNTS:
    _BUILDERS["classes-N%d" % _n] = functools.partial(lambda n: Case("classes N%d M300" % n, *_class_count(n)), _n)
for _n in ROW_COUNT_CLASSES:
    for _m in ROW_COUNTS:
        _BUILDERS["rows-N%d-M%d" % (_n, _m)] = functools.partial(
            lambda n, m: Case("rows N%d M%d" % (n, m), *_class_count(n, m)), _n, _m)
_BUILDERS["ties-N400"] = _ties
for _n in EQUAL_COUNTS:
    _BUILDERS["equal-N%d" % _n] = functools.partial(_equal, _n)
for _n in NEGATIVE_COUNTS:
    _BUILDERS["negative-N%d" % _n] = functools.partial(_negative, _n)
_BUILDERS["large-N97"] = lambda: Case("large logits N97 M300", *_class_count(97, scale=40.0), prob_rule="finite")
CASE_IDS = list(_BUILDERS)
CLASS_COUNT_IDS = ["classes-N%d" % n for n in CLASS_COUNTS]


@functools.lru_cache(maxsize=None)
def case(case_id):
    return _BUILDERS[case_id]()

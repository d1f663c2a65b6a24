"""Rec flip (retto_amd/csrc/rec_flip.h) restated in numpy, independently of the C++: the choice between the two views, two
mutants of it that the CPU tests must tell from the rule, the greedy CTC score of one view (k_ctc_decode's arithmetic: the kept
count, an fp32 sum in step order, one division), the both-ways predicate and the 180-degree rotation of a crop and of a packed
list of crops."""
import numpy as np

ONE_WAY, KEPT_0, TOOK_1 = 0, 1, 2


def choose(ntok0, score0, ntok1, score1):
    """1 when view 1 is taken: it kept a token, and view 0 kept none or score1 > score0 in fp32; a tie or a NaN keeps view 0"""
    if ntok1 <= 0:
        return 0
    if ntok0 <= 0:
        return 1
    return 1 if bool(np.float32(score1) > np.float32(score0)) else 0


def choose_ge(ntok0, score0, ntok1, score1):
    """MUTANT: >= for >, so a tie takes view 1"""
    if ntok1 <= 0:
        return 0
    if ntok0 <= 0:
        return 1
    return 1 if bool(np.float32(score1) >= np.float32(score0)) else 0


def choose_ignores_ntok(ntok0, score0, ntok1, score1):
    """MUTANT: the token counts are not read"""
    return 1 if bool(np.float32(score1) > np.float32(score0)) else 0


def _ulp(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf), dtype=np.float32)


def grid():
    """(ntok0, score0, ntok1, score1): zero tokens on either side or both, equal scores, NaN on either side, score1 one ulp above
    and one ulp below score0, and a spread of ordinary values"""
    nan = np.float32(np.nan)
    scores = [np.float32(v) for v in (0.0, 1e-6, 0.25, 0.5, 0.75, 0.99999994, 1.0)]
    out = []
    for n0 in (0, 1, 7):
        for n1 in (0, 1, 7):
            for s0 in scores + [nan]:
                cands = scores + [nan]
                if not np.isnan(s0):
                    cands = cands + [s0, _ulp(s0, True), _ulp(s0, False)]
                for s1 in cands:
                    out.append((n0, np.float32(s0), n1, np.float32(s1)))
    return out


def score(idx, prob):
    """(kept tokens, greedy score) of one view's rows, as k_ctc_decode computes them: a step is kept when its class is not the
    blank and differs from the step before; the kept probabilities are summed sequentially in fp32 in step order and divided by
    the count once (0 / 0 = NaN)"""
    idx = np.asarray(idx); prob = np.asarray(prob, np.float32)
    cnt = 0
    acc = np.float32(0.0)
    for t in range(len(idx)):
        if idx[t] != 0 and (t == 0 or idx[t] != idx[t - 1]):
            acc = np.float32(acc + prob[t]); cnt += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return cnt, np.float32(acc / np.float32(cnt))


def both_ways(cls_score, cls_below):
    cls_below = np.float32(cls_below)
    if not cls_below > 0:
        return False
    return bool(cls_below > np.float32(1.0)) or bool(np.float32(cls_score) < cls_below)


def rotate180(crop):
    """pixel (y, x) -> (h - 1 - y, w - 1 - x)"""
    return np.ascontiguousarray(crop[::-1, ::-1])


def pattern_crops(sizes):
    """the crops of the stand-alone driver's rotate query: byte i of the packed pool is (i * 7 + 3) mod 256"""
    total = sum(h * w * 3 for h, w in sizes)
    pool = ((np.arange(total, dtype=np.int64) * 7 + 3) % 256).astype(np.uint8)
    crops, o = [], 0
    for h, w in sizes:
        crops.append(pool[o:o + h * w * 3].reshape(h, w, 3)); o += h * w * 3
    return crops


def fnv1a(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h

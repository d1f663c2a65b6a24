"""The page deskew rule (estimate a page's skew from shifted row profiles of its ink grid, rotate it back) in numpy with int64 and
Python ints, written from the rule's text in retto_amd/csrc/page_deskew.h, not from its C++; plus the pages and case tables the
two test files share."""
import math

import numpy as np


def ink_grid(img):
    """I [gh, gw]: 255 - the minimum luma of each c x c cell (edge cells partial), c = 4 doubled until the grid is <= 512 cells"""
    img = np.asarray(img, np.int64); h, w = img.shape[:2]
    luma = (77 * img[..., 0] + 150 * img[..., 1] + 29 * img[..., 2] + 128) >> 8
    c = 4
    while -(-max(h, w) // c) > 512:
        c *= 2
    gh, gw = -(-h // c), -(-w // c)
    padded = np.full((gh * c, gw * c), 255, np.int64); padded[:h, :w] = luma
    return 255 - padded.reshape(gh, c, gw, c).min(axis=(1, 3))


def scores(I, K):
    """S_k for k = -K .. K as Python ints"""
    gh, gw = I.shape
    gy, gx = np.arange(gh)[:, None], np.arange(gw)[None, :]
    out = []
    for k in range(-K, K + 1):
        d = ((gx - gw // 2) * k * 128 + 32768) >> 16
        rows = gy + d
        P = np.zeros(rows.max() - rows.min() + 3, np.int64)   # a zero row at either end
        np.add.at(P, (rows - rows.min() + 1).ravel(), I.ravel())
        out.append(int((np.diff(P) ** 2).sum()))
    return out


def choose(S, K, min_gain):
    best = max(range(-K, K + 1), key=lambda k: (S[k + K], -abs(k), k))
    return 0 if S[best + K] * 100 < S[K] * (100 + min_gain) else best


def angle(k):
    """(cosq, sinq) of slope k / 512 in units of 2^-16"""
    a = abs(k); r = math.isqrt((512 * 512 + a * a) << 16)
    s = (a * (1 << 24) + r // 2) // r
    return (512 * (1 << 24) + r // 2) // r, s if k >= 0 else -s


def turn(img, k):
    if k == 0:
        return np.array(img, np.uint8)
    img = np.asarray(img, np.int64); h, w = img.shape[:2]
    cosq, sinq = angle(k)
    dx, dy = (2 * np.arange(w, dtype=np.int64) - (w - 1))[None, :], (2 * np.arange(h, dtype=np.int64) - (h - 1))[:, None]
    U = cosq * dx + sinq * dy + (w - 1) * 65536
    V = -sinq * dx + cosq * dy + (h - 1) * 65536
    u0, fu, v0, fv = U >> 17, ((U >> 9) & 255)[..., None], V >> 17, ((V >> 9) & 255)[..., None]
    x0, x1, y0, y1 = np.clip(u0, 0, w - 1), np.clip(u0 + 1, 0, w - 1), np.clip(v0, 0, h - 1), np.clip(v0 + 1, 0, h - 1)
    out = ((256 - fu) * (256 - fv) * img[y0, x0] + fu * (256 - fv) * img[y0, x1] + (256 - fu) * fv * img[y1, x0]
           + fu * fv * img[y1, x1] + 32768) >> 16
    return out.astype(np.uint8)


def deskew(img, K, min_gain, S=None):
    """(deskewed page, slope, scores); S: the scores of an earlier call on the same page and range"""
    S = scores(ink_grid(img), K) if S is None else S
    k = choose(S, K, min_gain)
    return turn(img, k), k, S


def matrix(k, h, w):
    """the affine of rt_results_page_deskew: a point of the deskewed page -> the original page, [a b c; d e f] row-major"""
    cosq, sinq = angle(k) if k else (65536, 0)
    cs, sn, cx, cy = cosq / 65536.0, sinq / 65536.0, (w - 1) / 2.0, (h - 1) / 2.0
    return np.array([cs, sn, cx - cs * cx - sn * cy, -sn, cs, cy + sn * cx - cs * cy], np.float32)


def page(kind, h, w, seed=0):
    """the test pages: an int = text lines (pitch 28 px, half of it tall, ragged: 30 % of a line's pixels ink at 40 on paper at 230
    -- solid bands alias with the 4-pixel cells at slopes like 3 / 16) rising to the right by kind / 512; "uniform"; "noise" """
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return np.full((h, w, 3), 200, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    line = ((y * 512 + int(kind) * (x - w // 2)) // 512) % 28 < 14
    ink = np.where(line & (rng.random((h, w)) < 0.3), 40, 230)
    return np.stack([ink, ink - 10, ink - 25], axis=2).astype(np.uint8)


# (h, w): one partial tile everywhere and an odd grid width; row bytes off the dword grid; more than one column band and many
# rotate tiles; c = 8 and the longest row registers
SHAPES = ((37, 53), (203, 291), (130, 1030), (2100, 90))
# planted slopes (-100 is outside range 16; 0 and the uniform page make every S_k that matters equal: the tie rule), noise
KINDS = (-100, -23, 7, 0, "uniform", "noise")
RANGES = (16, 128)
GAINS = (0, 50)

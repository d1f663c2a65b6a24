"""The page flatten rule (divide every channel by its estimated paper level) in numpy with int64, written from the rule's text in
retto_amd/csrc/page_flatten.h, not from its C++; plus the pages the two test files share."""
import numpy as np


def window(a, r, op):
    """op over the (2 r + 1)^2 window clipped to the grid, around every cell of a [gh, gw]"""
    a = np.stack([op(a[max(0, j - r):j + r + 1], axis=0) for j in range(a.shape[0])])
    return np.stack([op(a[:, max(0, i - r):i + r + 1], axis=1) for i in range(a.shape[1])], axis=1)


def flatten(img, radius, floor, level=None):
    """img [h, w, 3] uint8 -> (flattened page, level B [3, gh, gw] uint8); level: B of an earlier call on the same page and radius"""
    img = np.asarray(img, np.int64); h, w = img.shape[:2]; r = int(radius)
    gh, gw = -(-h // 4), -(-w // 4)
    n = window(np.ones((gh, gw), np.int64), r, np.sum)

    def along(count, g):   # per coordinate: the two cells and the weight of the second
        u = 2 * np.arange(count) - 3
        first = (g == 1) | (u <= 0)
        i0 = np.where(first, 0, u // 8)
        last = ~first & (i0 >= g - 1)
        i0 = np.where(last, g - 1, i0)
        inner = ~first & ~last
        return i0, np.where(inner, i0 + 1, i0), np.where(inner, u - 8 * i0, 0)

    y0, y1, wy = (a[:, None] for a in along(h, gh))
    x0, x1, wx = (a[None, :] for a in along(w, gw))
    out = np.zeros_like(img); known = level is not None; level = np.array(level, np.int64) if known else np.zeros((3, gh, gw), np.int64)
    for ch in range(3):
        if not known:
            P = np.array([[img[4 * gy:4 * gy + 4, 4 * gx:4 * gx + 4, ch].max() for gx in range(gw)] for gy in range(gh)])
            C = window(window(P, r, np.max), r, np.min)
            level[ch] = (window(C, r, np.sum) + n // 2) // n
        B = level[ch]
        L = (8 - wy) * ((8 - wx) * B[y0, x0] + wx * B[y0, x1]) + wy * ((8 - wx) * B[y1, x0] + wx * B[y1, x1])
        L = np.maximum(L, 64 * int(floor))
        out[..., ch] = np.minimum(255, (img[..., ch] * 16320 + L // 2) // L)
    return out.astype(np.uint8), level.astype(np.uint8)


def page(kind, h, w, seed=0):
    """the test pages: noise, text (5 % at 60 on 240 under a left-to-right illumination ramp 255 -> 90 with a blue cast: the use
    case), white, black (the floor engages everywhere), colour (saturated channels)"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "text":
        ink = np.where(rng.random((h, w)) < 0.05, 60, 240)
        ramp = 255 - (165 * np.arange(w)) // max(w - 1, 1)
        return np.stack([ink * ramp * cast // (255 * 255) for cast in (200, 225, 255)], axis=2).astype(np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)   # colour
    img[..., 0] = np.where(rng.random((h, w)) < 0.5, 255, img[..., 0]); img[..., 2] = np.where(rng.random((h, w)) < 0.5, 0, img[..., 2])
    return img


KINDS = ("noise", "text", "white", "black", "colour")
# (radius, h, w): one cell; smaller than a cell; one-pixel partial cells; rows off the dword grid; the window taller than the grid;
# wider than the grid; several level tiles whose halos cross tile borders; the halo wider than a tile
SHAPES = ((1, 4, 4), (1, 3, 2), (1, 5, 9), (2, 33, 95), (16, 40, 300), (16, 300, 37), (3, 130, 262), (16, 200, 530))
FLOORS = (1, 64, 255)

"""The page enhance rule (tile-wise contrast-limited histogram equalisation of the luma) in numpy with int64, written from the
rule's text in retto_amd/csrc/page_enhance.h, not from its C++; plus the pages the two test files share."""
import numpy as np


def enhance(img, tile, clip):
    """img [h, w, 3] uint8 -> (enhanced page, luts [nty, ntx, 256] uint8)"""
    img = np.asarray(img, np.int64); h, w = img.shape[:2]; t = int(tile)
    clip_x16 = int(np.rint(np.float32(clip) * np.float32(16)))
    Y = (77 * img[..., 0] + 150 * img[..., 1] + 29 * img[..., 2] + 128) >> 8
    nty, ntx = -(-h // t), -(-w // t)
    luts = np.zeros((nty, ntx, 256), np.int64)
    for ty in range(nty):
        for tx in range(ntx):
            part = Y[ty * t:(ty + 1) * t, tx * t:(tx + 1) * t]
            area = part.size
            hist = np.bincount(part.ravel(), minlength=256)
            L = max(1, (clip_x16 * area) >> 12)
            excess = int(np.maximum(hist - L, 0).sum())
            hist = np.minimum(hist, L) + excess // 256
            r = excess % 256
            for k in range(r):
                hist[(k * 256) // r] += 1
            assert hist.sum() == area
            luts[ty, tx] = (np.cumsum(hist) * 255 + area // 2) // area

    def along(n, nt):   # per coordinate: the two tiles and the weight of the second
        u = 2 * np.arange(n) + 1 - t
        i0 = np.where((nt == 1) | (u <= 0), 0, u // (2 * t))
        last = i0 >= nt - 1
        i0 = np.where(last, nt - 1, i0)
        inner = ~last & ~((nt == 1) | (u <= 0))
        return i0, np.where(inner, i0 + 1, i0), np.where(inner, u - 2 * t * i0, 0)

    y0, y1, wy = (a[:, None] for a in along(h, nty))
    x0, x1, wx = (a[None, :] for a in along(w, ntx))
    top = (2 * t - wx) * luts[y0, x0, Y] + wx * luts[y0, x1, Y]
    bot = (2 * t - wx) * luts[y1, x0, Y] + wx * luts[y1, x1, Y]
    Yn = ((2 * t - wy) * top + wy * bot + 2 * t * t) // (4 * t * t)
    return np.clip(img + (Yn - Y)[..., None], 0, 255).astype(np.uint8), luts.astype(np.uint8)


def page(kind, h, w, seed=0):
    """the test pages: noise, gradient (horizontal), white (one bin), text (95 % at 240, 5 % at 60), colour (saturated channels)"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        return np.repeat(np.repeat(((np.arange(w) * 255) // max(w - 1, 1)).astype(np.uint8)[None, :, None], h, 0), 3, 2)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "text":
        return np.repeat(np.where(rng.random((h, w)) < 0.05, 60, 240).astype(np.uint8)[..., None], 3, 2)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)   # colour
    img[..., 0] = np.where(rng.random((h, w)) < 0.5, 255, img[..., 0]); img[..., 2] = np.where(rng.random((h, w)) < 0.5, 0, img[..., 2])
    return img


KINDS = ("noise", "gradient", "white", "text", "colour")
# (tile, h, w): one tile; one-pixel partial edge tiles with misaligned rows; whole tiles; several partial; smaller than a tile;
# tile 64 and tile 512
SHAPES = ((32, 32, 32), (32, 33, 95), (32, 64, 64), (32, 70, 130), (32, 31, 7), (64, 150, 201), (512, 520, 40))
CLIPS = (1.0, 2.5, 64.0)

"""Det tiles (retto_amd/csrc/det_tiles.h) restated independently in Python: the plan along one axis, the ownership bounds and
the stitch as a numpy selection.  Shared by tests/test_det_tiles_cpu.py and tests/test_gpu_det_tiles.py."""
import numpy as np


def accepted(T, O):
    """what rt_set_det_tiles / rt_det_tile_plan accept"""
    if T == 0:
        return O >= 0
    return T >= 64 and T % 32 == 0 and O >= 0 and O % 32 == 0 and 2 * O <= T


def axis_plan(L, T, O):
    """(tile length, origins, bounds) along an axis of length L; tile i owns [bounds[i - 1], bounds[i]) with bounds[-1] = 0"""
    if T == 0 or L <= T:
        return L, [0], [L]
    n = -(-(L - T) // (T - O)) + 1
    xs = [min(i * (T - O), L - T) for i in range(n)]
    bs = [(xs[i] + T + xs[i + 1]) // 2 for i in range(n - 1)] + [L]
    return T, xs, bs


def page_plan(H, W, T, O):
    """the plan of rt_det_tile_plan as retto_amd.det_tile_plan returns it (a page that fits into one tile comes out as one)"""
    th, ro, rb = axis_plan(H, T, O)
    tw, co, cb = axis_plan(W, T, O)
    return {"tile_h": th, "tile_w": tw, "row_origins": ro, "row_bounds": rb, "col_origins": co, "col_bounds": cb}


def check_axis(L, T, O, tlen, xs, bs):
    """the properties the issue states for one axis"""
    n = len(xs)
    assert len(bs) == n and bs[-1] == L and all(a < b for a, b in zip([0] + bs, bs)), (L, T, O, bs)   # a partition of [0, L)
    for i in range(n):
        assert 0 <= xs[i] and xs[i] + tlen <= L, (L, T, O, xs)                # inside the page
        lo = bs[i - 1] if i else 0
        assert xs[i] <= lo and bs[i] <= xs[i] + tlen, (L, T, O, i)            # a tile owns pixels of its own only
        assert bs[i] % 16 == 0, (L, T, O, bs)
    for i in range(n - 1):                                                    # an interior boundary: O / 2 inside both tiles
        assert bs[i] - xs[i + 1] >= O // 2 and xs[i] + tlen - bs[i] >= O // 2, (L, T, O, i)
        assert xs[i + 1] > xs[i], (L, T, O, xs)


def cut(img, plan):
    """the tiles of an [H, W, ...] array in plan order"""
    th, tw = plan["tile_h"], plan["tile_w"]
    return [img[y:y + th, x:x + tw] for y in plan["row_origins"] for x in plan["col_origins"]]


def stitch(tile_maps, plan, H, W):
    """page_map[y][x] = tile_map(ty(y), tx(x))[y - y0][x - x0]: a selection, no arithmetic"""
    out = np.full((H, W), np.nan, np.float32)
    nc = len(plan["col_origins"])
    for ty, y0 in enumerate(plan["row_origins"]):
        a0, a1 = (plan["row_bounds"][ty - 1] if ty else 0), plan["row_bounds"][ty]
        for tx, x0 in enumerate(plan["col_origins"]):
            b0, b1 = (plan["col_bounds"][tx - 1] if tx else 0), plan["col_bounds"][tx]
            out[a0:a1, b0:b1] = tile_maps[ty * nc + tx][a0 - y0:a1 - y0, b0 - x0:b1 - x0]
    return out

"""The rec window rule (retto_amd/csrc/rec_windows.h) restated in Python, independently of the C++: the plan along a line, its
properties, and the stitch as a numpy selection.  Shared by test_rec_windows_cpu.py and test_gpu_rec_windows.py."""
import numpy as np

STEP = 8


def tokens(L):
    """time steps of a rec line of L columns: two stride-2 convolutions (pad k // 2), then a pool of 2 without padding"""
    a = -(-L // 2)
    c = -(-a // 2)
    return c // 2


def accepted(window, overlap):
    if window == 0:
        return overlap >= 0
    return window >= 128 and window % 32 == 0 and overlap >= 0 and overlap % 32 == 0 and 2 * overlap <= window


def plan(L, window, overlap):
    """(origins, widths, bounds, T) of a line of L columns"""
    T = tokens(L)
    last = ((L - window) // STEP) * STEP
    if window == 0 or last <= 0:
        return [0], [L], [T], T
    S = window - overlap
    n = -(-last // S) + 1
    xs = [min(i * S, last) for i in range(n)]
    ws = [window] * (n - 1) + [L - xs[-1]]
    Tw = window // STEP
    cs = [(xs[i] // STEP + Tw + xs[i + 1] // STEP) // 2 for i in range(n - 1)] + [T]
    return xs, ws, cs, T


def as_dict(L, window, overlap):
    xs, ws, cs, T = plan(L, window, overlap)
    return {"T": T, "origins": xs, "widths": ws, "bounds": cs}


def check(L, window, overlap, xs, ws, cs, T):
    """the properties the header states, on a plan however it was made"""
    n = len(xs)
    assert len(ws) == n and len(cs) == n and n >= 1
    assert T == tokens(L)
    if n == 1:
        assert (xs, ws, cs) == ([0], [L], [T])
        assert window == 0 or L < window + STEP
        return
    assert L >= window + STEP
    assert xs[0] == 0 and all(x % STEP == 0 for x in xs) and all(b > a for a, b in zip(xs, xs[1:]))
    assert all(w == window for w in ws[:-1]) and ws[-1] == window + L % STEP
    assert all(x + w <= L for x, w in zip(xs, ws)) and xs[-1] + ws[-1] == L
    assert all(b - a <= window - overlap for a, b in zip(xs, xs[1:]))          # no stride beyond window - overlap
    assert xs[-1] // STEP + tokens(ws[-1]) == T                                 # the last unit ends at the line's last step
    lo = 0
    for i in range(n):
        m = xs[i] // STEP
        assert lo < cs[i], "an empty ownership interval"
        assert m <= lo and cs[i] <= m + tokens(ws[i]), "owned steps outside the unit"
        if i + 1 < n:   # an interior boundary lies at least overlap / 16 steps inside both units of its pair
            assert cs[i] - xs[i + 1] // STEP >= overlap // 16 and m + window // STEP - cs[i] >= overlap // 16
        lo = cs[i]
    assert cs[-1] == T                                                          # the intervals partition [0, T)


def owner(cs, t):
    for i, c in enumerate(cs):
        if t < c:
            return i
    raise AssertionError("step beyond the line")


def stitch(unit_rows, xs, cs, T):
    """the selection line_row[t] = unit_row(i(t))[t - m_i] over arrays whose first axis is the time step"""
    out = np.empty((T,) + unit_rows[0].shape[1:], unit_rows[0].dtype)
    lo = 0
    for i, c in enumerate(cs):
        m = xs[i] // STEP
        out[lo:c] = unit_rows[i][lo - m:c - m]
        lo = c
    return out

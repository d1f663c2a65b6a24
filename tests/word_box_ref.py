"""A numpy restatement of the word-box rule (retto_amd/csrc/word_boxes.h, include/retto_hip.h "word boxes").

Every f32 operation is a numpy float32 scalar operation in the header's order, so the results are comparable bit for bit;
the crop geometry (size, rotate270, homography) comes from the CPU oracle (oracle/ref_lib.py), and scale_and_clip is the
oracle's f64 one.
"""
import ctypes as C

import numpy as np

from oracle import ref_lib as R

f32 = np.float32
RAW_SPLIT, RAW_DIGIT, RAW_ALPHA, RAW_DOT, RAW_HYPHEN, RAW_CJK = range(6)
EFF_SPLIT, EFF_ALNUM, EFF_CJK = range(3)
KIND_CJK, KIND_ALNUM = 0, 1


def raw_class(entry: str) -> int:
    if entry == "":
        return RAW_SPLIT
    if entry == ".":
        return RAW_DOT
    if entry == "-":
        return RAW_HYPHEN
    if all("0" <= c <= "9" for c in entry):
        return RAW_DIGIT
    if all(("0" <= c <= "9") or ("A" <= c <= "Z") or ("a" <= c <= "z") for c in entry):
        return RAW_ALPHA
    if all(0x4E00 <= ord(c) <= 0x9FFF for c in entry):
        return RAW_CJK
    return RAW_SPLIT


def eff_classes(raw):
    """raw classes of the kept tokens in order -> effective classes"""
    n = len(raw)
    out = []
    for k, r in enumerate(raw):
        prev = out[-1] if k > 0 else EFF_SPLIT
        if r in (RAW_DIGIT, RAW_ALPHA):
            e = EFF_ALNUM
        elif r == RAW_CJK:
            e = EFF_CJK
        elif r == RAW_HYPHEN:
            e = EFF_ALNUM if (k > 0 and prev == EFF_ALNUM) else EFF_SPLIT
        elif r == RAW_DOT:
            e = EFF_ALNUM if (k > 0 and prev == EFF_ALNUM and k + 1 < n and raw[k + 1] == RAW_DIGIT) else EFF_SPLIT
        else:
            e = EFF_SPLIT
        out.append(e)
    return out


def segment(raw):
    """-> list of (first token, token count, kind) in token order"""
    eff = eff_classes(raw)
    words, a0 = [], None
    for k, e in enumerate(eff + [EFF_SPLIT]):
        if e != EFF_ALNUM and a0 is not None:
            words.append((a0, k - a0, KIND_ALNUM)); a0 = None
        if e == EFF_ALNUM and a0 is None:
            a0 = k
        if e == EFF_CJK:
            words.append((k, 1, KIND_CJK))
    return words


def crop_geometry(box_after):
    """(w, h, rot270, cw, ch, inv[9]) of a det box, pre-rotation dims, as the crop stage derives them."""
    b = np.ascontiguousarray(np.asarray(box_after, np.float32).reshape(8))
    ow, oh, r = C.c_int(), C.c_int(), C.c_int()
    cw, ch = C.c_float(), C.c_float()
    R.lib().orc_crop_dims(R.f32p(b), C.byref(ow), C.byref(oh), C.byref(r), C.byref(cw), C.byref(ch))
    rot = bool(r.value)
    w, h = (oh.value, ow.value) if rot else (ow.value, oh.value)
    _, inv = R.crop_projection(b)
    return w, h, rot, f32(cw.value), f32(ch.value), inv.reshape(9)


def span_to_quad(x0, x1, w_c, h_c, rot270, rot180, w, h, cw, ch, inv):
    wc = f32(w_c)
    x0 = min(max(f32(x0), f32(0)), wc)
    x1 = min(max(f32(x1), f32(0)), wc)
    if rot180:
        x0, x1 = wc - x1, wc - x0
    if not rot270:
        ua, ub, va, vb = x0, x1, f32(0), f32(h_c)
    else:
        va, vb, ua, ub = x0, x1, f32(0), f32(w)
    su, sv = cw / f32(w), ch / f32(h)
    Ua, Ub, Va, Vb = ua * su, ub * su, va * sv, vb * sv
    i = [f32(v) for v in inv]
    q = np.zeros(8, np.float32)
    for c, (U, V) in enumerate(((Ua, Va), (Ub, Va), (Ub, Vb), (Ua, Vb))):
        dd = i[6] * U + i[7] * V + i[8]
        q[2 * c] = (i[0] * U + i[1] * V + i[2]) / dd
        q[2 * c + 1] = (i[3] * U + i[4] * V + i[5]) / dd
    return q


def line_words(raw_of_id, tokens, cols, T, W, resized_w, box_after, rot180, after_w, after_h, ori_w, ori_h):
    """-> list of dicts {quad [8] f32 (original-image coordinates), first_token, n_tokens, first_col, last_col, kind}"""
    tokens = [int(t) for t in tokens]; cols = [int(c) for c in cols]
    n = len(tokens)
    if n == 0 or resized_w <= 0:
        return []
    w, h, rot, cw, ch, inv = crop_geometry(box_after)
    w_c, h_c = (h, w) if rot else (w, h)
    p = (f32(W) / f32(T)) * (f32(w_c) / f32(resized_w))
    raw = [raw_of_id[t] for t in tokens]
    eff = eff_classes(raw)
    dsum, runs, k = f32(0), 0, 0
    while k < n:
        if eff[k] != EFF_CJK:
            k += 1; continue
        j = k
        while j < n and eff[j] == EFF_CJK:
            j += 1
        m = j - k
        if m >= 2:
            dsum = dsum + (f32(cols[j - 1] - cols[k]) * p) / f32(m - 1); runs += 1
        k = j
    w_cjk = dsum / f32(runs) if runs else f32(w_c) / f32(n)
    out = []
    for a, cnt, kind in segment(raw):
        if kind == KIND_ALNUM:
            x0, x1 = f32(cols[a]) * p, f32(cols[a + cnt - 1] + 1) * p
        else:
            mid = (f32(cols[a]) + f32(0.5)) * p
            x0, x1 = mid - f32(0.5) * w_cjk, mid + f32(0.5) * w_cjk
        q = span_to_quad(x0, x1, w_c, h_c, rot, rot180, w, h, cw, ch, inv)
        q = R.scale_and_clip(q, after_w, after_h, ori_w, ori_h).reshape(8)
        out.append(dict(quad=q, first_token=a, n_tokens=cnt, first_col=cols[a], last_col=cols[a + cnt - 1], kind=kind))
    return out


def kept_columns(idx_row):
    """the CTC selection of one line's argmax row: (ids, columns) of the kept tokens"""
    ids, cols = [], []
    for t, v in enumerate(idx_row):
        if v != 0 and (t == 0 or v != idx_row[t - 1]):
            ids.append(int(v)); cols.append(t)
    return ids, cols


def split_free_text(dictionary, tokens, raw_of_id):
    """the rec text with the effective-SPLIT tokens removed"""
    raw = [raw_of_id[int(t)] for t in tokens]
    return "".join(dictionary[int(t)] for t, e in zip(tokens, eff_classes(raw)) if e != EFF_SPLIT)

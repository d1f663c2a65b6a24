"""Word boxes (rt_config.rec_return_word_box) on the CPU: rt_debug_word_boxes, which runs retto_amd/csrc/word_boxes.h on the
host, against the numpy restatement in word_box_ref.py, plus constructed cases of the rule.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, synth
from oracle import ref_lib as R
import word_box_ref as WR

PUNCT = list("!?,;:()[]/'\"@#%&*+=_") + ["。", "，", "é"]
CJK = [chr(0x4E00 + i) for i in range(0, 0x51FF, 97)] + ["鿿", "一"]


def _dict_bytes(entries):
    return ("\n".join(entries) + "\n").encode("utf-8")


def _debug(dic, tokens, cols, T, W, resized_w, box, rot180, after_w, after_h, ori_w, ori_h):
    """raw rt_debug_word_boxes: (rc, list of rt_word)"""
    lib = _lib.load()
    tok = np.ascontiguousarray(tokens, np.int32); col = np.ascontiguousarray(cols, np.int32)
    b = np.ascontiguousarray(np.asarray(box, np.float32).reshape(8))
    out = (_lib.Word * max(len(tok), 1))(); nw = C.c_int()
    P = C.POINTER
    rc = lib.rt_debug_word_boxes(dic, len(dic), tok.ctypes.data_as(P(C.c_int32)), col.ctypes.data_as(P(C.c_int32)), len(tok),
                                 T, W, resized_w, b.ctypes.data_as(P(C.c_float)), int(rot180), after_w, after_h, ori_w, ori_h,
                                 out, C.byref(nw))
    return rc, [out[j] for j in range(nw.value)]


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        q = np.array(list(g.quad), np.float32)
        assert np.array_equal(q.view(np.uint32), w["quad"].view(np.uint32)), (q, w["quad"])
        assert (g.first_token, g.n_tokens, g.first_col, g.last_col, g.kind) == \
            (w["first_token"], w["n_tokens"], w["first_col"], w["last_col"], w["kind"])


def _rot_box(cx, cy, bw, bh, ang):
    c, s = math.cos(ang), math.sin(ang)
    pts = [(-bw / 2, -bh / 2), (bw / 2, -bh / 2), (bw / 2, bh / 2), (-bw / 2, bh / 2)]
    return np.array([[cx + x * c - y * s, cy + x * s + y * c] for x, y in pts], np.float32)


def _random_dict(rng):
    pool = list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ") + list("0123456789") + [".", "-"] * 6 + PUNCT + CJK
    ents = [pool[int(rng.integers(len(pool)))] for _ in range(int(rng.integers(20, 120)))]
    ents += ["ab", "12", "a1", "中国", "a中", "1.", "", "x y"]   # multi-character entries, an empty line
    rng.shuffle(ents)
    return ents


# ---------------------------------------------------------------- the restatement equals the header, bit for bit
@pytest.mark.parametrize("seed", range(12))
def test_debug_word_boxes_fuzz_against_restatement(seed):
    rng = np.random.default_rng(1000 + seed)
    ents = _random_dict(rng)
    dic = _dict_bytes(ents)
    full = retto_amd.parse_dictionary(dic)
    raw_of_id = [WR.raw_class(e) for e in full]
    for case in range(40):
        W = int(rng.choice([320, 480, 640, 1024, 2000, 3648]))
        T = W // 8
        resized_w = W if rng.random() < 0.4 else int(rng.integers(1, W + 1))
        n = int(rng.integers(0, min(T, 60) + 1))
        cols = np.sort(rng.choice(T, n, replace=False)).astype(np.int32)
        tokens = rng.integers(1, len(full), n).astype(np.int32)
        after_w, after_h = int(rng.integers(600, 1400)), int(rng.integers(400, 1200))
        if rng.random() < 0.5:
            ori_w, ori_h = after_w, after_h
        else:
            ori_w, ori_h = int(rng.integers(100, 3000)), int(rng.integers(100, 3000))
        if rng.random() < 0.3:   # tall: the crop is rotated by 270 degrees
            bw, bh = float(rng.uniform(6, 40)), float(rng.uniform(70, 300))
        else:
            bw, bh = float(rng.uniform(20, 500)), float(rng.uniform(6, 60))
        ang = float(rng.uniform(-0.5, 0.5)) if rng.random() < 0.6 else 0.0
        box = _rot_box(float(rng.uniform(300, after_w - 300)), float(rng.uniform(160, after_h - 160)), bw, bh, ang)
        if rng.random() < 0.3:
            box = np.round(box).astype(np.float32)
        rot180 = bool(rng.random() < 0.4)
        rc, got = _debug(dic, tokens, cols, T, W, resized_w, box, rot180, after_w, after_h, ori_w, ori_h)
        assert rc == 0
        want = WR.line_words(raw_of_id, tokens, cols, T, W, resized_w, box, rot180, after_w, after_h, ori_w, ori_h)
        _assert_same(got, want)


def test_fuzz_covers_rot270_and_every_class():
    """the fuzz above reaches rotate270 boxes and dictionaries with every raw class"""
    rng = np.random.default_rng(1000)
    full = retto_amd.parse_dictionary(_dict_bytes(_random_dict(rng)))
    assert {WR.raw_class(e) for e in full} == set(range(6))
    assert WR.crop_geometry(_rot_box(300, 300, 20, 200, 0.1))[2]


# ---------------------------------------------------------------- constructed cases
MIXED = list("abcdefghijklmnopqrstuvwxyz") + list("0123456789") + [".", "-", "!", "中", "国", "人"]
MIXED_DICT = _dict_bytes(MIXED)
MIXED_FULL = ["blank"] + MIXED + [" "]
SPACE = len(MIXED_FULL) - 1
BOX = np.array([[100, 50], [500, 50], [500, 82], [100, 82]], np.float32)


def _ids(text):
    return [SPACE if ch == " " else MIXED_FULL.index(ch) for ch in text]


def _words(text, cols=None, T=80, W=640, resized_w=640, box=BOX, rot180=False, page=(1000, 600), ori=None):
    ids = _ids(text)
    cols = list(range(0, 2 * len(ids), 2)) if cols is None else cols
    ori = page if ori is None else ori
    w = retto_amd.debug_word_boxes(MIXED_DICT, ids, cols, T, W, resized_w, box, rot180, page[0], page[1], ori[0], ori[1])
    raw_of_id = [WR.raw_class(e) for e in MIXED_FULL]
    want = WR.line_words(raw_of_id, ids, cols, T, W, resized_w, box, rot180, page[0], page[1], ori[0], ori[1])
    assert [(x.first_token, x.n_tokens) for x in w] == [(d["first_token"], d["n_tokens"]) for d in want]
    for x, d in zip(w, want):
        assert np.array_equal(x.box.as_array().reshape(8), d["quad"])
    return w


@pytest.mark.parametrize("text", ["3.14", "v1.2-rc", "state-of-the-art", "ab-"])
def test_one_alnum_word(text):
    w = _words(text)
    assert [(x.text, x.kind) for x in w] == [(text, "alnum")]


@pytest.mark.parametrize("text,words", [("a.b", ["a", "b"]), ("a - b", ["a", "b"]), (".5", ["5"]), ("-a", ["a"]),
                                        ("1.", ["1"]), ("a!b", ["a", "b"]), ("x中y", ["x", "中", "y"])])
def test_splits(text, words):
    assert [x.text for x in _words(text)] == words


def test_each_cjk_character_gets_its_own_box():
    w = _words("中国人", cols=[3, 7, 11])
    assert [(x.text, x.kind) for x in w] == [("中", "cjk"), ("国", "cjk"), ("人", "cjk")]
    xs = [x.box.as_array()[:, 0] for x in w]
    assert xs[0].max() <= xs[1].min() + 1 and xs[1].max() <= xs[2].min() + 1   # left to right, abutting at pitch 4 columns
    assert all(a.max() > a.min() for a in xs)


def test_cjk_pitch_falls_back_to_crop_width_over_n():
    """no run of two CJK tokens: w_cjk = w_c / n.  Line of 400 x 32 crop pixels, 4 kept tokens -> 100 pixels per CJK word."""
    w = _words("中a国b", cols=[10, 20, 40, 60], T=80, W=640, resized_w=640, box=BOX)
    cj = [x for x in w if x.kind == "cjk"]
    assert len(cj) == 2
    for x in cj:
        xs = x.box.as_array()[:, 0]
        assert xs.max() - xs.min() == 100.0 or (xs.min() == 100.0 and xs.max() - xs.min() < 100.0)


def test_empty_and_all_split_lines_have_no_words():
    assert retto_amd.debug_word_boxes(MIXED_DICT, [], [], 80, 640, 640, BOX, False, 1000, 600, 1000, 600) == []
    assert _words(" ! . - ") == []
    assert _words("ab", resized_w=0) == []


@pytest.mark.parametrize("tall", [False, True])
@pytest.mark.parametrize("rot180", [False, True])
def test_whole_line_word_is_the_line_box(tall, rot180):
    """an ALNUM word over columns 0..T-1 with resized_w == W maps back to the line's own box (ori == after)"""
    box = np.array([[300, 100], [340, 110], [330, 370], [290, 360]], np.float32) if tall else \
        np.array([[100, 50], [520, 60], [518, 92], [98, 82]], np.float32)
    assert WR.crop_geometry(box)[2] == tall
    T, W = 60, 480
    text = "ab" * 30
    w = _words(text, cols=list(range(T)), T=T, W=W, resized_w=W, box=box, rot180=rot180)
    assert len(w) == 1
    line = R.scale_and_clip(box, 1000, 600, 1000, 600)
    assert np.array_equal(w[0].box.as_array(), line)


def test_rot180_puts_the_first_word_at_the_far_end():
    w0 = _words("ab cd", cols=[0, 1, 20, 40, 41], rot180=False)
    w1 = _words("ab cd", cols=[0, 1, 20, 40, 41], rot180=True)
    tl = BOX[0]
    d0 = np.linalg.norm(w0[0].box.as_array().mean(0) - tl)
    d1 = np.linalg.norm(w1[0].box.as_array().mean(0) - tl)
    assert d0 < d1 and np.linalg.norm(w1[0].box.as_array().mean(0) - BOX[2]) < d1


def test_ori_differs_from_after():
    w = _words("abc", page=(1000, 600), ori=(2000, 1200))
    w1 = _words("abc", page=(1000, 600))
    assert np.allclose(w[0].box.as_array(), 2 * w1[0].box.as_array(), atol=1)


def test_invalid_arguments():
    ids = _ids("ab")
    assert _debug(MIXED_DICT, ids, [3, 3], 80, 640, 640, BOX, 0, 1000, 600, 1000, 600)[0] == retto_amd.InvalidArgument.code
    assert _debug(MIXED_DICT, ids, [0, 80], 80, 640, 640, BOX, 0, 1000, 600, 1000, 600)[0] == retto_amd.InvalidArgument.code
    assert _debug(MIXED_DICT, [0, SPACE + 1], [0, 1], 80, 640, 640, BOX, 0, 1000, 600, 1000, 600)[0] == retto_amd.InvalidArgument.code


# ---------------------------------------------------------------- the class table
def _probe_class(dic, full, i):
    """the raw class the library gives entry i, observed through rt_debug_word_boxes (dic ends with probes "a", ".", "1")"""
    a, dot, one = len(full) - 4, len(full) - 3, len(full) - 2
    box = BOX

    def words(ids):
        rc, w = _debug(dic, ids, list(range(len(ids))), 80, 640, 640, box, 0, 1000, 600, 1000, 600)
        assert rc == 0
        return [(x.first_token, x.n_tokens, x.kind) for x in w]
    alone = words([i])
    if alone == [(0, 1, WR.KIND_CJK)]:
        return WR.RAW_CJK
    if alone == [(0, 1, WR.KIND_ALNUM)]:
        return WR.RAW_DIGIT if words([a, dot, i]) == [(0, 3, WR.KIND_ALNUM)] else WR.RAW_ALPHA
    assert alone == []
    if words([a, i]) == [(0, 2, WR.KIND_ALNUM)]:
        return WR.RAW_HYPHEN
    if words([a, i, one]) == [(0, 3, WR.KIND_ALNUM)]:
        return WR.RAW_DOT
    return WR.RAW_SPLIT


@pytest.mark.parametrize("which", ["mixed", "synthetic"])
def test_class_table(which):
    if which == "mixed":
        ents = MIXED + ["Ab9", "09", "中国", "中a", "", "　x", ". ", "--", "龥", "䷿", "ꀀ"]
    else:
        ents = synth.synth_dict().decode("utf-8").split("\n")[:-1]
    dic = _dict_bytes(ents + ["a", ".", "1"])
    full = retto_amd.parse_dictionary(dic)
    ids = list(range(len(full))) if which == "mixed" else list(range(0, len(full), 53)) + [len(full) - 1]
    for i in ids:
        assert _probe_class(dic, full, i) == WR.raw_class(full[i]), (i, full[i])
    assert full[-1] == " " and WR.raw_class(full[-1]) == WR.RAW_SPLIT
    if which == "synthetic":
        assert all(WR.raw_class(e) == WR.RAW_CJK for e in full[1:-4])


def test_config_field_is_last_and_defaults_off():
    from retto_amd._lib import Config
    assert Config._fields_[-1][0] == "rec_return_word_box"
    c = Config(); _lib.load().rt_config_default(C.byref(c))
    assert c.rec_return_word_box == 0 and c.struct_size == C.sizeof(Config)
    assert retto_amd.RecProcessorConfig().return_word_box is False
    assert retto_amd.RecProcessorSingleResult("", 0.0).words is None


def test_rt_create_rejects_other_values():
    """checked before any device is touched"""
    c = _lib.Config(); lib = _lib.load()
    lib.rt_config_default(C.byref(c))
    c.rec_return_word_box = 2
    h = C.c_void_p()
    assert lib.rt_create(C.byref(c), C.byref(h)) == retto_amd.InvalidArgument.code
    assert b"rec_return_word_box" in lib.rt_last_error(None)


def test_cli_flag():
    from retto_amd import cli
    assert cli.build_parser().parse_args(["-i", "x"]).rec_return_word_box is False
    assert cli.build_parser().parse_args(["-i", "x", "--rec-return-word-box"]).rec_return_word_box is True
